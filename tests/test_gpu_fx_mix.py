"""The fused mix-down of the effect banks (fdsp_bank_process_mix / fdsp_bank_process_mix_planar on reverb_stereo, reverb4_stereo, the
generic fdn, reverb3_stereo, the filtered / per-instance networks and the feedback delay banks) and of chains that end in one.

Bar: bit for bit.  The fused mix equals fdsp_sum_voices / fdsp_mix_stereo of the same bank's voice-minor render and the summation order's
numpy statement (tests/mix_order.py) applied to it; the planar entry gives the same bits; the state after a mix launch is the state after a
render; chunking the scratch, splitting the launch, the bus, a stream capture and sharding change nothing."""
import numpy as np
import pytest

import oracle as O
from mix_order import mix_order_reference
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MIX_PAN, MIX_SUM, MODE_PROCESS, MODE_TICK, _lib
from fundsp_amd import graph as GR
from test_gpu_fdn import delays_of
from test_gpu_fdn_network import params as network_params
from test_gpu_feedback_delay import params as feedback_params
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
SR = 48000.0
W2 = (0.55, 0.4)


def _at_rate(b):
    b.set_sample_rate(SR)
    return b


# every delay is at least 128 samples at 44.1 kHz and at 48 kHz (the constructor arguments of test_gpu_reverb / _fdn / _reverb3 / _fdn_network /
# _feedback_delay)
FAMILIES = {
    "reverb_stereo": lambda gpu, V: _at_rate(gpu.Bank.reverb_stereo(V, 10.0, 1.0, 0.5)),
    "reverb4_stereo": lambda gpu, V: _at_rate(gpu.Bank.reverb4_stereo(V, 20.0, 2.0)),
    "fdn8_2x2": lambda gpu, V: _at_rate(gpu.Bank.fdn(V, 8, delays_of(8), 2, W2, 2, 2)),
    "fdn8_1x1": lambda gpu, V: _at_rate(gpu.Bank.fdn(V, 8, delays_of(8), 2, W2, 1, 1)),
    "reverb3_lowpole": lambda gpu, V: _at_rate(gpu.Bank.reverb3_stereo(V, 2.0, 0.6, 1800.0)),
    "reverb3_svf": lambda gpu, V: _at_rate(gpu.Bank.reverb3_stereo(V, 1.8, 0.7, 3000.0, svf="lowpass", q=0.7)),
    "network_filtered": lambda gpu, V: gpu.Bank.fdn_network(V, 16, place="line", inputs=1, outputs=1, sample_rate=SR,
                                                            **network_params(16, V, "lowpass", 0, True, False, 16)),
    "network_per_instance": lambda gpu, V: gpu.Bank.fdn_network(V, 32, place="loop", inputs=2, outputs=2, sample_rate=SR,
                                                                **network_params(32, V, "lowpole", 3, True, True, 35)),
    # k_fb_frames<1, 2>: line form, lowpole, line gain and outer gain | k_fb_frames<2, 3>: loop form, reversed, every parameter per instance
    "feedback_delay_mono": lambda gpu, V: gpu.Bank.feedback_delay(V, sample_rate=SR, **feedback_params(1, "line", "lowpole", 2, True, True, False)),
    "feedback_delay_stereo": lambda gpu, V: gpu.Bank.feedback_delay(V, sample_rate=SR, **feedback_params(2, "loop", "lowpole", 3, True, False, True, V=V)),
}
V_GRID, T_GRID = (1, 5, 63, 64, 65, 64 * 3 + 21), (1, 64, 65, 64 * 5 + 9)
SUBSET = [(65, 64 * 5 + 9), (5, 65), (64 * 3 + 21, 64), (1, 1)]   # every family: a ragged second group over ragged blocks, fewer than a quarter


def noise(V, nin, T, seed):
    """seeded noise, planar [V][nin][T]"""
    rng = np.random.default_rng(seed)
    return (rng.random((V, nin, T), dtype=np.float32) * 2 - 1).astype(np.float32)


def dev(x, layout=LAYOUT_VOICE_MINOR, stride=None):
    """planar host [V][c][T] -> the device tensor of a layout (planar: rows of `stride` floats)"""
    import torch

    if layout == LAYOUT_VOICE_MINOR:
        return torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0))).cuda()
    V, c, T = x.shape
    p = np.zeros((V, c, stride or T), dtype=np.float32)
    p[:, :, :T] = x
    return torch.from_numpy(p).cuda()


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


WARM = 64 * 200   # frames: several trips around the longest line of any bank here (reverb4_stereo's two networks in series), so the mixes below are non-zero


def warm(b, x=None):
    """a bank in mid-tail: a fresh network answers the first frames with zeros, and equal zeros would prove nothing"""
    x = noise(b.voices, b.inputs(), WARM, 99) if x is None else x
    b.process(x.shape[2], dev(x))
    return b


def make(gpu, name, V):
    return warm(FAMILIES[name](gpu, V))


def check_family(gpu, name, V, T, mode):
    b = make(gpu, name, V)
    ref, pl = b.clone(), b.clone()
    x = noise(V, b.inputs(), T, 1000 * V + T)
    mix = host(b.process_mix(T, dev(x), mix=MIX_SUM, mode=mode))
    out = ref.process(T, dev(x), mode=mode)                                         # [outputs][T][V]
    assert mix.shape == (b.outputs(), T)
    assert_bit_equal(mix, host(gpu.sum_voices(out)), f"{name} V={V} T={T}: fused vs sum_voices(voice-minor render)")
    assert_bit_equal(mix, mix_order_reference(host(out)), f"{name} V={V} T={T}: fused vs the order's statement")
    stride = T if T % 2 else T + 3                                                  # planar rows at an odd offset from each other as well
    mp = host(pl.process_mix(T, dev(x, LAYOUT_PLANAR, stride), mix=MIX_SUM, mode=mode, layout=LAYOUT_PLANAR, frame_stride=stride))
    assert_bit_equal(mp, mix, f"{name} V={V} T={T}: the planar entry")
    # the state after a mix launch is the state after a render
    x2 = dev(noise(V, b.inputs(), 70, 7))
    nxt = host(ref.process(70, x2, mode=mode))
    assert_bit_equal(host(b.process(70, x2, mode=mode)), nxt, f"{name}: the next render after a voice-minor mix launch")
    assert_bit_equal(host(pl.process(70, x2, mode=mode)), nxt, f"{name}: the next render after a planar mix launch")
    assert b.get_option("has_fused_mix") == 1
    assert np.abs(mix).max(axis=1).min() > 0, "every channel sounds"


@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("V", V_GRID)
def test_reverb_stereo_over_the_whole_grid(gpu, V, T):
    check_family(gpu, "reverb_stereo", V, T, MODE_PROCESS)


@pytest.mark.parametrize("mode", [MODE_PROCESS, MODE_TICK])
@pytest.mark.parametrize("V,T", SUBSET)
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_every_family_mixes(gpu, name, V, T, mode):
    check_family(gpu, name, V, T, mode)


@pytest.mark.parametrize("name", ["fdn8_1x1", "network_filtered", "feedback_delay_mono"])
def test_mix_pan_on_mono_banks(gpu, name):
    import torch

    V, T = 70, 64 * 2 + 5
    pan = np.linspace(-1.2, 1.2, V).astype(np.float32)
    b = make(gpu, name, V)
    b.set_pan(pan)
    ref, pl = b.clone(), b.clone()
    x = noise(V, 1, T, 5)
    mix = host(b.process_mix(T, dev(x), mix=MIX_PAN))
    out = ref.process(T, dev(x))
    assert mix.shape == (2, T)
    assert_bit_equal(mix, host(gpu.mix_stereo(out[0], torch.from_numpy(pan).cuda())), f"{name}: MIX_PAN vs mix_stereo(out[0], pan)")
    assert_bit_equal(host(pl.process_mix(T, dev(x, LAYOUT_PLANAR), mix=MIX_PAN, layout=LAYOUT_PLANAR)), mix, f"{name}: MIX_PAN, the planar entry")
    assert np.abs(mix[0] - mix[1]).max() > 0


def test_mix_pan_on_a_stereo_bank_is_einval(gpu):
    b = make(gpu, "reverb_stereo", 3)
    with pytest.raises(gpu.FdspError) as e:
        b.process_mix(64, dev(noise(3, 2, 64, 1)), mix=MIX_PAN)
    assert e.value.code == _lib.EINVAL


@pytest.mark.parametrize("layout", [LAYOUT_VOICE_MINOR, LAYOUT_PLANAR])
def test_chunks_and_split_launches_change_no_bit(gpu, layout):
    V, T = 65, 64 * 4 + 9
    x = noise(V, 2, T, 21)
    kw = {"layout": layout}

    def run(chunk, cuts):
        b = make(gpu, "reverb_stereo", V)
        if chunk is not None:
            b.set_option("fx_mix_chunk_frames", chunk)
            assert b.get_option("fx_mix_chunk_frames") == chunk
        return np.concatenate([host(b.process_mix(e - a, dev(np.ascontiguousarray(x[:, :, a:e]), layout), **kw)) for a, e in zip(cuts[:-1], cuts[1:])], axis=1)

    auto = run(None, [0, T])
    assert_bit_equal(run(64, [0, T]), auto, "chunks of 64 frames vs the automatic chunking")
    assert_bit_equal(run(128, [0, T]), auto, "chunks of 128 frames vs the automatic chunking")
    assert_bit_equal(run(None, [0, 67, T]), auto, "launches of 67 and T - 67 frames vs one launch")
    assert_bit_equal(run(64, [0, 67, T]), auto, "... and both at once")
    b = FAMILIES["reverb_stereo"](gpu, V)   # (the option table's check; no launch)
    with pytest.raises(gpu.FdspError) as e:
        b.set_option("fx_mix_chunk_frames", 100)
    assert e.value.code == _lib.EINVAL


def test_the_mix_is_the_mix_of_the_bussed_output(gpu):
    V, T = 65, 64 * 2 + 9
    b = make(gpu, "reverb_stereo", V)
    b.set_bus(_lib.BUS_DRY_WET, wet=0.2, dry=1.0)
    ref, dry = b.clone(), make(gpu, "reverb_stereo", V)
    x = dev(noise(V, 2, T, 31))
    mix = host(b.process_mix(T, x))
    assert_bit_equal(mix, host(gpu.sum_voices(ref.process(T, x))), "bus (wet 0.2, dry 1.0): fused vs sum_voices of the bussed render")
    assert np.any(mix != host(dry.process_mix(T, x)))


def test_mix_of_the_oracles_own_instances(gpu):
    V, T, WARM = 8, 200, 64 * 70   # (reverb_stereo(10, ..): the longest line has 3 980 samples)
    x = noise(V, 2, WARM + T, 41)
    b = warm(FAMILIES["reverb_stereo"](gpu, V), np.ascontiguousarray(x[:, :, :WARM]))
    mix = host(b.process_mix(T, dev(np.ascontiguousarray(x[:, :, WARM:]))))
    want = np.zeros((2, T, V), dtype=np.float32)
    for v in range(V):
        n = O.reverb_stereo(10.0, 1.0, 0.5)   # the oracle node of tests/test_gpu_reverb.py
        n.set_sample_rate(SR)
        n.render_blocks(x[v][:, :WARM])
        want[:, :, v] = n.render_blocks(x[v][:, WARM:])
    assert np.abs(want).max(axis=(0, 1)).min() > 0   # every instance sounds
    assert_bit_equal(mix, mix_order_reference(want), "fused mix vs the order's statement over the oracle's instances")


def test_two_shards_add_up_to_the_one_bank(gpu):
    """the per-instance network: instances 0..63 and 64..127 as banks of their own are the two children of the tree's top node"""
    V, T, n = 128, 64 + 9, 32
    p = network_params(n, V, "lowpole", 3, True, True, 35)
    cut = lambda a, e: {k: (v[a:e] if isinstance(v, np.ndarray) and v.ndim == 2 and v.shape[0] == V else v) for k, v in p.items()}
    mk = lambda a, e: gpu.Bank.fdn_network(e - a, n, place="loop", inputs=2, outputs=2, sample_rate=SR, **cut(a, e))
    x, w = noise(V, 2, T, 51), noise(V, 2, WARM, 52)
    run = lambda a, e: host(warm(mk(a, e), np.ascontiguousarray(w[a:e])).process_mix(T, dev(np.ascontiguousarray(x[a:e]))))
    whole, lo, hi = run(0, V), run(0, 64), run(64, V)
    assert_bit_equal(lo + hi, whole, "the shards' mixes added once vs the one bank's mix")
    assert np.any(lo != hi)


def test_captured_mix_launches_and_the_refusal_without_a_reservation(gpu):
    import torch

    V, T = 65, 64 + 9
    b = make(gpu, "reverb_stereo", V)
    ref = b.clone()
    xs = [dev(noise(V, 2, T, 60 + k)) for k in range(3)]
    want = np.concatenate([host(ref.process_mix(T, xs[k])) for k in range(3)], axis=1)
    b.mix_reserve(T)
    outs = [torch.empty((2, T), dtype=torch.float32, device="cuda") for _ in range(3)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for k in range(3):
                b.process_mix(T, xs[k], out=outs[k])
        g.replay()
    torch.cuda.synchronize()
    assert_bit_equal(np.concatenate([host(o) for o in outs], axis=1), want, "three captured mix launches, replayed, vs three plain ones")
    fresh, twin = make(gpu, "reverb_stereo", V), make(gpu, "reverb_stereo", V)
    with torch.cuda.stream(s):
        g2 = torch.cuda.CUDAGraph()
        with pytest.raises(gpu.FdspError) as e:
            with torch.cuda.graph(g2, stream=s):
                fresh.process_mix(T, xs[0], out=outs[0])
    assert e.value.code == _lib.EINVAL and "fdsp_bank_mix_reserve" in str(e.value)
    torch.cuda.synchronize()
    assert_bit_equal(host(fresh.process_mix(T, xs[0])), host(twin.process_mix(T, xs[0])), "the refused bank mixes correctly afterwards")


def test_a_voice_bank_refuses_the_planar_entry(gpu):
    import torch
    from fundsp_amd import workloads as W

    b = W.make_fm_svf_bank(64, SR, params=W.fm_svf_params(64, SR))
    out = torch.empty((1, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(gpu.FdspError) as e:
        b.process_mix(64, mix=MIX_SUM, out=out, layout=LAYOUT_PLANAR)
    assert e.value.code == _lib.ENOTSUP


def chain_mix_checks(gpu, ch, mix, pan, V, T):
    import torch

    for layout in (LAYOUT_VOICE_MINOR, LAYOUT_PLANAR):
        a, r = ch.clone(), ch.clone()
        if pan is not None:
            a.set_pan(pan)
        got = host(a.process_mix(T, mix=mix, layout=layout))
        out = r.process(T, layout=layout)
        torch.cuda.synchronize()
        vm = out if layout == LAYOUT_VOICE_MINOR else out[:, :, :T].permute(1, 2, 0).contiguous()      # [outputs][T][V]
        want = gpu.sum_voices(vm) if mix == MIX_SUM else gpu.mix_stereo(vm[0], torch.from_numpy(pan).cuda())
        assert_bit_equal(got, host(want), f"chain.process_mix vs the mix of chain.clone().process, layout {layout}")
        assert np.abs(got).max() > 0
    # captured after mix_reserve: the mid buffer, the partials and the scratch exist
    a, r = ch.clone(), ch.clone()
    if pan is not None:
        a.set_pan(pan); r.set_pan(pan)
    want = host(r.process_mix(T, mix=mix))
    a.mix_reserve(T)
    out = torch.empty((2, T), dtype=torch.float32, device="cuda")
    a.clone().process_mix(T, mix=mix)          # the source's kernels are loaded outside the capture
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            a.process_mix(T, mix=mix, out=out, stream=s.cuda_stream)
        g.replay()
    torch.cuda.synchronize()
    assert_bit_equal(host(out), want, "a captured chain.process_mix after mix_reserve")


def test_chain_of_noise_into_reverb_stereo_mixes(gpu):
    V, T = 70, 64 * 2 + 9
    ch = gpu.Bank.from_graph((GR.noise() | GR.noise()) >> GR.reverb_stereo(10.0, 1.0, 0.5), V, sample_rate=SR)
    assert isinstance(ch, gpu.Chain) and ch.effect.kind == "reverb_stereo"
    ch.process(WARM)
    assert all(hasattr(ch, m) for m in ("process_mix", "set_pan", "mix_reserve"))
    chain_mix_checks(gpu, ch, MIX_SUM, None, V, T)


def test_chain_of_a_mono_front_into_the_mono_fdn_pans(gpu):
    V, T = 70, 64 * 2 + 9
    ch = gpu.Chain(gpu.Bank.from_graph(GR.noise(), V, sample_rate=SR), FAMILIES["fdn8_1x1"](gpu, V))
    ch.process(WARM)
    chain_mix_checks(gpu, ch, MIX_PAN, np.linspace(-1.2, 1.2, V).astype(np.float32), V, T)
