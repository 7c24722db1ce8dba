"""reverb4_stereo_delays banks with a delay table per instance (fdsp_reverb4_stereo_delays_create, Bank.reverb4_stereo_delays, Bank.set_delays):
bit-exact against tests/oracle.py's reverb4_stereo_delays, one oracle graph per instance.

Three instances with three tables drawn from the search range of examples/optimize.rs (0.030-0.070 s): one with a delay of exactly 128 samples
(the kernel's shortest), one with the longest delay of the bank (8 100 samples: the rings have 8 192 slots), one with equal delays inside a
network and across the two.  T = 2 x ring capacity + 37 frames of noise: the rings wrap twice and the last block is ragged."""
import numpy as np
import pytest

import oracle as O
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MIX_SUM, MODE_PROCESS, MODE_TICK, _lib
from mix_order import mix_order_reference
from test_gpu_fdn import run
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
SR = 44100.0
CAP = 8192                      # slots per ring at 44.1 kHz: the power of two above max(8 100, 0.105 s x 44 100 = 4 631) + 1
T = 2 * CAP + 37
TIME = 2.0


def tables():
    rng = np.random.default_rng(4)
    d = (0.030 + 0.040 * rng.random((3, 32))).astype(np.float32)
    d[0, 5] = np.float32(128.0 / SR)            # exactly 128 samples
    d[1, 23] = np.float32(8100.0 / SR)          # the longest delay of the bank, in the second network
    d[2, 2] = d[2, 1]                           # two equal delays in one network ...
    d[2, 20] = d[2, 3]                          # ... and one in each
    assert int(np.round(np.float64(d[0, 5]) * SR)) == 128 and int(np.round(np.float64(d[1, 23]) * SR)) == 8100
    return d


def noise(V, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((V, 2, n), dtype=np.float32) * 2 - 1).astype(np.float32)


def oracle_node(row, time=TIME, sr=SR):
    n = O.reverb4_stereo_delays([float(x) for x in row], time)
    n.set_sample_rate(sr)
    return n


def oracle_render(node, x, mode=MODE_PROCESS):
    return node.render_blocks(x) if mode == MODE_PROCESS else node.render_ticks(x)


_REF = {}


def reference(mode):
    """the three oracle graphs over the whole input, computed once per executor and left unchanged"""
    if mode not in _REF:
        d, x = tables(), noise(3, T, 11)
        _REF[mode] = np.stack([oracle_render(oracle_node(d[v]), x[v], mode) for v in range(3)])
        _REF[mode].setflags(write=False)
    return _REF[mode]


def make(gpu, V=3):
    d = tables()
    b = gpu.Bank.reverb4_stereo_delays(V, d[np.arange(V) % 3], TIME)
    assert b.kind == "reverb4_stereo" and b.inputs() == 2 and b.outputs() == 2
    return b


@pytest.mark.parametrize("mode", [MODE_PROCESS, MODE_TICK])
@pytest.mark.parametrize("layout", [LAYOUT_PLANAR, LAYOUT_VOICE_MINOR])
def test_three_tables_match_the_oracle(gpu, layout, mode):
    want = reference(mode)
    got = run(make(gpu), noise(3, T, 11), layout, mode, [0, T])
    for v in range(3):
        assert_bit_equal(got[v], want[v], f"instance {v}")
    assert np.abs(want).max(axis=(1, 2)).min() > 0.01


def test_a_split_launch_equals_the_whole(gpu):
    cuts = [0, 64 * 3 + 1, 64 * 100 + 37, 64 * 200 + 37 + 5, T]   # 64 k + odd: every later launch starts a block in mid-ring
    got = run(make(gpu), noise(3, T, 11), LAYOUT_PLANAR, MODE_PROCESS, cuts)
    # (the oracle's process() of the whole input: FDN graphs tick inside process, so block boundaries change nothing there either)
    assert_bit_equal(got, reference(MODE_PROCESS), "split launch")


def test_one_stock_table_for_the_bank_is_reverb4_stereo(gpu):
    """per_instance = 0: reverb4_stereo(10, time) scales the stock table by max(10, 15) / 10 in f32 (prelude.rs:1909-1913)"""
    n = 64 * 150 + 13
    d = np.array(O.REVERB4_DELAYS, dtype=np.float32) * (np.float32(15.0) / np.float32(10.0))
    x = noise(3, n, 5)
    a = gpu.Bank.reverb4_stereo_delays(3, d, TIME)
    b = gpu.Bank.reverb4_stereo(3, 10.0, TIME)
    ya, yb = run(a, x, LAYOUT_PLANAR, MODE_PROCESS, [0, n]), run(b, x, LAYOUT_PLANAR, MODE_PROCESS, [0, n])
    assert_bit_equal(ya, yb, "table bank vs the uniform bank")
    ref = O.reverb4_stereo(10.0, TIME)
    ref.set_sample_rate(SR)
    assert_bit_equal(ya[1], ref.render_blocks(x[1]), "the oracle's stock graph")
    assert np.abs(ya).max() > 0.01


def test_sample_rate_change_in_mid_tail(gpu):
    """every row is re-derived; the lines restart empty, the FIRs and the feedback go on (Delay / Fir / Feedback::set_sample_rate); a rate at
    which a delay falls under 128 samples is refused and changes nothing"""
    d, n0, n1 = tables(), 64 * 120 + 9, 64 * 150 + 21
    x = noise(3, n0 + n1, 7)
    b = make(gpu)
    got0 = run(b, x[:, :, :n0], LAYOUT_PLANAR, MODE_PROCESS, [0, n0])
    with pytest.raises(gpu.FdspError):
        b.set_sample_rate(30000.0)              # the 128-sample delay would be 87
    b.set_sample_rate(48000.0)
    got1 = run(b, x[:, :, n0:], LAYOUT_PLANAR, MODE_PROCESS, [0, n1])
    for v in range(3):
        node = oracle_node(d[v])
        assert_bit_equal(got0[v], node.render_blocks(x[v][:, :n0]), f"instance {v} at 44.1 kHz")
        node.set_sample_rate(48000.0)
        assert_bit_equal(got1[v], node.render_blocks(x[v][:, n0:]), f"instance {v} after the change to 48 kHz")
    assert np.abs(got1[:, :, :64]).max() > 0     # the FIR history and the feedback value sound on


def test_clone_in_mid_stream(gpu):
    n0 = 64 * 130 + 3
    x = noise(3, T, 11)
    b = make(gpu)
    run(b, x[:, :, :n0], LAYOUT_PLANAR, MODE_PROCESS, [0, n0])
    c = b.clone()
    rest = reference(MODE_PROCESS)[:, :, n0:]
    assert_bit_equal(run(c, x[:, :, n0:], LAYOUT_PLANAR, MODE_PROCESS, [0, T - n0]), rest, "the clone")
    assert_bit_equal(run(b, x[:, :, n0:], LAYOUT_PLANAR, MODE_PROCESS, [0, T - n0]), rest, "the original")


def test_set_delays_resets_that_instance_only(gpu):
    d, n0, n1 = tables(), 64 * 110 + 5, 64 * 140 + 11
    x = noise(3, n0 + n1, 13)
    a, twin = make(gpu), make(gpu)
    for b in (a, twin):
        run(b, x[:, :, :n0], LAYOUT_PLANAR, MODE_PROCESS, [0, n0])
    row = (d[1] * np.float32(0.5) + np.float32(0.01)).astype(np.float32)
    a.set_delays(row, first=1)
    ya = run(a, x[:, :, n0:], LAYOUT_PLANAR, MODE_PROCESS, [0, n1])
    yt = run(twin, x[:, :, n0:], LAYOUT_PLANAR, MODE_PROCESS, [0, n1])
    assert_bit_equal(ya[[0, 2]], yt[[0, 2]], "the instances whose rows stay go on like the untouched twin's")
    assert_bit_equal(ya[1], oracle_node(row).render_blocks(x[1][:, n0:]), "the instance with the new row starts like a fresh graph")
    assert np.abs(yt[1, :, :64]).max() > 0 and np.abs(ya[1, :, :1000]).max() == 0.0


def test_set_bus(gpu):
    n = 64 * 120 + 7
    x = np.ascontiguousarray(noise(3, T, 11)[:, :, :n])     # the head of the reference's input
    b = make(gpu)
    b.set_bus(_lib.BUS_DRY_WET, wet=0.25, dry=0.5)
    got = run(b, x, LAYOUT_PLANAR, MODE_PROCESS, [0, n])
    y = reference(MODE_PROCESS)[:, :, :n]
    assert_bit_equal(got, np.float32(0.5) * x + np.float32(0.25) * y, "dry * multipass() & wet * reverb")


def test_fused_mix_equals_the_sum_of_the_instances(gpu):
    import torch

    V, warm, n = 65, 64 * 100, 192
    b = make(gpu, V)
    xw, x = noise(V, warm, 21), noise(V, n, 22)
    b.process(warm, torch.from_numpy(xw).cuda(), layout=LAYOUT_PLANAR, frame_stride=warm)   # (a fresh network answers with zeros)
    c = b.clone()
    xi = torch.from_numpy(x).cuda()
    mix = b.process_mix(n, xi, mix=MIX_SUM, layout=LAYOUT_PLANAR, frame_stride=n)
    out = c.process(n, xi, layout=LAYOUT_PLANAR, frame_stride=n)
    tree = gpu.sum_instances(out)
    torch.cuda.synchronize()
    mix, out, tree = mix.cpu().numpy(), out.cpu().numpy(), tree.cpu().numpy()
    # The fused mix adds the instances in the mix-down's documented order (include/fundsp_hip.h; tests/mix_order.py: quarters of 16 one after the
    # other, then trees) -- for every family (tests/test_gpu_fx_mix.py) -- and sum_instances in a plain binary tree: the same sum of the same
    # bit-exact terms in two fixed orders.  Bit for bit against the order the mix states; against the tree within both orders' rounding:
    # at most 18 and 7 additions deep, so 25 * 2^-24 * sum |x|.
    assert_bit_equal(mix, mix_order_reference(out.transpose(1, 2, 0)), "process_mix(MIX_SUM) vs the instances' process output added in the mix-down's order")
    assert np.all(np.abs(mix.astype(np.float64) - tree) <= 25 * 2.0 ** -24 * np.abs(out.astype(np.float64)).sum(axis=0)), "process_mix(MIX_SUM) vs sum_instances(process)"
    assert np.abs(mix).max(axis=1).min() > 0


def test_refusals(gpu):
    d = tables()
    bad = d.copy()
    bad[2, 9] = np.float32(127.0 / SR)
    with pytest.raises(gpu.FdspError, match="128 samples"):
        gpu.Bank.reverb4_stereo_delays(3, bad, TIME)
    bad = d.copy()
    bad[1, 0] = np.nan
    with pytest.raises(gpu.FdspError, match="not a number"):
        gpu.Bank.reverb4_stereo_delays(3, bad, TIME)
    bad = d.copy()
    bad[0, 31] = -0.01
    with pytest.raises(gpu.FdspError):
        gpu.Bank.reverb4_stereo_delays(3, bad, TIME)
    b = make(gpu)
    row = d[0].copy()
    row[4] = np.float32(0.2)                    # 8 820 samples: beyond the 8 192 slots
    with pytest.raises(gpu.FdspError, match="larger ring"):
        b.set_delays(row, first=2)
    with pytest.raises(gpu.FdspError):
        b.set_delays(d, first=1)                # rows out of range
    with pytest.raises(gpu.FdspError):
        gpu.Bank.reverb4_stereo(2, 20.0, 2.0).set_delays(d[0])   # not such a bank
    # nothing changed: the bank renders its own tables
    n = 64 * 60 + 1
    assert_bit_equal(run(b, noise(3, T, 11)[:, :, :n], LAYOUT_PLANAR, MODE_PROCESS, [0, n]), reference(MODE_PROCESS)[:, :, :n], "after the refusals")
