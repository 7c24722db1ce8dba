"""GPU parity of the convolver banks (fdsp_convolve_create, Bank.convolve, convolve(..) in Bank.from_graph): every output bit-exact against
the numpy restatement tests/convolve_ref.py -- response lengths around the partition edges and up to 48 000 taps, 1 / 2 / 8 channels, shared
and per-instance responses, 1 / 3 / 2048 instances, ragged launches, both layouts and executors, a launch of several chunks, reset, clone,
set_sample_rate, set_response, a captured launch replayed, subnormal inputs through the IEEE and flush-to-zero builds, chains from graphs
against the oracle's generators, and invalid specs."""
import numpy as np
import pytest

import convolve_ref as CR
import oracle as O
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from fundsp_amd import graph as GR
from test_gpu_parity import assert_bit_equal, oracle_render, run_bank

pytestmark = pytest.mark.gpu
B0 = 64


def signal(V, C, T, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (V, C, T)).astype(np.float32)


def response(shape, M, seed):
    rng = np.random.default_rng(seed + 1000)
    return (rng.uniform(-1.0, 1.0, tuple(shape) + (M,)) * np.exp(-np.arange(M) / (M / 5 + 1))).astype(np.float32)


def same_bits(got, want, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: first differences at {np.argwhere(got != want)[:4].tolist()}"


@pytest.mark.parametrize("M", [1, 3, B0 - 1, B0, B0 + 1, 5 * B0 + 17, 600, 2049])
@pytest.mark.parametrize("channels", [1, 2, 8])
@pytest.mark.parametrize("per", [False, True])
def test_matrix_bit_exact(gpu, M, channels, per):
    """B = 64 up to 512 taps, 128 at 600 (5 partitions), 256 at 2049 (9 partitions, the last one tap long)"""
    import fundsp_amd as F

    V = 3
    B = CR.block_length(M)
    T = M + 3 * B + 11
    x = signal(V, channels, T, seed=M + channels)
    h = response((V, channels) if per else (channels,), M, seed=M)
    b = F.Bank.convolve(V, h, per_instance=per)
    assert (b.inputs(), b.outputs(), b.kind, b.block_length) == (channels, channels, "convolve", B)
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x, h), f"M={M} C={channels} per_instance={per}")


def test_long_response_48000_taps(gpu):
    """48 000 taps: B = 1024, 47 partitions; one instance of three checked, 52 000 frames in one launch"""
    import fundsp_amd as F

    M, V, T = 48000, 3, 52000
    x = signal(V, 1, T, seed=1)
    h = response((V, 1), M, seed=2)
    b = F.Bank.convolve(V, h, per_instance=True)
    assert b.block_length == 1024
    got = run_bank(b, x, T, LAYOUT_PLANAR, MODE_PROCESS)
    same_bits(got[1:2], CR.render(x[1:2], h[1:2]), "48000 taps")
    y64 = np.convolve(x[1, 0].astype(np.float64), h[1, 0].astype(np.float64))[:T]
    assert np.abs(got[1, 0] - y64).max() / (np.abs(h[1, 0]).sum() * np.abs(x[1, 0]).max()) <= 4 * 1.01e-7, "the bound of tests/test_convolve_ref.py"


@pytest.mark.parametrize("V", [1, 2048])
def test_instances_one_and_many(gpu, V):
    import fundsp_amd as F

    M, T = 200, 500
    for per in (False, True):
        x = signal(V, 2, T, seed=5)
        h = response((V, 2) if per else (2,), M, seed=6)
        b = F.Bank.convolve(V, h, per_instance=per)
        same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x, h), f"V={V} per_instance={per}")


@pytest.mark.parametrize("layout", [LAYOUT_VOICE_MINOR, LAYOUT_PLANAR])
def test_ragged_launches_layouts_and_executors(gpu, layout):
    import fundsp_amd as F

    M, V = 200, 3
    lens = [1, 63, 64, B0 - 1, B0, B0 + 5, 3 * B0 + 7]
    T = sum(lens)
    x = signal(V, 2, T, seed=9)
    h = response((2,), M, seed=9)
    want = CR.render(x, h)
    for mode in (MODE_PROCESS, MODE_TICK):
        b = F.Bank.convolve(V, h)
        parts, t0 = [], 0
        for n in lens:
            parts.append(run_bank(b, np.ascontiguousarray(x[:, :, t0:t0 + n]), n, layout, mode))
            t0 += n
        same_bits(np.concatenate(parts, axis=2), want, f"mode {mode}: ragged launches")
    b = F.Bank.convolve(V, h)
    got = np.concatenate([run_bank(b, np.ascontiguousarray(x[:, :, t:t + 1]), 1, layout, MODE_TICK) for t in range(150)], axis=2)
    same_bits(got, want[:, :, :150], "sample by sample")


def test_long_launch_spans_several_chunks(gpu):
    """B = 64 and 64 blocks per chunk: 10 000 frames are rendered in 3 chunks (and 7 tail groups of 8 boundaries each plus a ragged one)"""
    import fundsp_amd as F

    M, V, T = 100, 3, 10000
    x = signal(V, 1, T, seed=3)
    h = response((1,), M, seed=3)
    b = F.Bank.convolve(V, h)
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x, h), "3 chunks")
    more = signal(V, 1, 77, seed=4)   # the state after the chunks is the state after the samples
    same_bits(run_bank(b, more, 77, LAYOUT_PLANAR, MODE_PROCESS), CR.render(np.concatenate([x, more], axis=2), h)[:, :, T:], "after the chunks")


def test_reset_clone_and_sample_rate(gpu):
    import fundsp_amd as F

    M, V, T1, T2 = 300, 3, 333, 280
    x = signal(V, 2, T1 + T2, seed=11)
    h = response((V, 2), M, seed=11)
    x1, x2 = np.ascontiguousarray(x[:, :, :T1]), np.ascontiguousarray(x[:, :, T1:])
    b = F.Bank.convolve(V, h, per_instance=True, max_len=1000, flush_denormals=True)
    run_bank(b, x1, T1, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    c = b.clone()
    assert (c.kind, c.max_len, c.block_length, c.per_instance) == ("convolve", 1000, 128, True)
    b.set_sample_rate(96000.0)   # Convolver has no set_sample_rate override: nothing moves
    want = CR.render(x, h, max_len=1000)
    same_bits(run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS), want[:, :, T1:], "after set_sample_rate")
    same_bits(run_bank(c, x2, T2, LAYOUT_PLANAR, MODE_PROCESS), want[:, :, T1:], "the clone continues in mid-stream")
    c.set_response(h[:, :, :40])   # (the clone carries the capacity and the per-instance rows)
    same_bits(run_bank(c, x2, T2, LAYOUT_PLANAR, MODE_PROCESS), CR.render(x2, h[:, :, :40], max_len=1000), "the clone takes a new response")
    b.reset()
    same_bits(run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x2, h, max_len=1000), "reset clears the history")


def test_set_response_between_launches(gpu):
    """shorter, longer up to the capacity, some rows of a per-instance bank; the history is cleared every time"""
    import fundsp_amd as F
    from fundsp_amd import FdspError

    V, cap, T = 3, 700, 450
    x = signal(V, 1, T, seed=21)
    h0 = response((1,), 300, seed=21)
    b = F.Bank.convolve(V, h0, max_len=cap)
    assert b.block_length == CR.block_length(cap) == 128
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x, h0, max_len=cap), "creation response")
    for M in (5, cap, 129):
        h = response((1,), M, seed=M)
        b.set_response(h)
        same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x, h, max_len=cap), f"set_response to {M} taps")
    with pytest.raises(FdspError, match="max_len"):
        b.set_response(np.ones(cap + 1, np.float32))
    hv = response((V, 1), 200, seed=23)
    p = F.Bank.convolve(V, hv, per_instance=True, max_len=cap)
    run_bank(p, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    new = response((1, 1), 200, seed=24)
    p.set_response(new, first=1)
    hv2 = hv.copy()
    hv2[1] = new[0]
    same_bits(run_bank(p, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x, hv2, max_len=cap), "row 1 replaced, the whole bank starts over")
    with pytest.raises(FdspError, match="one response length"):
        p.set_response(new[:, :, :100], first=1)
    with pytest.raises(FdspError, match="rows out of range"):
        p.set_response(new, first=3)
    with pytest.raises(ValueError):
        F.Bank.resynth(2, 64).set_response(new)


def test_captured_launch_replays(gpu):
    """A 64-frame launch captured on a caller's stream and replayed across several block boundaries (B = 128: one every second replay);
    a set_response in between is followed by the replay (the lengths live on the device)"""
    import torch

    import fundsp_amd as F

    M, V, T = 600, 5, 64
    reps = 9
    x = signal(V, 1, T * (reps + 1), seed=13)
    h = response((1,), M, seed=13)
    b = F.Bank.convolve(V, h)
    assert b.block_length == 128
    head = run_bank(b, np.ascontiguousarray(x[:, :, :T]), T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    inp = torch.zeros((1, T, V), dtype=torch.float32, device="cuda")
    out = torch.zeros((1, T, V), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.process(T, inp, out)

    def replay(lo, n):
        parts = []
        for r in range(lo, lo + n):
            inp.copy_(torch.from_numpy(np.ascontiguousarray(x[:, :, T * r:T * (r + 1)].transpose(1, 2, 0))))
            g.replay()
            torch.cuda.synchronize()
            parts.append(out.cpu().numpy().transpose(2, 0, 1).copy())
        return np.concatenate(parts, axis=2)

    got = np.concatenate([head, replay(1, reps)], axis=2)
    same_bits(got, CR.render(x, h), "captured launch, replayed")
    h2 = response((1,), 77, seed=14)
    b.set_response(h2)
    same_bits(replay(0, 5), CR.render(x[:, :, :5 * T], h2, max_len=M), "replays after set_response")


def test_subnormal_inputs_ieee_and_flushed(gpu):
    import fundsp_amd as F

    M, V, T = 150, 2, 400
    x = signal(V, 1, T, seed=17)
    x[0] *= np.float32(2.0 ** -130)   # instance 0: subnormal input samples
    x[1] *= np.float32(2.0 ** -122)   # instance 1: normal samples whose products with the taps fall into the denormal range
    h = response((1,), M, seed=17)
    assert np.any((np.abs(x) < np.float32(2.0 ** -126)) & (x != 0))
    for ftz in (False, True):
        b = F.Bank.convolve(V, h, flush_denormals=ftz)
        want = CR.render(x, h, ftz=ftz)
        got = run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
        same_bits(got, want, f"ftz={ftz}")
        if not ftz:
            assert np.any(got[0] != 0), "IEEE build: the denormal input comes through"
        else:
            assert not np.any(got[0]), "flushed build: a denormal input reads as zero"


def test_chains_from_graphs_against_the_oracle(gpu):
    """noise() >> convolve(h) and (noise() | noise()) >> (convolve(h0) | convolve(h1)) as Chains whose front is seeded from the Pipe's
    construction hash, into which Convolver::ID = 100 enters; and the two halves of the reference's check_wave case (test_basic.rs:329-330),
    noise() >> convolve([1.0, 0.9, 0.8]) and pink() >> convolve([0.5, 0.4, 0.3]), in both executors: equal bits (the reference asks 1e-4)"""
    import torch

    import fundsp_amd as F
    from fundsp_amd.bank import PIPE_ID, atto, probe_hash

    T = 1000
    h0, h1 = response((), 300, seed=31), response((), 170, seed=32)
    w = np.zeros((2, 300), np.float32)
    w[0], w[1, :170] = h0, h1
    g = GR.noise() >> GR.convolve(h0)
    hn = atto(atto(np.uint64(PIPE_ID), PIPE_ID), 20)   # Pipe::new: ping(true, AttoHash::new(Pipe::ID)); Noise::ID = 20, Convolver::ID = 100
    assert probe_hash(g) == int(atto(hn, 100))
    g2 = (GR.noise() | GR.noise()) >> (GR.convolve(w, 0) | GR.convolve(h1))
    cases = ((g, h0[None], lambda: O.noise(), (MODE_PROCESS,)), (g2, w, lambda: O.noise() | O.noise(), (MODE_PROCESS,)),
             (GR.noise() >> GR.convolve([1.0, 0.9, 0.8]), np.array([[1.0, 0.9, 0.8]], np.float32), lambda: O.noise(), (MODE_PROCESS, MODE_TICK)),
             (GR.pink() >> GR.convolve([0.5, 0.4, 0.3]), np.array([[0.5, 0.4, 0.3]], np.float32), lambda: O.pink(), (MODE_PROCESS, MODE_TICK)))
    for graph, h, mk, modes in cases:
        for mode in modes:
            ch = F.Bank.from_graph(graph, 2)
            assert isinstance(ch, F.Chain) and ch.effect.kind == "convolve"
            out = ch.process(T, mode=mode)
            torch.cuda.synchronize()
            got = out.cpu().numpy().transpose(2, 0, 1)
            n = mk()
            n.set_seed(int(atto(np.uint64(probe_hash(graph)), PIPE_ID)))
            x = oracle_render(n, None, T, mode)
            want = CR.render(x[None], h)[0]
            for v in range(2):
                assert_bit_equal(got[v], want, f"{graph.type} mode {mode}, instance {v}")
    # the node alone and a stack of nodes are banks; a stack of chains is refused
    b = F.Bank.from_graph(GR.convolve(w, 0) | GR.convolve(w, 1), 3)
    assert isinstance(b, F.Bank) and b.kind == "convolve" and b.outputs() == 2
    x = signal(3, 2, 400, seed=33)
    same_bits(run_bank(b, x, 400, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x, w), "stack of convolvers")
    with pytest.raises(ValueError, match="front >> convolve"):
        F.Bank.from_graph((GR.noise() >> GR.convolve([1.0, 0.9, 0.8])) | (GR.pink() >> GR.convolve([0.5, 0.4, 0.3])), 2)


def test_invalid_specs_and_unsupported_calls(gpu):
    import ctypes as C

    import fundsp_amd as F
    from fundsp_amd import _lib

    L = _lib.lib()
    h = np.ones(16, np.float32)
    fp = h.ctypes.data_as(C.POINTER(C.c_float))
    for kw, msg in ((dict(channels=9), b"channels"), (dict(len=17), b"len = 17"), (dict(per_instance=3), b"per_instance"), (dict(max_len=0), b"max_len")):
        s = _lib.ConvolveSpec()
        s.channels, s.max_len, s.len, s.per_instance = kw.get("channels", 1), kw.get("max_len", 16), kw.get("len", 16), kw.get("per_instance", 0)
        s.response = fp
        out = C.c_void_p()
        assert L.fdsp_convolve_create(4, C.byref(s), C.byref(out)) == _lib.EINVAL and not out.value
        assert msg in L.fdsp_last_error(), L.fdsp_last_error()
    b = F.Bank.convolve(2, h)
    assert L.fdsp_bank_set_bus(b._h, _lib.BUS_WET, 0.5, 1.0) == _lib.ENOTSUP
    assert L.fdsp_bank_get_bus(b._h, None, None, None) == _lib.ENOTSUP
    out = C.c_void_p()
    assert L.fdsp_bank_process_mix(b._h, 64, None, out, _lib.MIX_SUM, 0, None) == _lib.ENOTSUP
    assert L.fdsp_convolve_set_response(F.Bank.resynth(2, 64)._h, fp, 16, 0, 1) == _lib.EINVAL
    assert b"not a convolver bank" in L.fdsp_last_error()
