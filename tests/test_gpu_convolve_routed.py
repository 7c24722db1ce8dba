"""GPU parity of the routed convolver banks (fdsp_convolve_routed_create, Bank.convolve(.., source=..), `a ^ b` in Bank.from_graph): one input
through several responses.  A routed bank shares the input side among the outputs of one input and changes no operation, so every output
is bit-exact against the numpy restatement of the plain bank fed copies of the input rows, CR.render(x[:, source, :], h): the routing
matrix around the partition edges, the identity map against the plain constructor, ragged launches in both layouts and executors, a block
length above the head tile, several chunks, 2048 instances, reset / clone / set_sample_rate / set_response, a captured launch replayed,
subnormal inputs through both builds, graphs with branches against the oracle's generators, and the refusals."""
import numpy as np
import pytest

import convolve_ref as CR
import oracle as O
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from fundsp_amd import graph as GR
from test_convolve_ref import BLOCK_BOUND
from test_gpu_convolve import response, same_bits, signal
from test_gpu_parity import assert_bit_equal, oracle_render, run_bank

pytestmark = pytest.mark.gpu
B0 = 64
MAPS = [(1, [0, 0]), (1, [0, 0, 0]), (2, [0, 0, 1, 1]), (2, [0, 1, 0, 1]), (2, [1, 0]), (3, [2, 0, 0, 1, 0, 0, 0, 2])]


def want_of(x, source, h, **kw):
    """the plain bank of len(source) channels fed copies of the input rows"""
    return CR.render(np.ascontiguousarray(x[:, list(source), :]), h, **kw)


def pieces(bank, x, lens, layout, mode):
    parts, t0 = [], 0
    for n in lens:
        parts.append(run_bank(bank, np.ascontiguousarray(x[:, :, t0:t0 + n]), n, layout, mode))
        t0 += n
    return np.concatenate(parts, axis=2)


@pytest.mark.parametrize("M", [1, 64, 65, 337])
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("inputs,source", MAPS, ids=["".join(map(str, s)) for _, s in MAPS])
def test_routing_matrix_bit_exact(gpu, M, per, inputs, source):
    """B = 64 on both sides of the partition edges; groups of two, a remainder of one, outputs of a group that are not adjacent, a
    permutation without sharing, five outputs on one input of three"""
    import fundsp_amd as F

    V, C = 3, len(source)
    B = CR.block_length(M)
    T = M + 3 * B + 11
    x = signal(V, inputs, T, seed=M + C)
    h = response((V, C) if per else (C,), M, seed=M)
    b = F.Bank.convolve(V, h, per_instance=per, source=source)
    assert (b.inputs(), b.outputs(), b.kind, b.block_length, b.source) == (inputs, C, "convolve", B, tuple(source))
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), want_of(x, source, h), f"M={M} source={source} per_instance={per}")


def test_identity_map_is_the_plain_bank(gpu):
    import fundsp_amd as F

    M, V, T, C = 200, 3, 500, 2
    x = signal(V, C, T, seed=41)
    h = response((C,), M, seed=41)
    plain = run_bank(F.Bank.convolve(V, h), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    b = F.Bank.convolve(V, h, source=range(C))
    assert (b.inputs(), b.outputs(), b.source) == (C, C, (0, 1))
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), plain, "identity map")
    same_bits(plain, CR.render(x, h), "plain bank")


@pytest.mark.parametrize("layout", [LAYOUT_VOICE_MINOR, LAYOUT_PLANAR])
def test_ragged_launches_layouts_and_executors(gpu, layout):
    import fundsp_amd as F

    M, V = 200, 3
    lens = [1, 63, 64, 65, 69, 199]
    T = sum(lens)
    for inputs, source in ((1, [0, 0]), (2, [0, 1, 0, 1])):
        x = signal(V, inputs, T, seed=9 + inputs)
        h = response((len(source),), M, seed=9)
        want = want_of(x, source, h)
        for mode in (MODE_PROCESS, MODE_TICK):
            b = F.Bank.convolve(V, h, source=source)
            same_bits(pieces(b, x, lens, layout, mode), want, f"source={source} mode {mode}: ragged launches")
    x = signal(V, 1, 150, seed=10)
    b = F.Bank.convolve(V, h[:2], source=[0, 0])
    same_bits(pieces(b, x, [1] * 150, layout, MODE_TICK), want_of(x, [0, 0], h[:2]), "sample by sample")


def test_block_length_above_the_head_tile(gpu):
    """9 000 taps of capacity: B = 512, two 256-sample tiles per block; 700 + 624 frames cross two block boundaries"""
    import fundsp_amd as F

    M, V, T = 9000, 2, 1324
    source = [0, 0, 0]
    x = signal(V, 1, T, seed=51)
    h = response((3,), M, seed=51)
    b = F.Bank.convolve(V, h, source=source)
    assert b.block_length == 512
    got = pieces(b, x, [700, 624], LAYOUT_PLANAR, MODE_PROCESS)
    same_bits(got, want_of(x, source, h), "B = 512")
    y64 = np.convolve(x[1, 0].astype(np.float64), h[2].astype(np.float64))[:T]
    err = np.abs(got[1, 2] - y64).max() / (np.abs(h[2]).sum() * np.abs(x[1, 0]).max())
    print(f"B = 512, output 2 of instance 1 against float64: {err:.3g}")
    assert err <= BLOCK_BOUND, "the bound of tests/test_convolve_ref.py for B = 128 .. 4096"


def test_long_launch_spans_several_chunks(gpu):
    """B = 64 and 64 blocks per chunk: 10 000 frames in one launch are 3 chunks; the same input in ragged launches gives the same bits"""
    import fundsp_amd as F

    M, V, T = 100, 3, 10000
    x = signal(V, 1, T, seed=3)
    h = response((2,), M, seed=3)
    one = run_bank(F.Bank.convolve(V, h, source=[0, 0]), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    lens = [4097, 1, 63, 2000, 3839]
    assert sum(lens) == T
    same_bits(one, pieces(F.Bank.convolve(V, h, source=[0, 0]), x, lens, LAYOUT_VOICE_MINOR, MODE_PROCESS), "3 chunks against ragged launches")
    same_bits(one, want_of(x, [0, 0], h), "3 chunks")


def test_many_instances(gpu):
    """2 048 instances: more (instance, group) units than a workgroup of the fan tail and head holds; every instance compared"""
    import fundsp_amd as F

    M, V, T = 200, 2048, 500
    x = signal(V, 1, T, seed=5)
    for per in (False, True):
        h = response((V, 2) if per else (2,), M, seed=6)
        b = F.Bank.convolve(V, h, per_instance=per, source=[0, 0])
        same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), want_of(x, [0, 0], h), f"V={V} per_instance={per}")


def test_reset_clone_and_sample_rate(gpu):
    import fundsp_amd as F

    M, V, T1, T2 = 300, 3, 333, 280
    source = [0, 0, 1]
    x = signal(V, 2, T1 + T2, seed=11)
    h = response((V, 3), M, seed=11)
    x1, x2 = np.ascontiguousarray(x[:, :, :T1]), np.ascontiguousarray(x[:, :, T1:])
    b = F.Bank.convolve(V, h, per_instance=True, max_len=1000, source=source)
    run_bank(b, x1, T1, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    c = b.clone()
    assert (c.kind, c.max_len, c.block_length, c.per_instance, c.source, c.inputs(), c.outputs()) == ("convolve", 1000, 128, True, (0, 0, 1), 2, 3)
    b.set_sample_rate(96000.0)   # Convolver has no set_sample_rate override: nothing moves
    want = want_of(x, source, h, max_len=1000)
    same_bits(run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS), want[:, :, T1:], "after set_sample_rate")
    same_bits(run_bank(c, x2, T2, LAYOUT_PLANAR, MODE_PROCESS), want[:, :, T1:], "the clone continues in mid-stream")
    # ... and independently: the clone goes on with other samples, the source starts over
    x3 = signal(V, 2, T2, seed=12)
    b.reset()
    same_bits(run_bank(c, x3, T2, LAYOUT_PLANAR, MODE_PROCESS), want_of(np.concatenate([x, x3], axis=2), source, h, max_len=1000)[:, :, T1 + T2:], "the clone alone")
    same_bits(run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS), want_of(x2, source, h, max_len=1000), "reset clears the history in mid-stream")


def test_set_response_between_launches(gpu):
    """all rows (shorter, up to the capacity), some rows of a per-instance bank; the history is cleared every time; the length rules"""
    import fundsp_amd as F
    from fundsp_amd import FdspError

    V, cap, T = 3, 700, 450
    source = [0, 0]
    x = signal(V, 1, T, seed=21)
    h0 = response((2,), 300, seed=21)
    b = F.Bank.convolve(V, h0, max_len=cap, source=source)
    assert b.block_length == CR.block_length(cap) == 128
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), want_of(x, source, h0, max_len=cap), "creation response")
    for M in (5, cap, 129):
        h = response((2,), M, seed=M)
        b.set_response(h)
        same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), want_of(x, source, h, max_len=cap), f"set_response to {M} taps")
    with pytest.raises(FdspError, match="max_len"):
        b.set_response(np.ones((2, cap + 1), np.float32))
    hv = response((V, 2), 200, seed=23)
    p = F.Bank.convolve(V, hv, per_instance=True, max_len=cap, source=source)
    run_bank(p, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    new = response((1, 2), 200, seed=24)
    p.set_response(new, first=1)
    hv2 = hv.copy()
    hv2[1] = new[0]
    same_bits(run_bank(p, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), want_of(x, source, hv2, max_len=cap), "row 1 replaced, the whole bank starts over")
    with pytest.raises(FdspError, match="one response length"):
        p.set_response(new[:, :, :100], first=1)
    with pytest.raises(FdspError, match="rows out of range"):
        p.set_response(new, first=3)


def test_captured_launch_replays(gpu):
    """A 64-frame launch of a [0, 0] bank captured on a caller's stream and replayed across block boundaries (B = 128: one every second
    replay); a set_response in between is followed by the replay (the lengths live on the device)"""
    import torch

    import fundsp_amd as F

    M, V, T = 600, 5, 64
    reps = 9
    source = [0, 0]
    x = signal(V, 1, T * (reps + 1), seed=13)
    h = response((2,), M, seed=13)
    b = F.Bank.convolve(V, h, source=source)
    assert b.block_length == 128
    head = run_bank(b, np.ascontiguousarray(x[:, :, :T]), T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    inp = torch.zeros((1, T, V), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, T, V), dtype=torch.float32, device="cuda")
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
    same_bits(got, want_of(x, source, h), "captured launch, replayed")
    h2 = response((2,), 77, seed=14)
    b.set_response(h2)
    same_bits(replay(0, 5), want_of(x[:, :, :5 * T], source, h2, max_len=M), "replays after set_response")


def test_subnormal_inputs_ieee_and_flushed(gpu):
    import fundsp_amd as F

    M, V, T = 150, 2, 400
    x = signal(V, 1, T, seed=17)
    x[0] *= np.float32(2.0 ** -130)   # instance 0: subnormal input samples
    x[1] *= np.float32(2.0 ** -122)   # instance 1: normal samples whose products with the taps fall into the denormal range
    h = response((2,), M, seed=17)
    assert np.any((np.abs(x) < np.float32(2.0 ** -126)) & (x != 0))
    for ftz in (False, True):
        b = F.Bank.convolve(V, h, flush_denormals=ftz, source=[0, 0])
        want = want_of(x, [0, 0], h, ftz=ftz)
        got = run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
        same_bits(got, want, f"ftz={ftz}")
        if not ftz:
            assert np.any(got[0, 0] != 0) and np.any(got[0, 1] != 0), "IEEE build: the denormal input comes through"
        else:
            assert not np.any(got[0]), "flushed build: a denormal input reads as zero"


def test_graphs_with_branches(gpu):
    """`a ^ b` and `(a ^ b) | (c ^ d)` are routed banks; noise() >> (a ^ b) is a Chain whose front is seeded from the construction hash of
    the whole graph, into which Branch::ID = 8 and both Convolver::ID = 100 enter; a branch inside a sum is refused"""
    import torch

    import fundsp_amd as F
    from fundsp_amd.bank import PIPE_ID, atto, probe_hash

    w = np.stack([response((), 300, seed=31), response((), 300, seed=32)])
    b = F.Bank.from_graph(GR.convolve(w, 0) ^ GR.convolve(w, 1), 3)
    assert isinstance(b, F.Bank) and (b.kind, b.inputs(), b.outputs(), b.source) == ("convolve", 1, 2, (0, 0))
    x = signal(3, 1, 400, seed=33)
    same_bits(run_bank(b, x, 400, LAYOUT_VOICE_MINOR, MODE_PROCESS), want_of(x, [0, 0], w), "a ^ b")
    h1 = response((), 170, seed=34)
    w4 = np.zeros((4, 300), np.float32)
    w4[0], w4[1, :170], w4[2], w4[3, :170] = w[0], h1, w[1], h1
    b = F.Bank.from_graph((GR.convolve(w, 0) ^ GR.convolve(h1)) | (GR.convolve(w, 1) ^ GR.convolve(h1)), 3)
    assert isinstance(b, F.Bank) and (b.kind, b.inputs(), b.outputs(), b.source) == ("convolve", 2, 4, (0, 0, 1, 1))
    x = signal(3, 2, 400, seed=35)
    same_bits(run_bank(b, x, 400, LAYOUT_VOICE_MINOR, MODE_PROCESS), want_of(x, [0, 0, 1, 1], w4), "(a ^ b) | (c ^ d)")

    T = 1000
    g = GR.noise() >> (GR.convolve(w, 0) ^ GR.convolve(h1))
    # Pipe::new: ping(true, AttoHash::new(Pipe::ID)); Pipe::ping hashes Pipe::ID, then Noise::ID = 20, then Branch::ping: 8, 100, 100
    hn = atto(atto(np.uint64(PIPE_ID), PIPE_ID), 20)
    assert probe_hash(g) == int(atto(atto(atto(hn, 8), 100), 100))
    for mode in (MODE_PROCESS, MODE_TICK):
        ch = F.Bank.from_graph(g, 2)
        assert isinstance(ch, F.Chain) and ch.effect.kind == "convolve" and ch.effect.source == (0, 0)
        assert (ch.inputs(), ch.outputs(), ch.effect.inputs()) == (0, 2, 1)
        out = ch.process(T, mode=mode)
        torch.cuda.synchronize()
        got = out.cpu().numpy().transpose(2, 0, 1)
        n = O.noise()
        n.set_seed(int(atto(np.uint64(probe_hash(g)), PIPE_ID)))
        xn = oracle_render(n, None, T, mode)
        want = want_of(xn[None], [0, 0], w4[:2])[0]
        for v in range(2):
            assert_bit_equal(got[v], want, f"{g.type} mode {mode}, instance {v}")
    with pytest.raises(ValueError, match="front >> convolve"):
        F.Bank.from_graph((GR.convolve(w, 0) ^ GR.convolve(w, 1)) + (GR.convolve(w, 0) ^ GR.convolve(w, 1)), 2)


def test_invalid_routings_and_unsupported_calls(gpu):
    import ctypes as C

    import fundsp_amd as F
    from fundsp_amd import FdspError, _lib

    L = _lib.lib()
    h = np.ones((2, 16), np.float32)
    for source, msg in (([0, 2], "inputs = 3"), ([1, 1], "input 0"), ([0, -1], r"source\[1\] = -1")):
        with pytest.raises(FdspError, match=msg):
            F.Bank.convolve(2, h, source=source)
    with pytest.raises(ValueError, match="one input index per output"):
        F.Bank.convolve(2, h, source=[0])
    s = _lib.ConvolveSpec()
    s.channels, s.max_len, s.len = 2, 16, 16
    s.response = h.ctypes.data_as(C.POINTER(C.c_float))
    for inputs, source in ((0, [0, 0]), (3, [0, 1]), (1, None)):
        out = C.c_void_p(1)
        src = None if source is None else (C.c_int * 2)(*source)
        assert L.fdsp_convolve_routed_create(4, C.byref(s), inputs, src, C.byref(out)) == _lib.EINVAL and not out.value
    b = F.Bank.convolve(2, h, source=[0, 0])
    assert L.fdsp_bank_set_bus(b._h, _lib.BUS_WET, 0.5, 1.0) == _lib.ENOTSUP
    assert L.fdsp_bank_get_bus(b._h, None, None, None) == _lib.ENOTSUP
    out = C.c_void_p()
    assert L.fdsp_bank_process_mix(b._h, 64, None, out, _lib.MIX_SUM, 0, None) == _lib.ENOTSUP
