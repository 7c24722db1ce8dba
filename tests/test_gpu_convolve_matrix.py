"""GPU parity of the summing convolver banks (fdsp_convolve_matrix_create, Bank.convolve(.., source=.., target=..), Bank.convolve_tree):
several inputs convolved and added into one output.  Every comparison is uint32-equal to the numpy restatement of the contract,
tests/convolve_matrix_ref.py: the shapes (2 -> 1, true stereo, 8 -> 2 with 16 terms, two terms of one input, one term next to three) around
the partition edges, shared and per-instance responses, ragged launches in both layouts and executors that start and end inside a head
tile, a block of two head tiles, a launch of two chunks, one term per output against the routed bank on the device, reset / clone /
set_response, a captured launch replayed, subnormal inputs through both builds, the graph constructor, a Chain, and the refusals."""
import numpy as np
import pytest

import convolve_matrix_ref as MR
import convolve_ref as CR
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from fundsp_amd import graph as GR
from test_gpu_convolve import response, same_bits, signal
from test_gpu_parity import run_bank

pytestmark = pytest.mark.gpu
B0 = 64
# (term_input, term_output)
TWO_ONE = ([0, 1], [0, 0])
STEREO = ([0, 1, 0, 1], [0, 0, 1, 1])                       # (ll + rl) ^ (lr + rr)
EIGHT_TWO = (list(range(8)) * 2, [0] * 8 + [1] * 8)         # 16 terms
SAME_INPUT = ([0, 0], [0, 0])
ONE_AND_THREE = ([1, 0, 1, 1], [0, 1, 1, 1])                # an output of one term next to one of three (two of them of one input in a row)
SHAPES = {"2to1": TWO_ONE, "stereo": STEREO, "8to2": EIGHT_TWO, "same_input": SAME_INPUT, "1and3": ONE_AND_THREE}


def bank_of(V, h, shape, **kw):
    import fundsp_amd as F

    tin, tout = shape
    b = F.Bank.convolve(V, h, source=tin, target=tout, **kw)
    assert (b.inputs(), b.outputs(), b.kind, b.source, b.target) == (max(tin) + 1, max(tout) + 1, "convolve", tuple(tin), tuple(tout))
    return b


def pieces(bank, x, lens, layout, mode):
    parts, t0 = [], 0
    for n in lens:
        parts.append(run_bank(bank, np.ascontiguousarray(x[:, :, t0:t0 + n]), n, layout, mode))
        t0 += n
    return np.concatenate(parts, axis=2)


@pytest.mark.parametrize("M", [1, 3, 63, 64, 65, 337])
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_bit_exact(gpu, name, per, M):
    """B = 64 on both sides of the partition edges, one tap, six partitions"""
    tin, tout = SHAPES[name]
    V, NT = 3, len(tin)
    B = CR.block_length(M)
    T = M + 3 * B + 11
    x = signal(V, max(tin) + 1, T, seed=M + NT)
    h = response((V, NT) if per else (NT,), M, seed=M)
    b = bank_of(V, h, (tin, tout), per_instance=per)
    assert b.block_length == B == B0
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), MR.render(x, h, tin, tout), f"{name} M={M} per_instance={per}")


@pytest.mark.parametrize("layout", [LAYOUT_VOICE_MINOR, LAYOUT_PLANAR])
@pytest.mark.parametrize("mode", [MODE_PROCESS, MODE_TICK])
def test_ragged_launches_layouts_and_executors(gpu, layout, mode):
    """launches of 1, 63, 64, 65 and 200 frames across block boundaries, then 7 + 5 + 20 frames that start and end inside one 64-sample
    head tile: lanes outside the launch's samples still reach every barrier of the term loop"""
    V, M = 3, 200
    lens = [1, 63, 64, 65, 200, 7, 5, 20, 41]
    assert sum(lens[:5]) == 393 and (393 + 7) // B0 == (393 + 7 + 5 + 20) // B0, "the three short launches lie inside one tile"
    T = sum(lens)
    for name in ("stereo", "1and3", "same_input"):
        tin, tout = SHAPES[name]
        x = signal(V, max(tin) + 1, T, seed=9 + len(tin))
        h = response((len(tin),), M, seed=9)
        same_bits(pieces(bank_of(V, h, (tin, tout)), x, lens, layout, mode), MR.render(x, h, tin, tout), f"{name}: ragged launches")


def test_sample_by_sample(gpu):
    V, T = 2, 150
    tin, tout = STEREO
    x = signal(V, 2, T, seed=10)
    h = response((4,), 100, seed=10)
    same_bits(pieces(bank_of(V, h, STEREO), x, [1] * T, LAYOUT_VOICE_MINOR, MODE_TICK), MR.render(x, h, tin, tout), "sample by sample")


def test_block_of_two_head_tiles(gpu):
    """a capacity of 8 193 taps: B = 512, two 256-sample tiles per block; launches that cross two block boundaries, end inside the second
    tile of a block, and one of 3 frames inside a tile"""
    V, M, cap = 2, 700, 8193
    lens = [700, 3, 100, 621]
    T = sum(lens)
    for name in ("stereo", "1and3"):
        tin, tout = SHAPES[name]
        x = signal(V, 2, T, seed=51)
        h = response((4,), M, seed=51)
        b = bank_of(V, h, (tin, tout), max_len=cap)
        assert b.block_length == 512
        same_bits(pieces(b, x, lens, LAYOUT_PLANAR, MODE_PROCESS), MR.render(x, h, tin, tout, max_len=cap), f"{name}: B = 512")


def test_long_launch_spans_two_chunks(gpu):
    """B = 64 and a small bank: KB = 64 blocks per chunk, so 4 096 + 130 frames in one launch are two chunks"""
    V, M, T = 3, 100, 4096 + 130
    assert CR.blocks_per_chunk(V, 1, B0) == 64
    tin, tout = TWO_ONE
    x = signal(V, 2, T, seed=3)
    h = response((2,), M, seed=3)
    same_bits(run_bank(bank_of(V, h, TWO_ONE), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), MR.render(x, h, tin, tout), "two chunks")


@pytest.mark.parametrize("per", [False, True])
def test_one_term_per_output_is_the_routed_bank(gpu, per):
    """both device results: the summing bank in which every output has one term IS the routed bank"""
    import fundsp_amd as F

    V, M, T = 3, 200, 500
    source = [0, 0, 1, 0, 1]
    x = signal(V, 2, T, seed=41)
    h = response((V, 5) if per else (5,), M, seed=41)
    routed = run_bank(F.Bank.convolve(V, h, per_instance=per, source=source), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    summing = run_bank(bank_of(V, h, (source, list(range(5))), per_instance=per), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    same_bits(summing, routed, "one term per output against the routed bank")
    same_bits(summing, CR.render(np.ascontiguousarray(x[:, source]), h), "and the plain restatement")


def test_reset_clone_and_sample_rate(gpu):
    V, M, T1, T2, cap = 3, 300, 333, 280, 1000
    tin, tout = ONE_AND_THREE
    x = signal(V, 2, T1 + T2, seed=11)
    h = response((V, 4), M, seed=11)
    x1, x2 = np.ascontiguousarray(x[:, :, :T1]), np.ascontiguousarray(x[:, :, T1:])
    b = bank_of(V, h, ONE_AND_THREE, per_instance=True, max_len=cap)
    run_bank(b, x1, T1, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    c = b.clone()
    assert (c.kind, c.max_len, c.block_length, c.per_instance, c.source, c.target, c.inputs(), c.outputs()) == \
        ("convolve", cap, 128, True, tuple(tin), tuple(tout), 2, 2)
    b.set_sample_rate(96000.0)   # Convolver has no set_sample_rate override: nothing moves
    want = MR.render(x, h, tin, tout, max_len=cap)
    same_bits(run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS), want[:, :, T1:], "after set_sample_rate")
    same_bits(run_bank(c, x2, T2, LAYOUT_PLANAR, MODE_PROCESS), want[:, :, T1:], "the clone continues in mid-stream")
    b.reset()
    same_bits(run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS), MR.render(x2, h, tin, tout, max_len=cap), "reset clears the history in mid-stream")


def test_set_response_between_launches(gpu):
    """all rows to another length (shorter, up to the capacity), one row of a per-instance bank; rows are [terms, len]"""
    from fundsp_amd import FdspError

    V, cap, T = 3, 700, 450
    tin, tout = STEREO
    x = signal(V, 2, T, seed=21)
    h0 = response((4,), 300, seed=21)
    b = bank_of(V, h0, STEREO, max_len=cap)
    assert b.block_length == 128
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), MR.render(x, h0, tin, tout, max_len=cap), "creation response")
    for M in (5, cap, 129):
        h = response((4,), M, seed=M)
        b.set_response(h)
        same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), MR.render(x, h, tin, tout, max_len=cap), f"set_response to {M} taps")
    with pytest.raises(FdspError, match="max_len"):
        b.set_response(np.ones((4, cap + 1), np.float32))
    with pytest.raises(ValueError, match="channels"):
        b.set_response(np.ones((2, 10), np.float32))   # rows are per term, not per output
    hv = response((V, 4), 200, seed=23)
    p = bank_of(V, hv, STEREO, per_instance=True, max_len=cap)
    run_bank(p, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    new = response((1, 4), 200, seed=24)
    p.set_response(new, first=1)
    hv2 = hv.copy()
    hv2[1] = new[0]
    same_bits(run_bank(p, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), MR.render(x, hv2, tin, tout, max_len=cap), "row 1 replaced, the whole bank starts over")
    with pytest.raises(FdspError, match="one response length"):
        p.set_response(new[:, :, :100], first=1)


def test_captured_launch_replays(gpu):
    """A 64-frame launch of a true-stereo bank captured on a caller's stream and replayed across block boundaries (B = 128: one every
    second replay); a set_response in between is followed by the replay (the lengths live on the device)"""
    import torch

    M, V, T = 600, 5, 64
    reps = 9
    tin, tout = STEREO
    x = signal(V, 2, T * (reps + 1), seed=13)
    h = response((4,), M, seed=13)
    b = bank_of(V, h, STEREO)
    assert b.block_length == 128
    head = run_bank(b, np.ascontiguousarray(x[:, :, :T]), T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    inp = torch.zeros((2, T, V), dtype=torch.float32, device="cuda")
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
    same_bits(got, MR.render(x, h, tin, tout), "captured launch, replayed")
    h2 = response((4,), 77, seed=14)
    b.set_response(h2)
    same_bits(replay(0, 5), MR.render(x[:, :, :5 * T], h2, tin, tout, max_len=M), "replays after set_response")


def test_subnormal_inputs_ieee_and_flushed(gpu):
    M, V, T = 150, 2, 400
    tin, tout = STEREO
    x = signal(V, 2, T, seed=17)
    x[0] *= np.float32(2.0 ** -130)   # instance 0: subnormal input samples
    x[1] *= np.float32(2.0 ** -122)   # instance 1: normal samples whose products with the taps fall into the denormal range
    h = response((4,), M, seed=17)
    assert np.any((np.abs(x) < np.float32(2.0 ** -126)) & (x != 0))
    for ftz in (False, True):
        got = run_bank(bank_of(V, h, STEREO, flush_denormals=ftz), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
        same_bits(got, MR.render(x, h, tin, tout, ftz=ftz), f"ftz={ftz}")
        if not ftz:
            assert np.any(got[0, 0] != 0) and np.any(got[0, 1] != 0), "IEEE build: the denormal input comes through"
        else:
            assert not np.any(got[0]), "flushed build: a denormal input reads as zero"


def test_graph_constructor_and_chain(gpu):
    """Bank.convolve_tree((ll + rl) ^ (lr + rr), ..) is the true-stereo bank; Chain(noise() | noise(), bank) feeds it the front's samples"""
    import torch

    import fundsp_amd as F

    V, T = 3, 400
    w = np.stack([response((), 300, seed=31 + c) for c in range(4)])
    ll, lr, rl, rr = (GR.convolve(w, c) for c in range(4))
    g = (ll + rl) ^ (lr + rr)
    b = F.Bank.convolve_tree(g, V)
    assert isinstance(b, F.Bank) and (b.kind, b.inputs(), b.outputs(), b.source, b.target) == ("convolve", 2, 2, (0, 1, 0, 1), (0, 0, 1, 1))
    x = signal(V, 2, T, seed=33)
    hw = w[[0, 2, 1, 3]]
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), MR.render(x, hw, *STEREO), "(ll + rl) ^ (lr + rr)")
    f = F.Bank.convolve_tree(g, V, max_len=1000, flush_denormals=True)
    assert f.block_length == 128 and f.max_len == 1000
    same_bits(run_bank(f, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), MR.render(x, hw, *STEREO, max_len=1000, ftz=True), "capacity and the flushed build")
    with pytest.raises(ValueError, match="convolve_tree"):
        F.Bank.convolve_tree(GR.noise() >> ll, V)
    with pytest.raises(ValueError, match="front >> convolve"):
        F.Bank.from_graph(g, V)   # from_graph answers as before

    front = GR.noise() | GR.noise()
    xn = run_bank(F.Bank.from_graph(front, V), None, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)   # the samples a stand-alone front renders
    ch = F.Chain(F.Bank.from_graph(front, V), F.Bank.convolve_tree(g, V))
    assert (ch.inputs(), ch.outputs(), ch.effect.inputs()) == (0, 2, 2)
    parts = []
    for n in (150, T - 150):
        out = ch.process(n)
        torch.cuda.synchronize()
        parts.append(out.cpu().numpy().transpose(2, 0, 1).copy())
    same_bits(np.concatenate(parts, axis=2), MR.render(xn, hw, *STEREO), "Chain(noise() | noise(), summing bank)")


def test_invalid_specs_and_unsupported_calls(gpu):
    import ctypes as C

    import fundsp_amd as F
    from fundsp_amd import FdspError, _lib

    L = _lib.lib()
    h = np.ones((2, 16), np.float32)
    for source, target, msg in (([0, 2], [0, 0], "input 1"), ([0, 1], [1, 0], "non-decreasing"), ([0, 1], [1, 1], "output 0"),
                                ([0, -1], [0, 0], r"term_input\[1\] = -1"), ([0, 1], [0, 2], "output 1")):
        with pytest.raises(FdspError, match=msg):
            F.Bank.convolve(2, h, source=source, target=target)
    with pytest.raises(ValueError, match="one output index per term"):
        F.Bank.convolve(2, h, source=[0, 1], target=[0])
    with pytest.raises(ValueError, match="1 .. 16"):
        F.Bank.convolve(2, np.ones((17, 4), np.float32), source=[0] * 17, target=[0] * 17)
    s = _lib.ConvolveSpec()
    s.channels, s.max_len, s.len = 2, 16, 16
    s.response = h.ctypes.data_as(C.POINTER(C.c_float))
    for inputs, outputs, tin, tout in ((0, 1, [0, 0], [0, 0]), (2, 9, [0, 1], [0, 0]), (2, 1, None, [0, 0]), (2, 1, [0, 1], None)):
        out = C.c_void_p(1)
        ti = None if tin is None else (C.c_int * 2)(*tin)
        to = None if tout is None else (C.c_int * 2)(*tout)
        assert L.fdsp_convolve_matrix_create(4, C.byref(s), inputs, outputs, ti, to, C.byref(out)) == _lib.EINVAL and not out.value
    b = F.Bank.convolve(2, h, source=[0, 1], target=[0, 0])
    assert L.fdsp_bank_set_bus(b._h, _lib.BUS_WET, 0.5, 1.0) == _lib.ENOTSUP
    assert L.fdsp_bank_get_bus(b._h, None, None, None) == _lib.ENOTSUP
    out = C.c_void_p()
    assert L.fdsp_bank_process_mix(b._h, 64, None, out, _lib.MIX_SUM, 0, None) == _lib.ENOTSUP
    assert L.fdsp_bank_process_mix_planar(b._h, 64, None, 64, out, _lib.MIX_SUM, 0, None) == _lib.ENOTSUP
    assert L.fdsp_bank_mix_reserve(b._h, 64) == _lib.ENOTSUP
    one = np.ones(2, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert L.fdsp_bank_set_pan(b._h, one, 0, 2) == _lib.ENOTSUP
    assert L.fdsp_bank_set_ring(b._h, 0, one, 1, 0, 2) == _lib.ENOTSUP                      # rings
    assert L.fdsp_bank_set_events(b._h, None, None, 0, 0) == _lib.ENOTSUP                   # events
    import torch

    dev = torch.zeros((1, 64, 2), dtype=torch.float32, device="cuda")   # (a NULL d_out is refused before the bank is looked at)
    assert L.fdsp_bank_process_events(b._h, 64, None, C.c_void_p(dev.data_ptr()), 0, None) == _lib.ENOTSUP
    assert b"render through fdsp_bank_process" in L.fdsp_last_error()
    # slots: the bank has none to name, as the plain convolver bank (FDSP_EINVAL, unknown slot)
    assert L.fdsp_bank_set_param(b._h, b"f", one, 0, 2) == _lib.EINVAL and b"unknown slot" in L.fdsp_last_error()
    # the calls above left the bank as it was
    x = signal(2, 2, 100, seed=1)
    same_bits(run_bank(b, x, 100, LAYOUT_VOICE_MINOR, MODE_PROCESS), MR.render(x, h, [0, 1], [0, 0]), "after the refused calls")
