"""GPU parity of the convolver banks at every block length and in both builds (tests/test_gpu_convolve.py stays at B = 64 .. 256 and the
IEEE build, one launch at B = 1024 apart).  Every output is compared bit for bit with the numpy restatement tests/convolve_ref.py; the long
responses also with float64 under the bound of tests/test_convolve_ref.py.  Every case asserts the block length that places it, and the
chunk cases the blocks per chunk and the chunk count.

Which test launches which instantiation.  A bank's creation and every set_response launch k_cv_forward<log2 B, true>; every launch of at
least one complete block launches k_cv_forward<log2 B, false>; every launch launches k_cv_inverse<log2 B> and k_cv_output.  k_cv_output
stages from r0 != 0 (a tile that does not start its block) whenever B > 256 and a launch reaches past the first 256 samples of a block.
`matrix[..]` is test_block_length_matrix with the ids it is parametrised by (short / long response, ieee / ftz build, B):

    log2 B   IEEE build (cv_ieee): forward<.,false>, forward<.,true>, inverse<.>          flushed build (cv_ftz): the same three
    7        matrix[short-ieee-B128-vm-c1], matrix[long-ieee-B128-vm-c1]                   matrix[short-ftz-B128-vm-c1], matrix[long-ftz-B128-vm-c1]
    8        matrix[short-ieee-B256-planar-c2], matrix[long-ieee-B256-planar-c2]           matrix[short-ftz-B256-planar-c2], matrix[long-ftz-B256-planar-c2]
    9        matrix[*-ieee-B512-vm-c8], matrix[*-ieee-B512-planar-c1],                     matrix[*-ftz-B512-vm-c8], matrix[*-ftz-B512-planar-c1]
             test_ragged_launches_tiles_inside_blocks[512-*], test_sample_by_sample_b512,
             test_captured_launch_replays_b512, test_chunk_edges[kb64 / between / kb8]
    10       matrix[*-ieee-B1024-vm-c2]                                                    matrix[*-ftz-B1024-vm-c2]
    11       matrix[*-ieee-B2048-vm-c2], matrix[*-ieee-B2048-planar-c1],                   matrix[*-ftz-B2048-vm-c2], matrix[*-ftz-B2048-planar-c1],
             test_long_responses[144000], test_ragged_launches_tiles_inside_blocks[2048-*], test_reset_and_clone_b2048
             test_set_response_b2048
    12       matrix[*-ieee-B4096-vm-c1], matrix[*-ieee-B4096-planar-c2],                   matrix[*-ftz-B4096-vm-c1], matrix[*-ftz-B4096-planar-c2]
             test_long_responses[600000]

    k_cv_output with r0 != 0, IEEE build: every B >= 512 entry of the left column (each renders more than 256 samples of a block);
    across launches and from counts off the multiples of 256: test_ragged_launches_tiles_inside_blocks, test_sample_by_sample_b512,
    test_captured_launch_replays_b512, test_chunk_edges.  Flushed build: matrix[*-ftz-B512-*], [*-ftz-B1024-*], [*-ftz-B2048-*],
    [*-ftz-B4096-*] in one launch, test_reset_and_clone_b2048 across launches."""
import numpy as np
import pytest

import convolve_ref as CR
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from test_convolve_ref import BLOCK_BOUND, conv64
from test_gpu_convolve import response, same_bits, signal
from test_gpu_parity import run_bank

pytestmark = pytest.mark.gpu

# the capacity that gives each block length to a response of any length up to it (the largest the rule maps to B; 600 000 for 4096)
CAPACITY = {128: 2048, 256: 8192, 512: 32768, 1024: 131072, 2048: 524288, 4096: 600000}
VM, PL = LAYOUT_VOICE_MINOR, LAYOUT_PLANAR


def pieces(b, x, lens, layout, mode):
    """x rendered as consecutive launches of the given lengths"""
    parts, t0 = [], 0
    for n in lens:
        parts.append(run_bank(b, np.ascontiguousarray(x[:, :, t0:t0 + n]), n, layout, mode))
        t0 += n
    assert t0 == x.shape[2]
    return np.concatenate(parts, axis=2)


@pytest.mark.parametrize("B,layout,channels", [pytest.param(B, lay, ch, id=f"B{B}-{'vm' if lay == VM else 'planar'}-c{ch}") for B, lay, ch in (
    (128, VM, 1), (256, PL, 2), (512, VM, 8), (512, PL, 1), (1024, VM, 2), (2048, VM, 2), (2048, PL, 1), (4096, VM, 1), (4096, PL, 2))])
@pytest.mark.parametrize("ftz", [False, True], ids=["ieee", "ftz"])
@pytest.mark.parametrize("shape", ["short", "long"])
def test_block_length_matrix(gpu, shape, ftz, B, layout, channels):
    """every B above 64 in both builds: 3 taps (P = 1) and B + 1 taps (P = 2, a full-length head) under the capacity that gives B; shared
    and per-instance responses; instance 0 subnormal samples, instance 1 normal samples whose products are subnormal, instance 2 plain"""
    import fundsp_amd as F

    V, cap = 3, CAPACITY[B]
    per = shape == "long"
    M = B + 1 if per else 3
    T = M + 3 * B + 11
    x = signal(V, channels, T, seed=B + channels)
    x[0] *= np.float32(2.0 ** -130)
    x[1] *= np.float32(2.0 ** -122)
    assert np.any((np.abs(x) < np.float32(2.0 ** -126)) & (x != 0)), "the two builds have different bits to give"
    h = response((V, channels) if per else (channels,), M, seed=B)
    b = F.Bank.convolve(V, h, max_len=cap, per_instance=per, flush_denormals=ftz)
    assert (b.block_length, CR.block_length(cap), b.outputs()) == (B, B, channels)
    got = run_bank(b, x, T, layout, MODE_PROCESS)
    same_bits(got, CR.render(x, h, max_len=cap, ftz=ftz), f"B={B} M={M} C={channels} ftz={ftz}")
    assert np.any(got[1] != 0) and np.any(got[2] != 0)
    if ftz:
        assert not np.any(got[0]), "flushed build: a denormal input reads as zero"
    else:
        assert np.any(got[0] != 0), "IEEE build: the denormal input comes through"


@pytest.mark.parametrize("M,B,T", [(144000, 2048, 148200), (600000, 4096, 608300)], ids=["144000", "600000"])
def test_long_responses(gpu, M, B, T):
    """144 000 taps (3 s at 48 kHz: B = 2048, 71 partitions) and 600 000 taps (B = 4096, 147 partitions), per-instance responses on three
    instances, one launch of T >= M + 2B frames so that every partition contributes; instance 1 bit-exact and within the float64 bound"""
    import fundsp_amd as F

    V = 3
    assert T >= M + 2 * B
    x = signal(V, 1, T, seed=M)
    h = response((V, 1), M, seed=M + 1)
    b = F.Bank.convolve(V, h, per_instance=True)
    assert b.block_length == B == CR.block_length(M)
    got = run_bank(b, x, T, LAYOUT_PLANAR, MODE_PROCESS)
    same_bits(got[1:2], CR.render(x[1:2], h[1:2]), f"{M} taps")
    err = np.abs(got[1, 0] - conv64(x[1, 0], h[1, 0])).max() / (np.abs(h[1, 0]).sum() * np.abs(x[1, 0]).max())
    print(f"M={M} B={B}: err {err:.3g} against float64, bound {BLOCK_BOUND:.3g}")
    assert err <= BLOCK_BOUND, "the bound of tests/test_convolve_ref.py for every block length"


def ragged_lengths(B):
    """launch lengths whose starts and ends fall 1 before, on and 1 after a multiple of 256 that is no block edge, the same around block
    edges, and inside tiles; then the lengths 255, 256, 257, B - 1, B, B + 5, 3B + 7 and 1 from wherever that leaves the count"""
    cuts = [0, 1, 255, 256, 257, B - 1, B, B + 1, B + 300, 2 * B - 1, 2 * B, 2 * B + 1, 2 * B + 255, 2 * B + 256, 2 * B + 257]
    assert cuts == sorted(set(cuts)) and B % 512 == 0
    return [int(n) for n in np.diff(cuts)] + [255, 256, 257, B - 1, B, B + 5, 3 * B + 7, 1]


@pytest.mark.parametrize("layout", [LAYOUT_VOICE_MINOR, LAYOUT_PLANAR], ids=["vm", "planar"])
@pytest.mark.parametrize("B", [512, 2048])
def test_ragged_launches_tiles_inside_blocks(gpu, B, layout):
    """B > 256: k_cv_output's tiles of 256 start inside blocks (r0 != 0) and a launch starts and ends anywhere in them; 2B + 77 taps (P = 3),
    so every sample has a full head and two tail terms; both executors; equal to the one-piece rendering bit for bit"""
    import fundsp_amd as F

    V, M, cap = 3, 2 * B + 77, CAPACITY[B]
    lens = ragged_lengths(B)
    ends = np.cumsum(lens)
    for r, rb in ((255, B - 1), (0, 0), (1, 1)):   # around a multiple of 256 inside a block, around a block edge, and well inside a tile
        assert any(e % 256 == r and 1 < e % B < B - 1 for e in ends) and any(e % B == rb for e in ends), r
    assert any(1 < e % 256 < 255 for e in ends) and 1 in lens and 3 * B + 7 in lens
    T = int(ends[-1])
    x = signal(V, 2, T, seed=B + 9)
    h = response((2,), M, seed=B + 9)
    want = CR.render(x, h, max_len=cap)
    for mode in (MODE_PROCESS, MODE_TICK):
        b = F.Bank.convolve(V, h, max_len=cap)
        assert b.block_length == B
        same_bits(pieces(b, x, lens, layout, mode), want, f"B={B} mode {mode}: ragged launches")


def test_sample_by_sample_b512(gpu):
    """2B + 3 launches of one sample across two block edges at B = 512: each tile of 256 is entered 256 times"""
    import fundsp_amd as F

    V, B = 3, 512
    M, T = B + 1, 2 * B + 3
    x = signal(V, 1, T, seed=41)
    h = response((1,), M, seed=41)
    b = F.Bank.convolve(V, h, max_len=CAPACITY[B])
    assert b.block_length == B
    same_bits(pieces(b, x, [1] * T, LAYOUT_VOICE_MINOR, MODE_TICK), CR.render(x, h, max_len=CAPACITY[B]), "sample by sample")


def test_captured_launch_replays_b512(gpu):
    """A 64-frame launch captured on a caller's stream and replayed across two block edges at B = 512 (8 replays a block, 4 a tile of
    k_cv_output); a set_response in between is followed by the replay (the lengths live on the device)"""
    import torch

    import fundsp_amd as F

    M, V, T = 8193, 5, 64
    reps = 18
    x = signal(V, 1, T * (reps + 1), seed=43)
    h = response((1,), M, seed=43)
    b = F.Bank.convolve(V, h)
    assert b.block_length == 512 and T * (reps + 1) > 2 * 512
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
    h2 = response((1,), 600, seed=44)
    b.set_response(h2)
    same_bits(replay(0, 11), CR.render(x[:, :, :11 * T], h2, max_len=M), "replays after set_response")


# V, C, B, max_len, M, per-instance, layout: blocks per chunk 64 (the upper clamp), 31 (the quotient itself), 8 (the lower clamp: the
# quotient is 7).  Device memory by fd_convolve.hpp's formula: 2 MB, 1.2 GB, 1.6 GB.
CHUNK_BANKS = {"kb64": (3, 1, 512, 32768, 600, False, VM, 64), "between": (256, 8, 512, 8193, 8193, True, PL, 31),
               "kb8": (1024, 8, 512, 8193, 8193, False, VM, 8)}


@pytest.mark.parametrize("name", list(CHUNK_BANKS))
def test_chunk_edges(gpu, name):
    """a launch of T > 2 KB B frames from a misaligned count (77 frames first): three chunks, the edges between them inside blocks and tiles;
    then 77 more frames: the state after the chunks is the state after the samples.  First, middle and last instance against the restatement"""
    import fundsp_amd as F

    V, C, B, cap, M, per, layout, KB = CHUNK_BANKS[name]
    assert CR.blocks_per_chunk(V, C, B) == KB and CR.block_length(cap) == B
    pcap = -(-cap // B)
    rx = 1 << ((KB + 1) * B - 1).bit_length()
    rows = V if per else 1
    mem = V * C * (rx * 4 + (pcap + 2 * KB) * (B + 1) * 8 + (KB + 1) * B * 4) + rows * C * ((pcap + 1) * B * 4 + pcap * (B + 1) * 8)
    assert mem < 8e9, mem
    T0, T1 = 77, 77
    T = 2 * KB * B + 600
    assert -(-T // (KB * B)) == 3, "three chunks"
    x = signal(V, C, T0 + T + T1, seed=51)
    h = response((V, C) if per else (C,), M, seed=52)
    b = F.Bank.convolve(V, h, max_len=cap, per_instance=per)
    assert b.block_length == B
    got = pieces(b, x, [T0, T, T1], layout, MODE_PROCESS)
    sel = sorted({0, V // 2, V - 1})
    want = CR.render(x[sel], h[sel] if per else h, max_len=cap)
    same_bits(got[sel], want, f"{name}: instances {sel}")


def test_reset_and_clone_b2048(gpu):
    """reset and a clone in mid-stream (inside the third block, inside a tile) at B = 2048, flushed build, per-instance responses of three
    partitions; the clone then takes a one-partition response"""
    import fundsp_amd as F

    M, V, B, cap = 5000, 3, 2048, 140000
    T1, T2 = 2 * B + 333, B + 280
    x = signal(V, 2, T1 + T2, seed=61)
    x[0] *= np.float32(2.0 ** -122)
    h = response((V, 2), M, seed=61)
    x1, x2 = np.ascontiguousarray(x[:, :, :T1]), np.ascontiguousarray(x[:, :, T1:])
    b = F.Bank.convolve(V, h, per_instance=True, max_len=cap, flush_denormals=True)
    run_bank(b, x1, T1, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    c = b.clone()
    assert (c.kind, c.max_len, c.block_length, c.per_instance) == ("convolve", cap, B, True)
    want = CR.render(x, h, max_len=cap, ftz=True)
    same_bits(run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS), want[:, :, T1:], "the bank continues")
    same_bits(run_bank(c, x2, T2, LAYOUT_PLANAR, MODE_PROCESS), want[:, :, T1:], "the clone continues in mid-stream")
    c.set_response(h[:, :, :40])
    same_bits(run_bank(c, x2, T2, LAYOUT_PLANAR, MODE_PROCESS), CR.render(x2, h[:, :, :40], max_len=cap, ftz=True), "the clone takes a new response")
    b.reset()
    same_bits(run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x2, h, max_len=cap, ftz=True), "reset clears the history")


def test_set_response_b2048(gpu):
    """B = 2048, capacity 140 000 (69 partitions): P = 1, then P = Pcap, then P = 1 again, 3B + 450 frames each; then one row of a
    per-instance bank.  The history is cleared every time"""
    import fundsp_amd as F
    from fundsp_amd import FdspError

    V, B, cap = 3, 2048, 140000
    T = 3 * B + 450
    x = signal(V, 1, T, seed=71)
    h0 = response((1,), 5, seed=71)
    b = F.Bank.convolve(V, h0, max_len=cap)
    assert b.block_length == CR.block_length(cap) == B and -(-cap // B) == 69
    same_bits(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x, h0, max_len=cap), "creation response, P = 1")
    for M in (cap, 7, B + 1):
        h = response((1,), M, seed=M)
        b.set_response(h)
        same_bits(run_bank(b, x, T, LAYOUT_PLANAR, MODE_PROCESS), CR.render(x, h, max_len=cap), f"set_response to {M} taps")
    with pytest.raises(FdspError, match="max_len"):
        b.set_response(np.ones(cap + 1, np.float32))
    hv = response((V, 1), B + 200, seed=73)
    p = F.Bank.convolve(V, hv, per_instance=True, max_len=cap)
    run_bank(p, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    new = response((1, 1), B + 200, seed=74)
    p.set_response(new, first=1)
    hv2 = hv.copy()
    hv2[1] = new[0]
    same_bits(run_bank(p, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), CR.render(x, hv2, max_len=cap), "row 1 replaced, the whole bank starts over")


def test_flushed_result_is_judged_before_rounding(gpu):
    """(1 - 2^-24) * 2^-126 lies half an ulp below 2^-126 and IEEE rounds it up to 2^-126 (ties to even).  The flushed build judges the exact
    product, which is below 2^-126: zero.  test_block_length_matrix[long-ftz-B1024-vm-c2] meets such a product by chance in one sample;
    the restatement (resynth_ref._Ops) flushes the same way, and this case pins both on purpose"""
    import fundsp_amd as F

    V, T = 2, 100
    h = np.array([1.0 - 2.0 ** -24], np.float32)
    x = np.full((V, 1, T), 2.0 ** -126, np.float32)
    x[1] = -x[1]
    assert h[0] < 1 and np.float32(h[0] * x[0, 0, 0]) == np.float32(2.0 ** -126)
    for ftz in (False, True):
        b = F.Bank.convolve(V, h, flush_denormals=ftz)
        got = run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
        same_bits(got, CR.render(x, h, ftz=ftz), f"ftz={ftz}")
        assert np.array_equal(got, np.zeros_like(x) if ftz else x)
