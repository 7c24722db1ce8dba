"""GPU parity of the resynthesizer banks at every window length and across the wrap of both rings: k_rs_frames / k_rs_forward / k_rs_inverse
<LOGN> for LOGN = 2 .. 13 in the IEEE and the flush-to-zero build, each launched by a test that is bit-exact against the numpy restatement
(tests/resynth_ref.py, tests/resynth_fn_ref.py) -- the window lengths the matrices of test_gpu_resynth.py / test_gpu_resynth_fn.py leave out
(8, 16, 64, 128, 512, 2048; the lane geometry P = min(N/2, 256), G = 256 / P changes inside them), one instance in a workgroup of 64 units and
of one, streams of ragged launches long enough to wrap the input ring (& (Rx - 1)) and the frame ring (k % R, R no power of two) with a clone
and a reset behind the wrap, the 8-slot frame ring of a large bank, and subnormal data through both builds at every size."""
import functools

import numpy as np
import pytest

import resynth_fn_cases as K
import resynth_ref as R
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS
from test_gpu_parity import assert_bit_equal, run_bank
from test_gpu_resynth import IO, SOURCES, signal, tables_for, tabs
from test_gpu_resynth_fn import bits_equal, make, run_split, want_of

pytestmark = pytest.mark.gpu
f32 = np.float32

SIZES = [4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]
MISSING = [8, 16, 64, 128, 512, 2048]   # the sizes the two existing matrices do not run
PROCS = ["pass", "band", "gain"]


def ring_sizes(N, V, I, O, closure=False):
    """(R, Lmax, Fc, Rx) as the library sizes a bank: rs_ring, fx_resynth and fx_resynth_fn of fundsp_amd/csrc/fd_fxbank.hip restated.
    R frame slots (at least 8, at most a 64 Ki-sample chunk, within 256 MiB), chunks of Lmax samples, Fc frames per chunk on the closure path,
    an input ring of Rx samples (the power of two that holds a chunk and a window)."""
    H = N // 4
    R = max(8, min((256 << 20) // (V * O * N * 4), 5 + 65536 // H))
    Lmax, Fc = (R - 5) * H, None
    if closure:
        Fc = max(2, min((R * O * N) // (2 * (I + O) * (N // 2 + 1)), R - 4))
        Lmax = (Fc - 1) * H
    Rx = 1
    while Rx < Lmax + N:
        Rx <<= 1
    return R, Lmax, Fc, Rx


def assert_both_rings_wrap(T, N, R, Rx):
    H = N // 4
    assert T > Rx + N, f"N={N}: {T} samples do not carry a whole window past the input ring's wrap (Rx = {Rx})"
    assert T > (R + 4) * H, f"N={N}: {T} samples do not reuse four slots of the frame ring (R = {R}, H = {H})"


def ragged(T, first):
    """launches off the hop grid, one straddling sample `first` and the few frames after it, one longer than a chunk"""
    lens = [7, first - 6, 1, 64, 64, min(70000, T // 2)]
    lens.append(T - sum(lens))
    assert min(lens) > 0 and sum(lens) == T
    return lens


# ---- A. every window length ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", MISSING)
@pytest.mark.parametrize("io", IO)
@pytest.mark.parametrize("proc", PROCS)
def test_stock_banks_at_the_remaining_window_lengths(gpu, N, io, proc):
    """test_matrix_bit_exact of test_gpu_resynth.py at the six other sizes: k_rs_frames<3, 4, 6, 7, 9, 11>"""
    import fundsp_amd as F

    I, O_ = io
    V, T = 3, 3 * N + 7
    x = signal(V, I, T, seed=N + 10 * I + O_)
    t = tables_for(proc, N, O_)
    b = F.Bank.resynth(V, N, I, O_, processor=proc, source=SOURCES[io], **t)
    want = R.render(x, N, O_, proc, SOURCES[io], tabs=tabs(N), **t)
    assert np.any(want != 0)
    bits_equal(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), want, f"N={N} {I}->{O_} {proc}")


@pytest.mark.parametrize("N", MISSING)
@pytest.mark.parametrize("io,proc", [(io, p) for io in IO for p in ("pass", "band")] + [((1, 1), "gain")])
def test_stock_functors_at_the_remaining_window_lengths(gpu, N, io, proc):
    """test_stock_functors_equal_the_stock_banks of test_gpu_resynth_fn.py at the six other sizes (k_rs_forward / k_rs_inverse<3, 4, 6, 7, 9,
    11>): the functor bank against the stock bank AND the restatement.  pass and band compile once for all sizes; gain is per size: 1 -> 1"""
    import fundsp_amd as F

    I, O_ = io
    V, T, NB = 3, 3 * N + 7, N // 2 + 1
    x = signal(V, I, T, seed=N + 10 * I + O_ + 1)
    kw = tables_for(proc, N, O_, V=V, seed=N)
    stock = F.Bank.resynth(V, N, I, O_, processor=proc, source=SOURCES[io], **kw)
    fn = make(K.stock(proc, N, I, O_, SOURCES[io]), V, N, K.stock_params(proc, V, O_, NB, **kw))
    want = R.render(x, N, O_, proc, SOURCES[io], tabs=tabs(N), **kw)
    assert np.any(want != 0)
    got = run_bank(fn, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    bits_equal(got, run_bank(stock, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), f"N={N} {I}->{O_} {proc}: functor bank against the stock bank")
    bits_equal(got, want, f"N={N} {I}->{O_} {proc}: functor bank against the restatement")


@pytest.mark.parametrize("N", [8, 512])
@pytest.mark.parametrize("io", IO)
def test_one_instance(gpu, N, io):
    """V = 1: at N = 8 a 1 -> 1 launch's 16 units (3N + 7 samples: 15 frames and one more) fill a quarter of ONE workgroup of 64 units, at
    N = 512 a workgroup is one unit"""
    import fundsp_amd as F

    I, O_ = io
    T, NB = 3 * N + 7, N // 2 + 1
    x = signal(1, I, T, seed=N + 3 * I + O_)
    for proc in PROCS:
        t = tables_for(proc, N, O_, V=1, seed=N + 1)
        want = R.render(x, N, O_, proc, SOURCES[io], tabs=tabs(N), **t)
        b = F.Bank.resynth(1, N, I, O_, processor=proc, source=SOURCES[io], **t)
        bits_equal(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), want, f"N={N} {I}->{O_} {proc}, one instance")
        if proc != "gain":
            fn = make(K.stock(proc, N, I, O_, SOURCES[io]), 1, N, K.stock_params(proc, 1, O_, NB, **t))
            bits_equal(run_bank(fn, x, T, LAYOUT_PLANAR, MODE_PROCESS), want, f"N={N} {I}->{O_} {proc} functor, one instance")


# ---- B. streams that wrap both rings ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(len(SIZES)), ids=[f"N{N}" for N in SIZES])
def test_stock_stream_wraps_both_rings_then_clone_and_reset(gpu, n):
    """2 instances, 140 000 samples in ragged launches: the input ring (131 072 samples) wraps once, the frame ring (5 + 65536 / H slots) once
    or twice; I/O shape and processor rotate over the sizes (2 -> 2 with source [1, 0] at N = 8, 128, 2048; per-instance gain tables at N =
    16, 128, 1024, 8192).  Then a clone continues like its source, and a reset bank -- stale frames in every slot -- renders like a fresh one"""
    import fundsp_amd as F

    N, io, proc = SIZES[n], IO[n % 4], PROCS[n % 3]
    I, O_ = io
    V, T, T2, T3 = 2, 140000, N + 100, 3 * N + 7
    Rr, Lmax, _, Rx = ring_sizes(N, V, I, O_)
    assert_both_rings_wrap(T, N, Rr, Rx)
    assert (Lmax, Rx) == (65536, 131072)
    lens = ragged(T, 65536)
    x = signal(V, I, T + T2, seed=40 + n)
    t = tables_for(proc, N, O_, V=V, seed=n)
    want = R.render(x, N, O_, proc, SOURCES[io], tabs=tabs(N), **t)
    layout = (LAYOUT_VOICE_MINOR, LAYOUT_PLANAR)[n % 2]
    b = F.Bank.resynth(V, N, I, O_, processor=proc, source=SOURCES[io], **t)
    bits_equal(run_split(b, x[:, :, :T], lens, layout), want[:, :, :T], f"N={N} {I}->{O_} {proc}: the stream")
    assert np.any(want[:, :, T - 2 * N:T] != 0)
    c = b.clone()
    tail = np.ascontiguousarray(x[:, :, T:])
    bits_equal(run_bank(b, tail, T2, layout, MODE_PROCESS), want[:, :, T:], f"N={N}: the source beyond the stream")
    bits_equal(run_bank(c, tail, T2, layout, MODE_PROCESS), want[:, :, T:], f"N={N}: the clone beyond the stream")
    b.reset()
    head = np.ascontiguousarray(x[:, :, :T3])   # (the restatement is causal: a fresh bank's first samples are the stream's)
    bits_equal(run_bank(b, head, T3, layout, MODE_PROCESS), want[:, :, :T3], f"N={N}: after reset")


@pytest.mark.parametrize("N,T", [(32, 70000), (512, 140000)])
@pytest.mark.parametrize("name", ["mid_side", "shift", "smooth"])
def test_closure_stream_wraps_both_rings(gpu, name, N, T):
    """The closure path's chunk is bounded by Fc: an input ring of 32 768 samples at N = 32 and of 65 536 at N = 512.  2 instances in ragged
    launches across the wraps of k_rs_forward's input ring and k_rs_inverse's frame ring; `smooth` carries per-bin state across both"""
    case = K.CLOSURES[name]
    V = 2
    Rr, Lmax, Fc, Rx = ring_sizes(N, V, case.inputs, case.outputs, closure=True)
    assert_both_rings_wrap(T, N, Rr, Rx)
    assert (Fc, Lmax, Rx) == {32: (3857, 30848, 32768), 512: (257, 32768, 65536)}[N]
    lens = ragged(T, Rx)
    assert max(lens) > Lmax
    x = signal(V, case.inputs, T, seed=N + 2)
    p = K.case_params(name, V, N, seed=5)
    want = want_of(case, x, N, p)
    assert np.any(want[:, :, T - 2 * N:] != 0)
    bits_equal(run_split(make(case, V, N, p), x, lens, LAYOUT_PLANAR if N == 32 else LAYOUT_VOICE_MINOR), want, f"{name} N={N}: the stream")


# ---- C. the smallest frame ring -----------------------------------------------------------------------------------------------------

def test_eight_slot_frame_ring(gpu):
    """1025 instances of N = 8192: 256 MiB / (1025 x 32 KiB) = 7 slots, clamped to R = 8 -- a chunk of 3 H samples launches 4 units per
    instance, 3 of which complete a frame, and its overlap-add reads those and the 4 before them: 7 of the 8 slots.  20 000 samples in launches off the hop grid: frame 8 takes slot 0 again at sample 16 384, where
    the input ring wraps too"""
    import fundsp_amd as F

    N, V, T = 8192, 1025, 20000
    H = N // 4
    Rr, Lmax, _, Rx = ring_sizes(N, V, 1, 1)
    assert (Rr, Lmax, Rx) == (8, 3 * H, 16384)
    assert T > Rx and T > (Rr + 1) * H, "the input ring wraps and frames R, R + 1 reuse slots 0, 1"
    lens = [5, 6144, 6143, T - 5 - 6144 - 6143]
    x = signal(V, 1, T, seed=8)
    got = run_split(F.Bank.resynth(V, N), x, lens)
    sel = [0, 512, 1024]
    want = R.render(x[sel], N, tabs=tabs(N))
    assert np.any(want[:, :, 9 * H:] != 0)
    for n, v in enumerate(sel):
        assert_bit_equal(got[v], want[n], f"instance {v}")


# ---- D. the flush-to-zero build at every size ---------------------------------------------------------------------------------------

GAIN_SIZES = (16, 512, 4096)


def subnormal_scale(N):
    """2^-118: normal samples whose window products and frames / N fall among the denormals.  At N = 4 the window is (0, 1/2, 1, 1/2) and
    1 / N = 1/4: the products are exact and few of them leave the normal range, so the data sits at 2^-122 there (17 of 19 samples still
    normal, 14 output samples differ between the builds)"""
    return f32(2.0 ** (-122 if N == 4 else -118))


@functools.lru_cache(maxsize=None)
def subnormal_case(N, proc):
    """x [2, 1, 3N + 7], the tables, and the restatement's output in the IEEE and in the flushed build -- which must tell the builds apart"""
    V, T = 2, 3 * N + 7
    x = signal(V, 1, T, seed=17 + N)
    x[0] *= f32(2.0 ** -130)      # instance 0: subnormal input samples
    x[1] *= subnormal_scale(N)    # instance 1: see subnormal_scale
    assert np.all(np.abs(x[0]) < f32(2.0 ** -126)) and np.any(x[0] != 0)
    t = tables_for(proc, N, 1, seed=N)
    want = {ftz: R.render(x, N, 1, proc, tabs=tabs(N), ftz=ftz, **t) for ftz in (False, True)}
    assert np.any(want[False][0] != 0) and not np.any(want[True][0]), "a denormal input comes through the IEEE build and reads as zero when flushed"
    assert np.any(want[False][1] != want[True][1]), "the builds differ on data that falls among the denormals"
    assert np.any(want[False][1] != 0) and np.any(want[True][1] != 0)
    return x, t, want


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("ftz", [False, True], ids=["ieee", "flushed"])
def test_subnormal_data_every_window_length(gpu, N, ftz):
    """k_rs_frames<LOGN> of rs_ieee and of rs_ftz at every size: pass, and gain at three sizes"""
    import fundsp_amd as F

    for proc in ("pass", "gain") if N in GAIN_SIZES else ("pass",):
        x, t, want = subnormal_case(N, proc)
        b = F.Bank.resynth(2, N, processor=proc, flush_denormals=ftz, **t)
        bits_equal(run_bank(b, x, x.shape[2], LAYOUT_VOICE_MINOR, MODE_PROCESS), want[ftz], f"N={N} {proc}, ftz={ftz}")


@pytest.mark.parametrize("N", SIZES)
def test_subnormal_data_flushed_closure_path(gpu, N):
    """k_rs_forward / k_rs_inverse<LOGN> of rs_ftz at every size (one functor, compiled once with the flush-to-zero flags): the pass functor
    against the flushed stock bank and the flushed restatement"""
    import fundsp_amd as F

    x, _, want = subnormal_case(N, "pass")
    T = x.shape[2]
    got = run_bank(make(K.stock("pass", N, 1, 1, [0]), 2, N, flush_denormals=True), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    bits_equal(got, run_bank(F.Bank.resynth(2, N, flush_denormals=True), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), f"N={N}: against the flushed stock bank")
    bits_equal(got, want[True], f"N={N}: against the flushed restatement")
