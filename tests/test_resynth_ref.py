"""Host checks of the resynthesizer banks' restatement (tests/resynth_ref.py) and of what the host decides before any launch: the restatement
against the reference's own pass-through test and a float64 STFT, the C library's tables bit for bit, spec validation and graph routing."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import resynth_ref as R


@functools.lru_cache(maxsize=None)
def tabs(N):
    return R.tables(N, O.lib().o_math_cosf)


SIZES = [4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192]   # every window length the library instantiates (LOGN = 2 .. 13)


def test_pass_through_is_the_input_delayed_by_the_window():
    """tests/test_basic.rs:662-686: resynth::<U1, U1, _>(32, pass) returns x[t - 32] from t = 64 on within 1e-6; every N: a stated bound
    (1e-6 up to 256, 2e-6 at 512 and 1024, 4e-6 above)"""
    rng = np.random.default_rng(0)
    for N, tol in ((32, 1e-6), (4, 1e-6), (64, 1e-6), (256, 1e-6), (1024, 2e-6), (4096, 4e-6), (8192, 4e-6),
                   (8, 1e-6), (16, 1e-6), (128, 1e-6), (512, 2e-6), (2048, 4e-6)):
        T = 3 * N + 100
        x = rng.uniform(-1.0, 1.0, (1, 1, T)).astype(np.float32)
        y = R.render(x, N, tabs=tabs(N))
        assert not y[0, 0, :N].any(), "silent for t < N"
        err = np.abs(y[0, 0, 2 * N:] - x[0, 0, N:T - N]).max()
        print(f"pass-through N={N}: max error {err:.3e} (bound {tol:.0e})")
        assert err <= tol, (N, err)


def stft64(x, N, proc_bins):
    """the same resynthesis in float64 on np.fft: window, rfft, per-bin processor, irfft, window * 2/3, overlap-add"""
    T, H = x.shape[-1], N // 4
    n = np.arange(N)
    w = 0.5 + 0.5 * np.cos((n - N / 2) * 2 * np.pi / N)
    y = np.zeros(T)
    for k in range(4, (T - 1) // H + 1):
        seg = x[k * H - N:k * H].astype(np.float64) * w
        Y = proc_bins(np.fft.rfft(seg))
        f = np.fft.irfft(Y, N) * w * (2.0 / 3.0)
        m = min(N, T - k * H)
        y[k * H:k * H + m] += f[:m]
    return y


@pytest.mark.parametrize("N", SIZES)
def test_restated_fft_and_processors_against_float64(N):
    rng = np.random.default_rng(N)
    T = 4 * N + 37
    x = rng.uniform(-1.0, 1.0, (1, 1, T)).astype(np.float32)
    hann, tw = tabs(N)
    # the rfft alone: relative to the spectrum's size
    seg = (x[0, 0, :N] * hann).astype(np.float32)
    Xr, Xi = R.rfft(seg, tw, R._Ops(False))
    ref = np.fft.rfft(seg.astype(np.float64))
    err = np.abs((Xr + 1j * Xi) - ref).max()
    print(f"N={N} rfft: max error {err:.3e}, {100.0 * err / (1e-6 * np.log2(N) * np.abs(ref).max()):.2f} % of the bound")
    assert err <= 1e-6 * np.log2(N) * np.abs(ref).max()
    sr = 44100.0
    lo, hi = 2000.0, 9000.0
    fr = np.float32(np.float32(sr) / np.float32(N)) * np.arange(N // 2 + 1, dtype=np.float32)
    band = (lo <= fr) & (fr <= hi)
    g = rng.uniform(-1.0, 1.0, N // 2 + 1).astype(np.float32)
    for proc, kw, f in (("band", dict(band=(lo, hi)), lambda Y: Y * band), ("gain", dict(gain=g), lambda Y: Y * g.astype(np.float64))):
        y = R.render(x, N, processor=proc, tabs=(hann, tw), **kw)[0, 0]
        want = stft64(x[0, 0], N, f)
        err, bound = np.abs(y - want).max(), 1e-6 * np.log2(N) * max(1.0, np.abs(want).max())
        print(f"N={N} {proc}: max error {err:.3e}, {100.0 * err / bound:.2f} % of the bound {bound:.3e}")
        assert err <= bound, proc


@pytest.mark.parametrize("N", SIZES)
def test_library_tables_equal_the_restatement(N):
    import fundsp_amd as F

    hann = np.zeros(N, np.float32)
    tw = np.zeros(N, np.float32)
    fp = C.POINTER(C.c_float)
    assert F.lib().fdsp_resynth_tables(N, hann.ctypes.data_as(fp), tw.ctypes.data_as(fp)) == 0
    h2, tw2 = tabs(N)
    assert np.array_equal(hann.view(np.uint32), h2.view(np.uint32))
    assert np.array_equal(tw.view(np.uint32), tw2.reshape(-1).view(np.uint32))
    assert F.lib().fdsp_resynth_tables(12, None, None) == -1


def test_invalid_specs_are_refused_before_any_device_work():
    import fundsp_amd as F
    from fundsp_amd import _lib

    L = F.lib()
    cases = ((dict(window_length=2), b"power of two"), (dict(window_length=16384), b"power of two"), (dict(window_length=96), b"power of two"),
             (dict(inputs=0), b"inputs and outputs"), (dict(outputs=9), b"inputs and outputs"), (dict(source=[2]), b"source[0]"),
             (dict(source=[-2]), b"source[0]"), (dict(processor=3), b"processor"), (dict(processor=1), b"lo_hz"), (dict(processor=2), b"gain"),
             (dict(per_instance=2), b"per_instance"))
    for kw, msg in cases:
        s = _lib.ResynthSpec()
        s.window_length, s.inputs, s.outputs = kw.get("window_length", 64), kw.get("inputs", 1), kw.get("outputs", 1)
        s.processor, s.per_instance = kw.get("processor", 0), kw.get("per_instance", 0)
        for o, v in enumerate(kw.get("source", [0])):
            s.source[o] = v
        h = C.c_void_p()
        assert L.fdsp_resynth_create(3, C.byref(s), C.byref(h)) == _lib.EINVAL, kw
        assert msg in L.fdsp_last_error(), (kw, L.fdsp_last_error())
        assert not h.value
    s = _lib.ResynthSpec()
    s.window_length, s.inputs, s.outputs = 64, 1, 1
    assert L.fdsp_resynth_create(0, C.byref(s), C.byref(C.c_void_p())) == _lib.EINVAL


def test_graph_notation_checks_and_routes():
    from fundsp_amd import Bank
    from fundsp_amd import graph as G

    for args, kw in (((1000,), {}), ((64, 0, 1), {}), ((64, 1, 9), {}), ((64, 2, 2), dict(source=[0, 2])), ((64,), dict(processor="comb")),
                     ((64,), dict(processor="band")), ((64,), dict(processor="gain", gain=np.ones(32))), ((64, 1, 2), dict(processor="band", band=np.ones((3, 2))))):
        with pytest.raises(ValueError):
            G.resynth(*args, **kw)
    r = G.resynth(1024, 2, 2, processor="gain", gain=np.ones((2, 513)))
    assert (r.nin, r.nout) == (2, 2) and r.resynth_plan["source"] == [0, 1] and G.has_resynth(r)
    assert not G.has_resynth(G.noise() >> G.lowpass_hz(1000.0, 1.0))
    # anything but the whole graph or `front >> resynth(..)` is refused on the host, with what is supported
    for bad in (G.noise() >> G.resynth(64) >> G.pass_(), G.resynth(64) + G.pass_(), G.resynth(64) | G.pass_(), G.pass_() >> (G.resynth(64) >> G.pass_())):
        with pytest.raises(ValueError, match="front >> resynth"):
            Bank.from_graph(bad, 2)


def test_setter_tables_are_shaped_on_the_host():
    """Bank.set_band / set_gain hand the library exactly rows x outputs x width floats: one-row shapes broadcast over the outputs, the rest
    is refused before the call (the library reads as many floats as the row count says)"""
    from fundsp_amd.bank import resynth_table_rows

    t = resynth_table_rows((100.0, 900.0), 2, 3, "band")
    assert t.shape == (1, 3, 2) and t.flags.c_contiguous and t.dtype == np.float32 and (t[0, :, 1] == 900.0).all()
    g = np.arange(33, dtype=np.float32)
    t = resynth_table_rows(g, 33, 2, "gain")
    assert t.shape == (1, 2, 33) and (t[0, 1] == g).all()
    assert resynth_table_rows(np.ones((4, 1, 33)), 33, 2, "gain").shape == (4, 2, 33)
    assert resynth_table_rows(np.ones((4, 2, 33)), 33, 2, "gain").shape == (4, 2, 33)
    for bad in (np.ones(32), np.ones((3, 33)), np.ones((2, 3, 33)), np.ones((2, 2, 2, 33)), 1.0, np.ones((0, 2, 33))):
        with pytest.raises(ValueError):
            resynth_table_rows(bad, 33, 2, "gain")
