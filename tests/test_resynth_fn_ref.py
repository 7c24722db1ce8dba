"""Host checks of the resynthesizer banks' closure path: the functor compiler without a device (fdsp_resynth_fn_check), the argument checks
of graph.resynth_fn / Bank.resynth_fn, and the restatement tests/resynth_fn_ref.py -- the stock processors written as closures against
tests/resynth_ref.py bit for bit, the README's band-pass against the reference's pass-through check, and a bin shift and a cross-synthesis
against a float64 STFT."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import resynth_fn_cases as K
import resynth_fn_ref as RF
import resynth_ref as R

f32 = np.float32


@functools.lru_cache(maxsize=None)
def tabs(N):
    return R.tables(N, O.lib().o_math_cosf)


def fn_spec(case, N=64, **over):
    from fundsp_amd import bank as B

    plan = dict(case.spec(N))
    plan.update({k: v for k, v in over.items() if k in plan})
    return B.resynth_fn_spec(plan, over.get("params", case.params), over.get("flush_denormals", False))


def test_check_compiles_the_example_functors_without_a_device():
    from fundsp_amd import _lib

    L = _lib.lib()
    cases = list(K.CLOSURES.values()) + [K.FOREIGN] + [K.stock(p, 64, 2, 2, [1, 0]) for p in ("pass", "band", "gain")]
    for case in cases:
        for ftz in (False, True):
            s = fn_spec(case, flush_denormals=ftz)
            assert L.fdsp_resynth_fn_check(C.byref(s)) == _lib.OK, (case.functor, L.fdsp_last_error().decode())
    # the header's own examples, as printed there
    header = ("struct Pass { static constexpr int PARAMS = 0, STATE = 0;\n template <class W> static __device__ void bin(W& fft, int i) { fft.set(0, i, fft.at(0, i)); } };\n"
              "struct Band { static constexpr int PARAMS = 2, STATE = 0;\n template <class W> static __device__ void bin(W& fft, int i) {\n"
              " const float f = fft.frequency(i);\n if (fft.param(0) <= f && f <= fft.param(1)) fft.set(0, i, fft.at(0, i)); } };\n"
              "template <int BINS> struct Gain { static constexpr int PARAMS = BINS, STATE = 0;\n"
              " template <class W> static __device__ void bin(W& fft, int i) { fft.set(0, i, fft.at(0, i) * fft.param(i)); } };\n")
    for functor, P in (("Pass", 0), ("Band", 2), ("Gain<33>", 33)):
        s = fn_spec(K.Case(functor, header, None, params=P))
        assert L.fdsp_resynth_fn_check(C.byref(s)) == _lib.OK, (functor, L.fdsp_last_error().decode())


def test_check_rejects_bad_functors_with_the_compilers_log():
    from fundsp_amd import _lib

    L = _lib.lib()
    broken = K.Case("Broken", K.GATE.source.replace("Gate", "Broken").replace("fft.set(0, i, x);", "fft.set(0, i, x) oops;"), None, params=1)
    assert L.fdsp_resynth_fn_check(C.byref(fn_spec(broken))) == _lib.EINVAL
    msg = L.fdsp_last_error().decode()
    assert "error:" in msg and "oops" in msg, msg
    for over, word in ((dict(params=2), "PARAMS"), (dict(params=0), "PARAMS")):
        assert L.fdsp_resynth_fn_check(C.byref(fn_spec(K.GATE, **over))) == _lib.EINVAL
        assert word in L.fdsp_last_error().decode(), L.fdsp_last_error().decode()
    assert L.fdsp_resynth_fn_check(C.byref(fn_spec(K.SMOOTH, state=1))) == _lib.EINVAL
    assert "STATE" in L.fdsp_last_error().decode()
    assert L.fdsp_resynth_fn_check(C.byref(fn_spec(K.GATE, state=2))) == _lib.EINVAL
    assert "STATE" in L.fdsp_last_error().decode()
    # the spec itself
    for over, word in ((dict(window=48), "power of two"), (dict(inputs=9), "inputs and outputs"), (dict(state=17), "state"), (dict(functor="Gate; int x"), "functor")):
        assert L.fdsp_resynth_fn_check(C.byref(fn_spec(K.GATE, **over))) == _lib.EINVAL
        assert word in L.fdsp_last_error().decode(), L.fdsp_last_error().decode()
    assert L.fdsp_resynth_fn_check(None) == _lib.EINVAL
    # creation refuses the same before any device work
    h = C.c_void_p()
    assert L.fdsp_resynth_fn_create(4, C.byref(fn_spec(broken)), C.byref(h)) == _lib.EINVAL and not h.value
    assert "oops" in L.fdsp_last_error().decode()
    assert L.fdsp_resynth_fn_create(0, C.byref(fn_spec(K.GATE)), C.byref(h)) == _lib.EINVAL and not h.value
    assert L.fdsp_resynth_set_params(None, None, 0, 0) == _lib.EINVAL


def test_argument_checks_raise_before_the_library_is_called(monkeypatch):
    import fundsp_amd as F
    from fundsp_amd import _lib
    from fundsp_amd import graph as GR

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(F.bank, "lib", no_library)
    g = K.GATE
    for make in (lambda **kw: GR.resynth_fn(**kw), lambda **kw: F.Bank.resynth_fn(3, **kw)):
        for bad in (dict(window=48), dict(window=2), dict(window=16384), dict(inputs=0), dict(outputs=9), dict(state=17), dict(state=-1), dict(functor=""),
                    dict(source=" ")):
            kw = dict(g.spec(64))
            kw.update(bad)
            with pytest.raises(ValueError):
                make(**kw)
        with pytest.raises(ValueError):
            make(**g.spec(64), threshold=np.ones((2, 2)))                       # a parameter is a scalar or a per-instance vector
        with pytest.raises(ValueError):
            make(**g.spec(64), a=np.ones(3), b=np.ones(4))                      # per-instance parameters of different lengths
        with pytest.raises(ValueError):
            make(**g.spec(64), param_values=np.ones((2, 1, 1)))
        with pytest.raises(ValueError):
            make(**g.spec(64), param_values=[1.0], threshold=1.0)
    with pytest.raises(ValueError):
        F.Bank.resynth_fn(3, **g.spec(64), threshold=np.ones(4))                # 4 values for 3 instances
    # keyword order = parameter index; scalars broadcast over the per-instance arrays
    t = GR.resynth_fn(64, "X", "struct X {};", a=1.0, b=np.array([2.0, 3.0]), c=4.0).resynth_fn_plan["param_values"]
    assert t.dtype == np.float32 and t.tolist() == [[1.0, 2.0, 4.0], [1.0, 3.0, 4.0]]
    assert GR.resynth_fn(64, "X", "struct X {};", a=1.0, b=2.0).resynth_fn_plan["param_values"].tolist() == [1.0, 2.0]
    assert GR.resynth_fn(64, "X", "struct X {};").resynth_fn_plan["param_values"] is None
    with pytest.raises(ValueError, match="resynth_fn"):
        GR.resynth(64, processor="gate")


def test_graph_routes_the_node_alone_and_behind_a_front(monkeypatch):
    import fundsp_amd as F
    from fundsp_amd import graph as GR

    made = []
    monkeypatch.setattr(F.Bank, "resynth_fn", classmethod(lambda cls, voices, **kw: made.append((voices, kw)) or "bank"))
    assert F.Bank.from_graph(GR.resynth_fn(**K.GATE.spec(64), threshold=0.5), 5) == "bank"
    assert made[0][0] == 5 and made[0][1]["functor"] == "Gate" and made[0][1]["flush_denormals"] is False
    g = GR.noise() >> GR.resynth_fn(**K.GATE.spec(64), threshold=0.5)
    assert g.pipe_parts[1].resynth_fn_plan["window"] == 64 and GR.has_resynth(g)
    with pytest.raises(ValueError):
        F.Bank.from_graph(GR.resynth_fn(**K.GATE.spec(64)) >> GR.resynth_fn(**K.GATE.spec(64)), 2)


IO = [(1, 1), (2, 2), (1, 2), (2, 1)]
SOURCES = {(1, 1): [0], (2, 2): [1, 0], (1, 2): [0, -1], (2, 1): [1]}


@pytest.mark.parametrize("N", [4, 32, 1024])
@pytest.mark.parametrize("io", IO)
def test_stock_processors_as_closures_equal_the_stock_restatement(N, io):
    I, O_ = io
    V, T = 2, 3 * N + 7
    rng = np.random.default_rng(N + I)
    x = rng.uniform(-1.0, 1.0, (V, I, T)).astype(f32)
    x[1] *= f32(2.0 ** -120)   # into the denormal range: the flushed build differs
    NB = N // 2 + 1
    lo = rng.uniform(0.0, 8000.0, (V, O_)).astype(f32)
    band = np.stack([lo, lo + f32(6000.0)], axis=-1)
    gain = rng.uniform(-1.5, 1.5, (V, O_, NB)).astype(f32)
    for proc, kw in (("pass", {}), ("band", dict(band=band)), ("gain", dict(gain=gain))):
        for ftz in (False, True):
            case = K.stock(proc, N, I, O_, SOURCES[io])
            want = R.render(x, N, O_, proc, SOURCES[io], tabs=tabs(N), ftz=ftz, **kw)
            got = RF.render(x, N, case.closure, O_, params=K.stock_params(proc, V, O_, NB, **kw), tabs=tabs(N), ftz=ftz)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (proc, ftz)


def test_setters_apply_to_the_frames_above_the_change():
    N, V, T1, T = 32, 2, 100, 260
    x = np.random.default_rng(3).uniform(-1.0, 1.0, (V, 1, T)).astype(f32)
    case = K.stock("band", N, 1, 1, [0])
    b1, b2 = (1000.0, 9000.0), (3000.0, 12000.0)
    want = R.render(x, N, processor="band", band=b1, changes=[(T1, dict(band=b2, sample_rate=22050.0))], tabs=tabs(N))
    got = RF.render(x, N, case.closure, params=np.array(b1, f32), changes=[(T1, dict(params=np.array(b2, f32), sample_rate=22050.0))], tabs=tabs(N))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_readme_band_pass_passes_the_pass_through_check_inside_its_band():
    """README.md:836-857 (window 1024, pass band 1000 .. 2000 Hz) fed a sine on bin 35 (1507 Hz): its Hann-windowed spectrum lives on bins
    34 .. 36, inside the band, so the output is the input delayed by the window from t = 2 N on within the reference's tolerance of 1e-6
    (tests/test_basic.rs:676-685); a sine on bin 100 (4307 Hz), outside, is silenced to the same tolerance"""
    N, sr = 1024, 44100.0
    T = 4 * N

    def readme(fft):
        fr = fft.frequency(fft.i)
        fft.set(0, fft.at(0, fft.i), where=(fr >= f32(1000.0)) & (fr <= f32(2000.0)))

    t = np.arange(T)
    for b, inside in ((35, True), (100, False)):
        x = (0.5 * np.sin(2 * np.pi * b * t / N + 0.3)).astype(f32)[None, None]
        y = RF.render(x, N, readme, sample_rate=sr, tabs=tabs(N))
        want = x[0, 0, N:T - N] if inside else np.zeros(T - 2 * N, f32)
        err = np.abs(y[0, 0, 2 * N:] - want).max()
        print(f"README band-pass, bin {b}: max error {err:.3e}")
        assert err <= 1e-6, (b, err)


def stft64(x, N, proc_bins, O_=1):
    """the resynthesis in float64 on np.fft: x [I, T] -> y [O, T]"""
    T, H = x.shape[-1], N // 4
    n = np.arange(N)
    w = 0.5 + 0.5 * np.cos((n - N / 2) * 2 * np.pi / N)
    y = np.zeros((O_, T))
    for k in range(4, (T - 1) // H + 1):
        X = np.fft.rfft(x[:, k * H - N:k * H].astype(np.float64) * w, axis=-1)
        f = np.fft.irfft(proc_bins(X), N, axis=-1) * w * (2.0 / 3.0)
        m = min(N, T - k * H)
        y[:, k * H:k * H + m] += f[:, :m]
    return y


# max |y - y64| / max |y64| of the restatement against the float64 STFT, measured with the inputs below (seed N):
#   shift by 3 bins:   N = 32: 1.586e-07,  N = 1024: 2.225e-07,  N = 8192: 2.159e-07
#   cross-synthesis:   N = 32: 3.395e-07,  N = 1024: 3.758e-07,  N = 8192: 4.026e-07
# The bound is 4 x the largest of them (the convolver's margin: the bound must not move with the seed).
ACCURACY_BOUND = 4 * 4.026e-07


@pytest.mark.parametrize("N", [32, 1024, 8192])
def test_shift_and_cross_synthesis_against_float64(N):
    rng = np.random.default_rng(N)
    T = 4 * N + 37
    x = rng.uniform(-1.0, 1.0, (1, 2, T)).astype(f32)
    NB = N // 2 + 1

    def shift64(X):
        Y = np.zeros_like(X[:1])
        Y[0, 3:] = X[0, :NB - 3]
        return Y

    y = RF.render(x[:, :1], N, K.SHIFT.closure, params=np.array([3.0], f32), tabs=tabs(N))[0]
    want = stft64(x[0, :1], N, shift64)
    e_shift = np.abs(y - want).max() / np.abs(want).max()
    y = RF.render(x, N, K.CROSS.closure, tabs=tabs(N))[0]
    want = stft64(x[0], N, lambda X: X[:1] * X[1:2])
    e_cross = np.abs(y - want).max() / np.abs(want).max()
    print(f"N = {N}: shift {e_shift:.3e}, cross-synthesis {e_cross:.3e} (relative to max |y64|)")
    assert e_shift <= ACCURACY_BOUND and e_cross <= ACCURACY_BOUND, (N, e_shift, e_cross)
