"""Host-side checks of the reverb search feature (no GPU): the new C ABI symbols in the header, the library, the ctypes table, the C++
wrapper and the Rust shim; NULL handles; the two host restatements of reverb_fitness (tests/reverb_fitness_ref.py) against each other and
against small cases worked out by hand."""
import ctypes as C
import os
import re

import numpy as np

import reverb_fitness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fdsp_reverb4_stereo_delays_create": 5, "fdsp_reverb4_stereo_delays_create_on": 6, "fdsp_reverb4_set_delays": 4,
       "fdsp_bank_fitness_reserve": 1, "fdsp_bank_reverb_fitness": 4}


def test_header_library_and_shims_agree_on_the_new_symbols():
    import fundsp_amd

    fundsp_amd.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fundsp_hip.h")).read(), flags=re.S)
    shim = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust_shim", "src", "lib.rs")).read())
    hpp = open(os.path.join(ROOT, "include", "fundsp_hip.hpp")).read()
    raw = C.CDLL(fundsp_amd._lib.SO_PATH)
    for name, nargs in NEW.items():
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == nargs, f"{name}: not declared with {nargs} parameters in include/fundsp_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert len(fundsp_amd._lib.SYMBOLS[name][1]) == nargs, f"{name}: ctypes signature"
        if name != "fdsp_reverb4_stereo_delays_create":          # (the shim binds the `_on` constructors)
            r = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", shim, flags=re.S)
            assert r and len([a for a in r.group(1).split(",") if a.strip()]) == nargs, f"{name}: rust_shim"
        if name != "fdsp_reverb4_stereo_delays_create_on":
            assert name + "(" in hpp, f"{name}: include/fundsp_hip.hpp"
    for method in ("pub fn reverb4_stereo_delays", "pub fn set_delays", "pub fn fitness_reserve", "pub fn reverb_fitness"):
        assert method in shim, f"HipBank lacks `{method}`"


def test_null_handles_are_einval():
    import fundsp_amd
    from fundsp_amd import _lib

    L = fundsp_amd.lib()
    row = (C.c_float * 32)(*([0.05] * 32))
    out = C.c_void_p()
    assert L.fdsp_bank_reverb_fitness(None, None, None, None) == _lib.EINVAL
    assert L.fdsp_bank_fitness_reserve(None) == _lib.EINVAL
    assert L.fdsp_reverb4_set_delays(None, row, 0, 1) == _lib.EINVAL
    assert L.fdsp_reverb4_stereo_delays_create(4, None, 0, 2.0, C.byref(out)) == _lib.EINVAL and not out.value
    # refused before anything is allocated (no device is touched): a negative delay, a NaN, 127 samples at 44.1 kHz
    for bad in (-0.01, float("nan"), 127.0 / 44100.0):
        row[7] = bad
        assert L.fdsp_reverb4_stereo_delays_create(4, row, 0, 2.0, C.byref(out)) == _lib.EINVAL and not out.value, bad


def test_bank_has_the_new_methods():
    import fundsp_amd

    for name in ("reverb4_stereo_delays", "set_delays", "reverb_fitness", "fitness_reserve"):
        assert callable(getattr(fundsp_amd.Bank, name)), name
    assert "reverb4_stereo" in fundsp_amd.bank.LANE_PER_FRAME_KINDS


def synthetic(n=32768, seed=9):
    """decaying noise behind a silent head, two channels"""
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal((2, n)) * np.exp(-np.arange(n) / 6000.0) * 0.05).astype(np.float32)
    r[:, :2700] = 0.0
    r[1, 5000:5010] = 0.0
    return r


def test_the_two_restatements_agree():
    r = synthetic()
    f64, t64 = R.fitness_f64(r)
    f32, t32 = R.fitness_f32_serial(r)
    assert np.all(t64 > 0) and f64 != 0
    assert abs(float(f32) - f64) <= 1e-4 * abs(f64), (f32, f64)
    assert np.all(np.abs(t32.astype(np.float64) - t64) <= 1e-4 * np.abs(t64)), (t32, t64)
    assert abs(f64 - (t64[0] - t64[1] + t64[2] - t64[3])) <= 1e-12 * abs(f64)
    # the echo term counts what it says: 10 samples fewer on channel 1
    assert len(R.echo_weights(r[0])) == 32768 - 2700 and len(R.echo_weights(r[1])) == 32768 - 2700 - 10


def test_hand_computed_64_sample_case():
    n = 64
    # the window: 0.5 + 0.5 cos((i - 32) 2 pi / 64) -- 0 at i = 0, 1/2 at 16 and 48, 1 at 32, (2 - sqrt 2) / 4 at 8
    for w in (R.hann_f64(n), R.hann_f32(n).astype(np.float64)):
        assert abs(w[0]) < 1e-7 and abs(w[16] - 0.5) < 1e-7 and abs(w[48] - 0.5) < 1e-7 and abs(w[32] - 1.0) < 1e-7
        assert abs(w[8] - (2.0 - np.sqrt(2.0)) / 4.0) < 1e-7 and np.allclose(w[1:], w[1:][::-1], atol=1e-7)
    # the packed bin 0: x = 3 + 2 (-1)^i has DC = 64 * 3 and Nyquist = 64 * 2 and nothing else; |bin 0| = 64 sqrt(13)
    x = 3.0 + 2.0 * (-1.0) ** np.arange(n)
    s = R.packed_spectrum(x)
    assert s.shape == (32,) and abs(s[0] - complex(192.0, 128.0)) < 1e-9 and np.all(np.abs(s[1:]) < 1e-9)
    assert abs(abs(s[0]) - 64.0 * np.sqrt(13.0)) < 1e-9
    # the 50-bin sliding mean: norm_k = k over 64 bins has mean_k = (k - 50 + .. + k - 1) / 50 = k - 25.5, so every bin from 51 on lies
    # 25.5 above it: pen = 0.1 * 13 * 25.5^2 = 845.325
    norm = np.arange(64, dtype=np.float64)
    assert abs(R.penalty_f64(norm) - 845.325) < 1e-9
    p32 = R.penalty_terms_f32(norm.astype(np.float32))
    assert p32.shape == (13,) and np.allclose(p32, 65.025, rtol=1e-6)
    # ... and a bin below the mean adds nothing: with norm_60 = 0 bin 60 drops out and the means of 61 .. 63 fall by 60 / 50 = 1.2
    norm[60] = 0.0
    want = 0.1 * (9 * 25.5 ** 2 + 3 * 26.7 ** 2)
    assert abs(R.penalty_f64(norm) - want) < 1e-9
    assert abs(float(np.sum(R.penalty_terms_f32(norm.astype(np.float32)), dtype=np.float64)) - want) < 1e-3
    # a whole 64-sample response through both restatements with a window of 5 bins: echo = H_63 - 1 - 1/2 for a response silent at i = 1, 2
    r = np.ones((2, n), dtype=np.float32)
    r[:, 1:3] = 0.0
    f64, t64 = R.fitness_f64(r, window=5)
    f32, t32 = R.fitness_f32_serial(r, window=5)
    h63 = float(np.sum(1.0 / np.arange(1, 64)))
    assert abs(t64[0] - (h63 - 1.5)) < 1e-12 and abs(t64[2] - (h63 - 1.5)) < 1e-12
    assert np.all(np.abs(t32.astype(np.float64) - t64) <= 1e-4 * np.maximum(np.abs(t64), 1e-3)) and abs(float(f32) - f64) <= 1e-4 * abs(f64)
