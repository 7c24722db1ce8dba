"""The time-split kernel with the time-parallel filter stage (fd_tsp.hpp k_render_ts3p; "svf_exec" = FDSP_SVF_PARALLEL, tolerance mode).

Truth without another oracle: a twin bank X whose filters are bells of gain 1 (m0 = 1, m1 = m2 = 0) renders the filter's INPUT through
the serial kernel, bit for bit; the f64 tick in numpy over that input, with the coefficients read back from the bank under test, is the
truth.  The bound is the host check's (tests/test_svf_par_host.py): per voice err_par <= R * err_ser + 2^-23 * peak, and bank-wide the
parallel form's worst error is no larger than the serial tolerance-mode kernel's.  Everywhere the kernel does not apply the launch is
the one "svf_exec" = 0 makes, bit for bit."""
import numpy as np
import pytest

import oracle as O
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MATH_EXACT, MATH_FAST, MIX_SUM, MODE_PROCESS, MODE_TICK, SVF_PARALLEL, SVF_SERIAL
from fundsp_amd import graph as GR
from fundsp_amd import workloads as W
from test_gpu_parity import assert_bit_equal, run_bank
from test_svf_par_host import R

pytestmark = pytest.mark.gpu
SR = 48000.0
LK_TIME_SPLIT, LK_TIME_SPLIT_SVF = 4, 11
BELL = 6


def fm_bank(p, svf_exec, math=MATH_FAST, modes=None, gain=2.0):
    """config 3 with per-voice filter modes (default: all nine spread over the voices; bells and shelves with `gain`)"""
    b = W.make_fm_svf_bank(len(p["f"]), SR, params=p)
    b.set_param(W.FM_SLOTS["mode"], (np.arange(len(p["f"])) % 9 if modes is None else modes).astype(np.float32))
    b.set_param(W.FM_SLOTS["gain"], gain)
    b.set_sample_rate(SR)
    b.set_option("math", math)
    b.set_option("svf_exec", svf_exec)
    return b


def filter_input_bank(p):
    """X: the same oscillators in tolerance mode, every filter a bell of gain 1 -- its output IS the filter's input"""
    x = fm_bank(p, SVF_SERIAL, modes=np.full(len(p["f"]), BELL), gain=1.0)
    assert np.all(x.get_slot("1:m0") == 1.0) and not x.get_slot("1:m1").any() and not x.get_slot("1:m2").any()
    return x


def f64_truth(bank, x, s1=None, s2=None):
    """the reference tick (svf.rs:995-1006) in f64 over x [V][T], coefficients of `bank`"""
    a1, a2, a3, m0, m1, m2 = (bank.get_slot("1:" + n).astype(np.float64) for n in ("a1", "a2", "a3", "m0", "m1", "m2"))
    V, T = x.shape
    ic1 = np.zeros(V) if s1 is None else s1.astype(np.float64)
    ic2 = np.zeros(V) if s2 is None else s2.astype(np.float64)
    y = np.empty((V, T))
    with np.errstate(all="ignore"):
        for t in range(T):
            v0 = x[:, t].astype(np.float64)
            v3 = v0 - ic2
            v1 = a1 * ic1 + a2 * v3
            v2 = ic2 + a2 * ic1 + a3 * v3
            ic1 = 2.0 * v1 - ic1
            ic2 = 2.0 * v2 - ic2
            y[:, t] = m0 * v0 + m1 * v1 + m2 * v2
    return y


def errors(got, truth):
    fin = np.isfinite(truth)
    with np.errstate(all="ignore"):
        err = np.where(fin, np.abs(got.astype(np.float64) - truth), 0.0).max(axis=1)
        peak = np.where(fin, np.abs(truth), 0.0).max(axis=1)
    return err, peak


def assert_within_bound(par, ser, truth, what, bank_wide=True):
    err_par, peak = errors(par, truth)
    err_ser, _ = errors(ser, truth)
    with np.errstate(all="ignore"):
        ratio = np.where(err_ser > 0, err_par / np.where(err_ser > 0, err_ser, 1.0), 0.0)
    print(f"\n{what}: worst error parallel {err_par.max():.3e} serial {err_ser.max():.3e}; parallel worse in {(err_par > err_ser).sum()} of "
          f"{len(err_par)} voices, by at most {ratio.max():.3f} x (R = {R:.3f}); peaks {peak.min():.2e} .. {peak.max():.2e}")
    slack = err_par - (R * err_ser + np.ldexp(peak, -23))
    assert (slack <= 0).all(), f"{what}: voice {slack.argmax()} err_par {err_par[slack.argmax()]:.3e} err_ser {err_ser[slack.argmax()]:.3e}"
    if bank_wide:
        assert err_par.max() <= err_ser.max(), what


def render(b, T):
    return run_bank(b, None, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)[:, 0, :]


def test_accuracy_all_modes(gpu):
    V, T = 192, 4096
    p = W.fm_svf_params(V, SR)
    par, ser, x = fm_bank(p, SVF_PARALLEL), fm_bank(p, SVF_SERIAL), filter_input_bank(p)
    assert par.get_option("has_svf_parallel") == 1 and par.get_option("svf_exec") == SVF_PARALLEL
    yp, ys, xin = render(par, T), render(ser, T), render(x, T)
    assert (par.get_option("last_kernel"), ser.get_option("last_kernel"), x.get_option("last_kernel")) == (LK_TIME_SPLIT_SVF, LK_TIME_SPLIT, LK_TIME_SPLIT)
    assert_within_bound(yp, ys, f64_truth(par, xin), f"{V} voices x {T} frames, nine modes")
    assert not np.array_equal(yp, ys)   # it IS a different arithmetic


@pytest.mark.parametrize("T", [64, 128, 192])
@pytest.mark.parametrize("V", [64, 65, 100])
def test_geometry(gpu, V, T):
    """one block (the pipeline fills and drains within the three extra rounds), ragged and whole voice groups"""
    p = W.fm_svf_params(V, SR)
    par, ser, x = fm_bank(p, SVF_PARALLEL), fm_bank(p, SVF_SERIAL), filter_input_bank(p)
    yp, ys, xin = render(par, T), render(ser, T), render(x, T)
    assert par.get_option("last_kernel") == LK_TIME_SPLIT_SVF
    truth = f64_truth(par, xin)
    assert_within_bound(yp, ys, truth, f"{V} voices x {T} frames", bank_wide=False)
    # the oscillators' state is the serial kernel's, bit for bit (the filter's: the hand-over and launch-split tests below)
    for slot in (W.FM_SLOTS["mod_phase"], W.FM_SLOTS["car_phase"]):
        assert_bit_equal(par.get_slot(slot), ser.get_slot(slot), slot)


def config1_params(V):
    rng = np.random.default_rng(5)
    f = (55.0 * 2.0 ** (5.0 * rng.random(V))).astype(np.float32)
    fc = (100.0 * 2.0 ** (7.0 * rng.random(V))).astype(np.float32)
    q = (0.5 + 3.5 * rng.random(V)).astype(np.float32)
    return dict(f=f, fc=fc, q=q)


def config1_bank(gpu, p, svf_exec, mode, gain):
    """sine_hz(f) >> lowpass_hz(fc, q) with per-voice filter modes, tolerance mode"""
    V = len(p["f"])
    b = gpu.Bank("sine_hz_lowpass_hz", V)
    b.set_param("0.0:value[0]", p["f"])
    b.set_param("1:cutoff", p["fc"])
    b.set_param("1:q", p["q"])
    b.set_param("1:mode", mode.astype(np.float32))
    b.set_param("1:gain", gain)
    b.set_sample_rate(SR)
    b.set_seed(np.arange(V, dtype=np.uint64))
    b.set_option("math", MATH_FAST)
    b.set_option("svf_exec", svf_exec)
    return b


def test_config1_kind(gpu):
    """sine_hz(f) >> lowpass_hz(fc, q): the other kind that has the kernel"""
    V, T = 100, 192
    p = config1_params(V)
    bank = lambda svf_exec, mode, gain: config1_bank(gpu, p, svf_exec, mode, gain)
    modes = np.arange(V) % 9
    par, ser, x = bank(SVF_PARALLEL, modes, 2.0), bank(SVF_SERIAL, modes, 2.0), bank(SVF_SERIAL, np.full(V, BELL), 1.0)
    assert par.get_option("has_svf_parallel") == 1
    yp, ys, xin = render(par, T), render(ser, T), render(x, T)
    assert (par.get_option("last_kernel"), ser.get_option("last_kernel")) == (LK_TIME_SPLIT_SVF, LK_TIME_SPLIT)
    assert_within_bound(yp, ys, f64_truth(par, xin), f"config 1, {V} voices x {T} frames", bank_wide=False)


def test_launch_splits_change_no_bit(gpu):
    V = 100
    p = W.fm_svf_params(V, SR)
    one, parts = fm_bank(p, SVF_PARALLEL), fm_bank(p, SVF_PARALLEL)
    a = render(one, 320)
    b = np.concatenate([render(parts, n) for n in (64, 128, 128)], axis=1)
    assert (one.get_option("last_kernel"), parts.get_option("last_kernel")) == (LK_TIME_SPLIT_SVF, LK_TIME_SPLIT_SVF)
    assert_bit_equal(a, b, "320 frames == 64 + 128 + 128")
    for slot in ("1:ic1eq", "1:ic2eq"):
        assert_bit_equal(one.get_slot(slot), parts.get_slot(slot), slot)


def test_state_hand_over_to_the_serial_kernel(gpu):
    V = 100
    p = W.fm_svf_params(V, SR)
    mixed, ser, x = fm_bank(p, SVF_PARALLEL), fm_bank(p, SVF_SERIAL), filter_input_bank(p)
    first = render(mixed, 128)
    assert mixed.get_option("last_kernel") == LK_TIME_SPLIT_SVF
    mixed.set_option("svf_exec", SVF_SERIAL)
    second = render(mixed, 128)
    assert mixed.get_option("last_kernel") == LK_TIME_SPLIT
    ys, xin = render(ser, 256), render(x, 256)
    assert_within_bound(np.concatenate([first, second], axis=1), ys, f64_truth(mixed, xin), "128 frames parallel, then 128 serial", bank_wide=False)


def test_non_finite_input(gpu):
    """Non-finite samples made through a parameter: after a first launch (a state to carry) voice 7's carrier offset becomes inf, voice 70's
    NaN.  The carrier emits the sine of its phase BEFORE it advances it, so frame 128 is still finite and the filter's input is NaN from
    frame 129 on -- the second frame of the second launch's first chunk, with a carried state.  (Any other frame of a block, inf as
    well as NaN: tests/host/check_svf_par.hip (d).)"""
    V = 100
    p = W.fm_svf_params(V, SR)
    par, ser, x = fm_bank(p, SVF_PARALLEL), fm_bank(p, SVF_SERIAL), filter_input_bank(p)
    outs = []
    for b in (par, ser, x):
        first = render(b, 128)
        off = b.get_slot(W.FM_SLOTS["f_add"])
        off[7], off[70] = np.inf, np.nan
        b.set_param(W.FM_SLOTS["f_add"], off)
        with np.errstate(all="ignore"):
            outs.append(np.concatenate([first, render(b, 128)], axis=1))
    yp, ys, xin = outs
    assert par.get_option("last_kernel") == LK_TIME_SPLIT_SVF
    assert not np.isfinite(xin[7, 129:]).any() and not np.isfinite(xin[70, 129:]).any() and np.isfinite(xin[7, :129]).all()
    assert np.array_equal(np.isfinite(yp), np.isfinite(ys))
    assert not np.isfinite(yp[7, 129:]).any() and np.isfinite(yp[7, :129]).all() and np.isfinite(np.delete(yp, (7, 70), axis=0)).all()
    assert_within_bound(yp, ys, f64_truth(par, xin), "non-finite input in two voices", bank_wide=False)


def test_per_bank_option_follows_the_default(gpu):
    V = 64
    p = W.fm_svf_params(V, SR)
    b = fm_bank(p, SVF_SERIAL)
    L = gpu.lib()
    try:
        assert L.fdsp_set_option(b"svf_exec", SVF_PARALLEL) == 0
        assert b.get_option("svf_exec") == SVF_SERIAL           # the bank's own value wins
        render(b, 64)
        assert b.get_option("last_kernel") == LK_TIME_SPLIT
        b.set_option("svf_exec", -1)                            # follow the process-wide default
        assert b.get_option("svf_exec") == SVF_PARALLEL
        render(b, 64)
        assert b.get_option("last_kernel") == LK_TIME_SPLIT_SVF
        with pytest.raises(gpu.FdspError):
            b.set_option("svf_exec", 2)
        b.set_option("svf_exec", SVF_PARALLEL)
        assert b.clone().get_option("svf_exec") == SVF_PARALLEL   # a clone copies the bank's own value
        b.set_option("svf_exec", -1)
    finally:
        assert L.fdsp_set_option(b"svf_exec", SVF_SERIAL) == 0
    assert b.get_option("svf_exec") == SVF_SERIAL
    assert gpu.Bank("noise_biquad", 64).get_option("has_svf_parallel") == 0


FALLBACKS = ["exact", "ragged_T", "planar", "tick", "time_split_0", "two_groups_per_cu", "process_mix", "from_graph"]


@pytest.mark.parametrize("case", FALLBACKS)
def test_fallbacks_are_todays_launches(gpu, case):
    """Where the kernel does not apply "svf_exec" = 1 changes nothing: bit for bit the twin bank with "svf_exec" = 0, and not kernel 11."""
    import torch

    V, T = 192, 128
    if case == "ragged_T":
        T = 100
    if case == "two_groups_per_cu":
        V, T = 64 * (torch.cuda.get_device_properties(0).multi_processor_count + 1), 64
    p = W.fm_svf_params(V, SR)
    math = MATH_EXACT if case == "exact" else MATH_FAST

    def bank(svf_exec):
        if case == "from_graph":
            g = GR.sine_hz(p["f"]) * p["f"] * p["m"] + p["f"] >> GR.sine() >> GR.lowpass_hz(p["fc"], p["q"])
            b = gpu.Bank.from_graph(g, V, sample_rate=SR)
            b.set_seed(p["seed"])
            b.set_option("math", math)
            b.set_option("svf_exec", svf_exec)
            assert b.get_option("has_svf_parallel") == 0
        else:
            b = fm_bank(p, svf_exec, math=math, modes=np.zeros(V) if case == "exact" else None)
        if case == "time_split_0":
            b.set_option("time_split", 0)
        return b

    outs = []
    for svf_exec in (SVF_PARALLEL, SVF_SERIAL):
        b = bank(svf_exec)
        if case == "process_mix":
            out = b.process_mix(T, mix=MIX_SUM)
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        else:
            outs.append(run_bank(b, None, T, LAYOUT_PLANAR if case == "planar" else LAYOUT_VOICE_MINOR, MODE_TICK if case == "tick" else MODE_PROCESS)[:, 0, :])
        assert b.get_option("last_kernel") not in (0, LK_TIME_SPLIT_SVF), case
    assert_bit_equal(outs[0], outs[1], case)
    if case == "exact":   # ... and exact mode is the oracle's bits, as in test_gpu_math_fast.py
        want, _ = O.bank_render(3, [p["f"], p["m"], p["fc"], p["q"]], p["seed"], T, SR, True, 0, 8)
        assert_bit_equal(outs[0], want, "exact mode under svf_exec = 1")
