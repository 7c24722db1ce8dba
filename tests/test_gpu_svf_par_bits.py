"""k_render_ts3p (fd_tsp.hpp; "svf_exec" = FDSP_SVF_PARALLEL, tolerance mode) held to the ORDER of fd_svf_par.hpp bit for bit: every
comparison here is an equality of bits against tests/svf_par_ref.py, the numpy restatement that tests/test_svf_par_ref.py shows to be
the header.  (tests/test_gpu_svf_par.py holds the same kernel to an accuracy bound; single faults of the order pass that bound.)

The filter's INPUT comes from a twin bank whose every filter is a bell of gain 1 (m0 = 1, m1 = m2 = 0), rendered by the serial kernel
from a zero filter state: 1 * v0 + 0 * v1 + 0 * v2 is v0 while the state is finite and v0 is no zero (-0.0 would come out as +0.0);
both conditions are asserted wherever the twin is used.  The coefficients are read back from the bank under test.  NaN compares equal
to NaN: which frames are NaN and which inf is compared, NaN payloads are not."""
import functools

import numpy as np
import pytest

import fundsp_amd
import svf_par_ref as S
from fundsp_amd import LAYOUT_VOICE_MINOR, MODE_PROCESS, SVF_PARALLEL, SVF_SERIAL
from fundsp_amd import workloads as W
from test_gpu_parity import assert_bit_equal, run_bank
from test_gpu_svf_par import BELL, LK_TIME_SPLIT, LK_TIME_SPLIT_SVF, SR, config1_bank, config1_params, filter_input_bank, fm_bank

pytestmark = pytest.mark.gpu
F = np.float32
KINDS = ["fm_svf", "sine_hz_lowpass_hz"]
IC = ("1:ic1eq", "1:ic2eq")


def params(kind, V):
    return W.fm_svf_params(V, SR) if kind == "fm_svf" else config1_params(V)


def make(kind, p, svf_exec, modes=None):
    """the bank under test: all nine modes spread over the voices (or `modes`), gain 2"""
    V = len(p["f"])
    modes = np.arange(V) % 9 if modes is None else modes
    return fm_bank(p, svf_exec, modes=modes) if kind == "fm_svf" else config1_bank(fundsp_amd, p, svf_exec, modes, 2.0)


def make_twin(kind, p):
    V = len(p["f"])
    return filter_input_bank(p) if kind == "fm_svf" else config1_bank(fundsp_amd, p, SVF_SERIAL, np.full(V, BELL), 1.0)


def render(b, T, kernel):
    with np.errstate(all="ignore"):
        y = run_bank(b, None, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)[:, 0, :]
    assert b.get_option("last_kernel") == kernel, (b.get_option("last_kernel"), kernel)   # a silent fall-back would compare a kernel with itself
    return y


def render_twin(x, T):
    """the filter's input: T more frames of the twin, with the two conditions that make its output the input"""
    assert np.all(x.get_slot("1:m0") == 1.0) and not x.get_slot("1:m1").any() and not x.get_slot("1:m2").any()
    xin = render(x, T, LK_TIME_SPLIT)
    assert not (xin == 0).any(), "a zero in the filter's input: the twin cannot tell -0.0 from +0.0"
    return xin


def coefs(b):
    return tuple(b.get_slot("1:" + n) for n in S.COEF_NAMES)


def state(b):
    return tuple(b.get_slot(n) for n in IC)


def set_filter_state(b, s1, s2):
    """through set_state, as preset() of tests/test_gpu_guard_bounds.py"""
    names = [n for n, _ in b.slots()]
    st = b.get_state()
    st[names.index(IC[0])], st[names.index(IC[1])] = s1, s2
    b.set_state(st)


def phases(b):
    names = [n for n, _ in b.slots() if n.endswith(":phase")]
    assert names
    return [b.get_slot(n) for n in names]


def assert_launch(got, end, ref, what):
    """frames and both state slots against (y, s1, s2) of the restatement"""
    assert_bit_equal(got, ref[0], what + ": frames")
    assert_bit_equal(end[0], ref[1], what + ": ic1eq")
    assert_bit_equal(end[1], ref[2], what + ": ic2eq")


@functools.lru_cache(maxsize=None)
def case(kind, V, T):
    """one launch of T frames of the parallel bank, the serial bank and the twin, and both restatements over the twin's frames"""
    p = params(kind, V)
    par, ser, x = make(kind, p, SVF_PARALLEL), make(kind, p, SVF_SERIAL), make_twin(kind, p)
    assert par.get_option("has_svf_parallel") == 1
    yp, ys, xin = render(par, T, LK_TIME_SPLIT_SVF), render(ser, T, LK_TIME_SPLIT), render_twin(x, T)
    co = coefs(par)
    for a, b in zip(co, coefs(ser)):
        assert_bit_equal(a, b, "both banks hold the same coefficients")
    zero = np.zeros(V, F)
    out = dict(yp=yp, ys=ys, xin=xin, co=co, par_state=state(par), ser_state=state(ser), par_phases=phases(par), ser_phases=phases(ser),
               launch=S.launch(co, zero, zero, xin), serial=S.serial(co, zero, zero, xin))
    for a in (yp, ys, xin):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("V", [65, 192])
@pytest.mark.parametrize("kind", KINDS)
def test_anchor_the_serial_kernel_is_the_serial_restatement(gpu, kind, V):
    """the serial tolerance-mode bank over the twin's frames: proves the extraction of xin and the hand-over reference at once"""
    c = case(kind, V, 448)
    assert np.isfinite(c["xin"]).all() and c["xin"].max() > 0.5
    assert_launch(c["ys"], c["ser_state"], c["serial"], f"{kind}, serial kernel, {V} voices")


@pytest.mark.parametrize("T", [64, 128, 192, 448])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 100, 192])
@pytest.mark.parametrize("kind", KINDS)
def test_matrix(gpu, kind, V, T):
    """ragged and whole voice groups, one to three of them; one block (the pipeline fills and drains inside the three extra rounds), then
    even and odd block counts on the double-buffered tiles"""
    c = case(kind, V, T)
    assert_launch(c["yp"], c["par_state"], c["launch"], f"{kind}, {V} voices x {T} frames")
    for a, b in zip(c["par_phases"], c["ser_phases"]):
        assert_bit_equal(a, b, "oscillator phase")


def test_largest_bank_that_takes_the_kernel(gpu):
    import torch

    V = 64 * torch.cuda.get_device_properties(0).multi_processor_count
    c = case("fm_svf", V, 64)
    assert_launch(c["yp"], c["par_state"], c["launch"], f"{V} voices x 64 frames")


def test_carried_states(gpu):
    """svf_par_ref.STATE_ROWS -- zero, a plain pair, -0.0, subnormal (this translation unit is IEEE), 2^96, 2^127, inf, NaN -- written over
    the voices before the first launch, every row under every mode.  Bits, including which frames are inf and which NaN, and the end
    state; NaN payloads are not compared."""
    V, T = 192, 128
    p = params("fm_svf", V)
    par, x = make("fm_svf", p, SVF_PARALLEL), make_twin("fm_svf", p)
    s1, s2 = S.state_rows(V)
    set_filter_state(par, s1, s2)
    assert_bit_equal(np.stack(state(par)), np.stack([s1, s2]), "set_state took the rows")
    yp, xin = render(par, T, LK_TIME_SPLIT_SVF), render_twin(x, T)
    ref = S.launch(coefs(par), s1, s2, xin)
    assert np.isnan(ref[0]).any() and np.isfinite(ref[0]).all(axis=1).sum() >= V // 4   # the rows reach both ends
    assert_launch(yp, state(par), ref, "carried edge states")


def run_sequence(kind, V, cuts, change=None, twin_change=None):
    """consecutive launches of `cuts` frames of one parallel bank, `change(bank, launch index)` before each; the restatement chained
    over the same cuts with the coefficients read back before each launch"""
    p = params(kind, V)
    par, x = make(kind, p, SVF_PARALLEL), make_twin(kind, p)
    s1 = s2 = np.zeros(V, F)
    got, want, cos = [], [], []
    for i, n in enumerate(cuts):
        if change is not None:
            change(par, i)
        if twin_change is not None:
            twin_change(x, i)
        co = coefs(par)
        got.append(render(par, n, LK_TIME_SPLIT_SVF))
        y, s1, s2 = S.launch(co, s1, s2, render_twin(x, n))
        want.append(y)
        cos.append(co)
        assert_launch(got[-1], state(par), (y, s1, s2), f"{kind}: launch {i} of {cuts}")
    return np.concatenate(got, axis=1), np.concatenate(want, axis=1), cos


@pytest.mark.parametrize("kind", KINDS)
def test_launch_splits(gpu, kind):
    V = 100
    one, ref_one, _ = run_sequence(kind, V, (320,))
    parts, ref_parts, _ = run_sequence(kind, V, (64, 128, 128))
    assert_bit_equal(one, ref_one, "320 frames")
    assert_bit_equal(parts, ref_parts, "64 + 128 + 128 frames")
    assert_bit_equal(one, parts, "320 == 64 + 128 + 128")


def changed(cos):
    return [int((S.bits(a) != S.bits(b)).sum()) for a, b in zip(cos[0], cos[1])]


def test_set_param_between_launches(gpu):
    """cutoff and q of every other voice: the tables follow with no hook (no host-side cache)"""
    V = 100

    def change(b, i):
        if i == 1:
            fc, q = b.get_slot(W.FM_SLOTS["cutoff"]), b.get_slot(W.FM_SLOTS["q"])
            fc[::2] *= F(0.5)
            q[::2] += F(2.5)
            b.set_param(W.FM_SLOTS["cutoff"], fc)
            b.set_param(W.FM_SLOTS["q"], q)

    got, want, cos = run_sequence("fm_svf", V, (128, 128), change)
    assert min(changed(cos)[:3]) > V // 4 and np.array_equal(cos[0][0][1::2], cos[1][0][1::2])   # a1 a2 a3 of the even voices move
    assert_bit_equal(got, want, "set_param between two launches")


def test_set_sample_rate_between_launches(gpu):
    V = 100
    change = lambda b, i: b.set_sample_rate(44100.0) if i == 1 else None
    got, want, cos = run_sequence("fm_svf", V, (128, 128), change, twin_change=change)
    assert min(changed(cos)[:3]) > V // 2
    assert_bit_equal(got, want, "set_sample_rate(44100) between two launches")


def test_mode_change_between_launches(gpu):
    V = 100
    change = lambda b, i: b.set_param(W.FM_SLOTS["mode"], ((np.arange(V) + 4) % 9).astype(F)) if i == 1 else None
    got, want, cos = run_sequence("fm_svf", V, (128, 128), change)
    assert max(changed(cos)[3:]) > V // 2   # the change reaches the mix coefficients of most voices
    assert_bit_equal(got, want, "a change of mode between two launches")


def test_hand_over_parallel_serial_parallel(gpu):
    """one bank through "svf_exec": 384 frames are launch / serial / launch of the restatement chained through the state"""
    V = 100
    p = params("fm_svf", V)
    b, x = make("fm_svf", p, SVF_PARALLEL), make_twin("fm_svf", p)
    s1 = s2 = np.zeros(V, F)
    for i, (svf_exec, kernel, fn) in enumerate([(SVF_PARALLEL, LK_TIME_SPLIT_SVF, S.launch), (SVF_SERIAL, LK_TIME_SPLIT, S.serial),
                                                (SVF_PARALLEL, LK_TIME_SPLIT_SVF, S.launch)]):
        b.set_option("svf_exec", svf_exec)
        got = render(b, 128, kernel)
        y, s1, s2 = fn(coefs(b), s1, s2, render_twin(x, 128))
        assert_launch(got, state(b), (y, s1, s2), f"hand-over, launch {i}")


def test_clone_continues_with_the_parents_bits(gpu):
    V = 100
    p = params("fm_svf", V)
    b, x = make("fm_svf", p, SVF_PARALLEL), make_twin("fm_svf", p)
    zero = np.zeros(V, F)
    first = S.launch(coefs(b), zero, zero, render_twin(x, 128))
    assert_launch(render(b, 128, LK_TIME_SPLIT_SVF), state(b), first, "before the clone")
    c = b.clone()
    ref = S.launch(coefs(b), first[1], first[2], render_twin(x, 128))
    yb, yc = render(b, 128, LK_TIME_SPLIT_SVF), render(c, 128, LK_TIME_SPLIT_SVF)
    assert_launch(yb, state(b), ref, "the parent after the clone")
    assert_launch(yc, state(c), ref, "the clone")


def test_non_finite_input(gpu):
    """The construction of test_gpu_svf_par.py::test_non_finite_input (after a first launch voice 7's carrier offset becomes inf, voice
    70's NaN: the filter's input is non-finite from frame 129 on, with a carried state), to the bit: every finite frame, and the position
    of every non-finite one.  (At a non-finite input frame the twin can only say NaN, so inf is not told from NaN there.)"""
    V = 100
    p = params("fm_svf", V)
    par, x = make("fm_svf", p, SVF_PARALLEL), make_twin("fm_svf", p)
    zero = np.zeros(V, F)
    first = S.launch(coefs(par), zero, zero, render_twin(x, 128))
    assert_launch(render(par, 128, LK_TIME_SPLIT_SVF), state(par), first, "first launch")
    for b in (par, x):
        off = b.get_slot(W.FM_SLOTS["f_add"])
        off[7], off[70] = np.inf, np.nan
        b.set_param(W.FM_SLOTS["f_add"], off)
    yp, xin = render(par, 128, LK_TIME_SPLIT_SVF), render_twin(x, 128)
    bad = ~np.isfinite(xin)
    assert bad[7, 1:].all() and bad[70, 1:].all() and not bad[:, 0].any() and not np.delete(bad, (7, 70), axis=0).any()
    ref = S.launch(coefs(par), first[1], first[2], xin)
    assert np.array_equal(np.isfinite(yp), np.isfinite(ref[0])) and np.array_equal(np.isfinite(yp), ~bad)
    fin = np.isfinite(ref[0])
    assert_bit_equal(np.where(fin, yp, F(0)), np.where(fin, ref[0], F(0)), "every finite frame")
    for got, want in zip(state(par), ref[1:]):
        assert np.array_equal(np.isfinite(got), np.isfinite(want))
        assert_bit_equal(np.where(np.isfinite(want), got, F(0)), np.where(np.isfinite(want), want, F(0)), "end state of the finite voices")


def test_long_run_and_the_cases_mean_something(gpu):
    """192 voices x 4 096 frames, nine modes, bits.  And the comparison is no tautology: on the same input the two restatements --
    chunked and serial -- differ in at least one sample of at least half the voices (on the CPU with noise: every one of 288 voices
    within 512 frames), so a kernel that ran the serial tick would be noticed."""
    V, T = 192, 4096
    c = case("fm_svf", V, T)
    assert_launch(c["yp"], c["par_state"], c["launch"], f"{V} voices x {T} frames")
    assert_launch(c["ys"], c["ser_state"], c["serial"], f"{V} voices x {T} frames, serial kernel")
    finite = np.isfinite(c["launch"][0]).all(axis=1) & np.isfinite(c["serial"][0]).all(axis=1)
    differ = (S.bits(c["launch"][0]) != S.bits(c["serial"][0])).any(axis=1)
    print(f"\nchunked and serial restatements differ in {differ[finite].sum()} of {finite.sum()} finite voices")
    assert finite.sum() >= V // 2 and 2 * differ[finite].sum() >= finite.sum()
