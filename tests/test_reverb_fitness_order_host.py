"""Host checks (no GPU) of fitness_device_order (tests/reverb_fitness_ref.py), the restatement of the order fundsp_amd/csrc/fd_fitness.hpp states
for the device's reverb_fitness -- the function tests/test_gpu_reverb_fitness_bits.py holds the device to bit for bit:

  * a 64-sample case against a scalar transliteration of the header, in plain loops, bit for bit;
  * on every crafted response (tests/reverb_fitness_cases.py) against fitness_f64, with the yardstick of tests/test_gpu_reverb_fitness.py
    measured on that very response;
  * the crafted responses discriminate: every single-fault variant of the order differs in bits on a case named here.
"""
import functools
import math

import numpy as np
import pytest

import convolve_ref
import oracle as O
import resynth_ref
import reverb_fitness_cases as K
import reverb_fitness_ref as R

f32 = np.float32
FLOOR = 16.0 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def tabs(n=K.N):
    hann, tw = resynth_ref.tables(n, O.lib().o_math_cosf)
    hann.setflags(write=False)
    tw.setflags(write=False)
    return hann, tw


def bits(fit, terms):
    return np.concatenate([np.asarray(terms, dtype=np.float32), [np.float32(fit)]]).view(np.uint32)


# ---- the header in plain loops ----------------------------------------------------------------------------------------------------------
def scalar_device_order(response, hann, tw, lanes, window):
    """fd_fitness.hpp / k_fit_terms one scalar f32 operation at a time: lanes, bit-reversed packing, radix-2 stages, the split, the norms,
    the means afresh, the fold trees"""
    n = response.shape[1]
    nh, logn = n // 2, n.bit_length() - 1
    one, thr = f32(1.0), f32(1.0e-9)

    def bitrev(x, nbits):
        return int(format(x, f"0{nbits}b")[::-1], 2)

    def fold(red):
        red = list(red)
        s = lanes // 2
        while s >= 1:
            for t in range(s):
                red[t] = red[t] + red[t + s]
            s //= 2
        return red[0]

    def norm(re, im):
        a, b = float(re), float(im)
        return f32(math.sqrt(a * a + b * b))

    def rfft_bin(buf, b):
        (ar, ai), (br, bi) = buf[b], buf[nh - b]
        bi = -bi
        er, ei = f32(0.5) * (ar + br), f32(0.5) * (ai + bi)
        dr, di = f32(0.5) * (ar - br), f32(0.5) * (ai - bi)
        wx, wy = tw[b]
        qr, qi = di, -dr
        return er + (wx * qr - wy * qi), ei + (wx * qi + wy * qr)

    terms = []
    for c in range(2):
        x = response[c]
        buf = [None] * nh
        lane = []
        for t in range(lanes):
            echo = f32(0.0)
            for m in range(t, nh, lanes):
                i0, i1 = 2 * m, 2 * m + 1
                if i0 >= 1 and abs(x[i0]) >= thr:
                    echo = echo + one / f32(i0)
                if abs(x[i1]) >= thr:
                    echo = echo + one / f32(i1)
                buf[bitrev(m, logn - 1)] = (x[i0] * hann[i0], x[i1] * hann[i1])
            lane.append(echo)
        terms.append(fold(lane))
        for ls in range(1, logn):
            half, tstep = 1 << (ls - 1), logn - ls
            for j in range(nh // 2):
                k = j & (half - 1)
                i = ((j >> (ls - 1)) << ls) + k
                wx, wy = tw[k << tstep]
                (pr, pi), (qr, qi) = buf[i], buf[i + half]
                yr, yi = wx * qr - wy * qi, wx * qi + wy * qr
                buf[i + half] = (pr - yr, pi - yi)
                buf[i] = (pr + yr, pi + yi)
        nrm = [None] * nh
        nrm[0] = norm(buf[0][0] + buf[0][1], buf[0][0] - buf[0][1])
        for u in range(1, nh):
            nrm[u] = norm(*rfft_bin(buf, u))
        lane = []
        for t in range(lanes):
            pen = f32(0.0)
            for k in range(window + 1 + t, nh, lanes):
                s = f32(0.0)
                for j in range(k - window, k):
                    s = s + nrm[j]
                mean = s / f32(window)
                if nrm[k] > mean:
                    d = nrm[k] - mean
                    pen = pen + d * d
            lane.append(pen)
        terms.append(fold(lane) * f32(0.1))
    assert all(type(t) is np.float32 for t in terms)
    return ((terms[0] - terms[1]) + terms[2]) - terms[3], np.array(terms, dtype=np.float32)


def test_the_vectorised_restatement_equals_the_header_in_plain_loops():
    n, lanes, window = 64, 4, 5
    hann, tw = tabs(n)
    rng = np.random.default_rng(64)
    for trial in range(4):
        r = (rng.standard_normal((2, n)) * np.exp(-np.arange(n) / 20.0)).astype(np.float32)
        r[0, [0, 3, 10, 11, 40]] = [0.5, 0.0, 5.0e-10, -2.0e-9, -9.9e-10]      # around the threshold, and a zero
        r[1, :trial] = 0.0                                                     # channel 1's head: frames 0 .. trial - 1 silent
        r[1, n - 1] = f32(1.0e-9)                                              # the last frame, exactly on the threshold: it counts
        fv, tv = R.fitness_device_order(r, hann, tw, lanes=lanes, window=window)
        fs, ts = scalar_device_order(r, hann, tw, lanes, window)
        assert fv.dtype == np.float32 and tv.dtype == np.float32 and tv.shape == (4,)
        assert np.array_equal(bits(fv, tv), bits(fs, ts)), (trial, fv, tv, fs, ts)
        f64, t64 = R.fitness_f64(r, window=window)
        assert np.all(np.abs(tv - t64) <= 1e-5 * np.abs(t64)), (tv, t64)       # (and it is the score, not just self-consistent)
        assert n - 1 in R.echo_weights(r[1]) and 10 not in R.echo_weights(r[0]) and 11 in R.echo_weights(r[0])


# ---- the crafted responses ----------------------------------------------------------------------------------------------------------------
def test_the_cases_meet_their_conditions_as_taps_and_through_the_convolver():
    """as given, and as a convolver bank renders them from the impulse (convolve_ref: the bank's bits, tests/test_gpu_convolve.py) -- the
    response the device test scores.  `sparse` needs the convolver's rounding residue below 1e-9 off its taps."""
    c = K.cases()
    assert tuple(c) == K.NAMES and set(K.REASONS) == set(K.NAMES)
    x = np.zeros((5, 2, K.N), dtype=np.float32)
    x[:, :, 0] = 1.0
    y = convolve_ref.render(x, K.taps())
    for v, name in enumerate(K.NAMES):
        for which, r in (("taps", c[name]), ("rendered", y[v])):
            counts = [len(R.echo_weights(r[ch])) for ch in range(2)]
            print(f"{name} ({which}): samples that count {counts} of {K.N - 1}; largest deviation from the taps {np.abs(r - c[name]).max():.3e}")
            K.check_conditions(name, r)
    off = np.ones(K.N, dtype=bool)
    off[[0, 1, 2, 77, K.N - 1]] = False
    assert np.abs(y[1][0][off]).max() < 1.0e-9 and np.abs(y[1][1][1:]).max() < 1.0e-9


@functools.lru_cache(maxsize=None)
def scored(name):
    """(device order, f64, f32 serial) of a case, each (fitness, terms)"""
    r = on_threshold() if name == "on_threshold" else K.cases()[name]
    hann, tw = tabs()
    return R.fitness_device_order(r, hann, tw), R.fitness_f64(r), R.fitness_f32_serial(r)


@pytest.mark.parametrize("name", K.NAMES)
def test_restatement_within_the_yardstick_of_the_high_precision_reference(name):
    """delta = the relative deviation of fitness_f32_serial (the reference's own f32 order) from fitness_f64 on this response, per term and
    for the total, floored at 16 * 2^-24; the restatement may deviate by 4 * delta; a term that is exactly zero in f64 is exactly zero.

    `sparse` channel 0's penalty is rounding noise in ANY f32 evaluation: five taps give a flat spectrum, every norm sits within rounding of
    its mean, and the penalty (1e-22) is the sum of squared rounding errors -- its delta is of order 1 and says so; the term is pinned by
    bits on the device, not by this bound."""
    (fd, td), (f64, t64), (fs, ts) = scored(name)
    for q in range(4):
        if t64[q] == 0.0:
            assert td[q].view(np.uint32) == 0 and ts[q] == 0.0, (name, q, td[q])
            print(f"{name} term {q}: exactly +0.0")
            continue
        delta = max(FLOOR, abs(float(ts[q]) - t64[q]) / abs(t64[q]))
        dev = abs(float(td[q]) - t64[q]) / abs(t64[q])
        print(f"{name} term {q}: f64 {t64[q]:.9e} device order {td[q]:.9e} rel dev {dev:.3e} | serial delta {delta:.3e}")
        assert dev <= 4.0 * delta, (name, q, dev, delta)
    assert f64 != 0.0
    delta = max(FLOOR, abs(float(fs) - f64) / abs(f64))
    dev = abs(float(fd) - f64) / abs(f64)
    print(f"{name} total: f64 {f64:.9e} device order {fd:.9e} rel dev {dev:.3e} | serial delta {delta:.3e}")
    assert dev <= 4.0 * delta, (name, dev, delta)
    if name == "tones":                                              # the case with cancellation in the combine
        assert td[1] > 0 and td[3] > 0 and abs(float(fd)) > 1000.0 * float(td[0] + td[2])
    if name == "zero_left":
        assert not td[:2].view(np.uint32).any() and not t64[:2].any()


# ---- the cases discriminate ---------------------------------------------------------------------------------------------------------------
def on_threshold():
    """host only (a convolver cannot place it): `threshold` with samples of exactly +-1e-9f, which count"""
    r = K.cases()["threshold"].copy()
    r[0, 5], r[1, 9] = f32(1.0e-9), -f32(1.0e-9)
    return r


# variant -> (the option of reverb_fitness_ref._device_order, the cases that must catch it)
MUTANTS = {
    "the penalty starts at bin 52": (dict(pen_first=52), ("natural", "threshold", "tones")),
    "the penalty stops at bin N/2 - 2": (dict(pen_stop=K.N // 2 - 1), ("tones",)),
    "the echo starts at i = 0": (dict(echo_first=0), ("threshold", "sparse", "tones")),
    "the echo starts at i = 2": (dict(echo_first=2), ("sparse", "tones")),
    "a window of 49 bins": (dict(mean_bins=49), ("tones", "natural")),
    "the window shifted by one (k - 49 .. k)": (dict(mean_shift=1), ("tones", "natural")),
    "the Hann index off by one": (dict(hann_shift=1), ("tones", "natural", "zero_left")),
    "0.1f applied per term, not per sum": (dict(weight_per_term=True), ("tones",)),
    "the threshold compared with >": (dict(strict_threshold=True), ("on_threshold",)),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_single_fault_differs_in_bits_on_a_named_case(mutant):
    kw, catching = MUTANTS[mutant]
    hann, tw = tabs()
    for name in K.NAMES + ("on_threshold",):
        r = on_threshold() if name == "on_threshold" else K.cases()[name]
        true = bits(*scored(name)[0])
        got = bits(*R._device_order(r, hann, tw, **kw))
        differs = not np.array_equal(true, got)
        print(f"{mutant} on {name}: {'differs in ' + str(np.flatnonzero(true != got)) + ' (echo_0 pen_0 echo_1 pen_1 total)' if differs else 'the same bits'}")
        if name in catching:
            assert differs, (mutant, name)


def test_what_a_silent_head_and_an_empty_top_cannot_see():
    """why the cases exist: a response silent at its head (and `zero_left`, whose channel 0 is silent throughout) gives the same bits whether
    the echo loop starts at 0, 1 or 2, and none of the natural responses holds a sample exactly on the threshold"""
    hann, tw = tabs()
    for name in ("natural", "zero_left"):
        r = K.cases()[name]
        assert not r[:, :3].any()
        for kw in (dict(echo_first=0), dict(echo_first=2), dict(strict_threshold=True)):
            assert np.array_equal(bits(*scored(name)[0]), bits(*R._device_order(r, hann, tw, **kw))), (name, kw)
