"""reverb_fitness (reference src/reverb.rs:31-139) restated twice on the host, for a rendered impulse response [2][N] (N = 32 768 in the
reference: `Impulse >> reverb` for 32768 / 44100 s at 44.1 kHz, :32-36).  TEST INFRASTRUCTURE ONLY.

Per channel c in {0, 1} (the stereo arm :67-73 is unreachable in `0..=1`):
    echo_c = sum_{i=1}^{N-1} (|r[i]| >= 1e-9 ? 1 / i : 0)                                             :45-53
    r[i]  *= 0.5 + 0.5 cos((i - N/2) 2 pi / N)                                                        :56-64
    S      = real_fft(r): N/2 bins, Nyquist packed into bin 0's imaginary part                        :75, fft.rs:6-29
    norm_k = |S_k|                                                                                    :103-108
    pen_c  = 0.1 sum_{k=W+1}^{N/2-1} max(0, norm_k - mean_k)^2, mean_k = (sum_{j=k-W}^{k-1} norm_j) / W,  W = 50    :98-115
fitness = echo_0 - pen_0 + echo_1 - pen_1.  Both functions return (fitness, [echo_0, pen_0, echo_1, pen_1]).

fitness_f64: numpy float64 throughout, np.fft.rfft, the means from a cumulative sum.
fitness_f32_serial: the reference's own order in f32 -- one serial `fitness +=` / `-=` chain over both channels, weights 1 / (i as f32), the
f32 window, the running `sum -= norm0; sum += norm1`, hypot norms -- with the spectrum taken from the f64 FFT of the f32 windowed samples and
rounded to f32 (microfft's own rounding is not restated).  Its terms are the same serial sums started from 0 each.
`window` is the reference's outlier_samples; the small hand-computed cases of the tests pass a shorter one.

fitness_device_order: the DEVICE's order (fundsp_amd/csrc/fd_fitness.hpp, "ORDER OF THE SUMS"), operation for operation in f32 -- the lanes'
partial sums, the fold tree, the windowed and packed row through resynth_ref.rfft (the project's radix-2 FFT), the norms through f64, every
mean summed afresh, the 0.1 once after the fold.  Every step is one f32 rounding, no FMA: the device's bits, not a tolerance."""
import numpy as np

import resynth_ref

THRESHOLD = np.float32(1.0e-9)
OUTLIER_WEIGHT = 0.1
OUTLIER_SAMPLES = 50


def hann_f64(n):
    i = np.arange(n, dtype=np.float64)
    return 0.5 + 0.5 * np.cos((i - (n >> 1)) * (2.0 * np.pi) / n)


def hann_f32(n):
    f = np.float32
    i = (np.arange(n, dtype=np.int64) - (n >> 1)).astype(np.float32)
    return f(0.5) + f(0.5) * np.cos(i * f(2.0 * np.pi) / f(n)).astype(np.float32)


def packed_spectrum(x):
    """real_fft's layout from np.fft.rfft (float64 in, complex128 out): N/2 bins, bin 0 = DC + i Nyquist"""
    s = np.fft.rfft(np.asarray(x, dtype=np.float64))
    out = s[:-1].copy()
    out[0] = complex(s[0].real, s[-1].real)
    return out


def echo_weights(r):
    """the indices i >= 1 that count: |r[i]| >= 1e-9, compared in f32 like the reference"""
    r = np.asarray(r, dtype=np.float32)
    return np.flatnonzero(np.abs(r[1:]) >= THRESHOLD) + 1


def penalty_f64(norm, window=OUTLIER_SAMPLES):
    norm = np.asarray(norm, dtype=np.float64)
    c = np.concatenate([[0.0], np.cumsum(norm)])          # c[k] = norm_0 + .. + norm_{k-1}
    k = np.arange(window + 1, len(norm))
    mean = (c[k] - c[k - window]) / window
    return OUTLIER_WEIGHT * float(np.sum(np.maximum(0.0, norm[k] - mean) ** 2))


def fitness_f64(response, window=OUTLIER_SAMPLES):
    r = np.asarray(response, dtype=np.float32)
    assert r.ndim == 2 and r.shape[0] == 2
    n = r.shape[1]
    terms = []
    for c in range(2):
        terms.append(float(np.sum(1.0 / echo_weights(r[c]).astype(np.float64))))
        norm = np.abs(packed_spectrum(r[c].astype(np.float64) * hann_f64(n)))
        terms.append(penalty_f64(norm, window))
    return terms[0] - terms[1] + terms[2] - terms[3], np.array(terms, dtype=np.float64)


def _serial_sum(x):
    """x[0] + x[1] + .. strictly in order, in f32 (np.cumsum accumulates sequentially); 0.0 for no terms"""
    x = np.asarray(x, dtype=np.float32)
    return np.float32(0.0) if x.size == 0 else np.cumsum(x, dtype=np.float32)[-1]


def penalty_terms_f32(norm, window=OUTLIER_SAMPLES):
    """the terms squared(norm1 - mean) * 0.1 of the reference's loop, in its order, with its running sum"""
    f = np.float32
    norm = np.asarray(norm, dtype=np.float32)
    nh = len(norm)
    if nh <= window + 1:
        return np.zeros(0, dtype=np.float32)
    moves = np.empty(2 * (nh - window - 1), dtype=np.float32)
    moves[0::2] = -norm[1:nh - window]                     # sum -= norm0 (i - window = 1 ..)
    moves[1::2] = norm[window + 1:nh]                      # sum += norm1
    run = np.cumsum(np.concatenate([norm[1:window + 1], moves]), dtype=np.float32)
    s = run[window - 1::2][:nh - window - 1]               # `sum` at the head of iteration i = window + 1 ..
    mean = s / f(window)
    n1 = norm[window + 1:]
    d = n1 - mean
    return np.where(n1 > mean, d * d * f(OUTLIER_WEIGHT), f(0.0)).astype(np.float32)


def fitness_f32_serial(response, window=OUTLIER_SAMPLES):
    f = np.float32
    r = np.asarray(response, dtype=np.float32)
    assert r.ndim == 2 and r.shape[0] == 2
    n = r.shape[1]
    chain, terms = [], []
    for c in range(2):
        w = f(1.0) / echo_weights(r[c]).astype(np.float32)
        spec = packed_spectrum((r[c] * hann_f32(n)).astype(np.float32)).astype(np.complex64)
        norm = np.hypot(spec.real, spec.imag).astype(np.float32)
        p = penalty_terms_f32(norm, window)
        chain += [w, -p]
        terms += [_serial_sum(w), _serial_sum(p)]
    return _serial_sum(np.concatenate(chain)), np.array(terms, dtype=np.float32)


def _lane_sums(terms, lanes):
    """lane t's sum of terms[t], terms[t + lanes], .. added in that order from 0.0; terms [count] or [count, parts] (the parts of one index
    are added in order before the next index).  A term that does not count is +0.0: x + 0.0 == x for the sums here, which never go below +0.0"""
    terms = np.asarray(terms, dtype=np.float32)
    if terms.ndim == 1:
        terms = terms[:, None]
    rounds = -(-terms.shape[0] // lanes)
    pad = np.zeros((rounds * lanes, terms.shape[1]), dtype=np.float32)
    pad[:terms.shape[0]] = terms
    pad = pad.reshape(rounds, lanes, terms.shape[1])
    acc = np.zeros(lanes, dtype=np.float32)
    for r in range(rounds):
        for p in range(terms.shape[1]):
            acc = acc + pad[r, :, p]
    return acc


def _fold(red):
    """red[t] += red[t + s], s = lanes/2 .. 1: red[0]"""
    red = np.array(red, dtype=np.float32)
    assert len(red) & (len(red) - 1) == 0, "the lanes are a power of two"
    s = len(red) // 2
    while s >= 1:
        red[:s] = red[:s] + red[s:2 * s]
        s //= 2
    return red[0]


def _device_order(response, hann, tw, lanes=1024, window=OUTLIER_SAMPLES, echo_first=1, strict_threshold=False, hann_shift=0, pen_first=None,
                  pen_stop=None, mean_bins=None, mean_shift=0, weight_per_term=False):
    """fitness_device_order and, through the options after `window`, single-fault variants of it for the tests that check that the crafted
    responses tell them apart (tests/test_reverb_fitness_order_host.py).  The defaults are the header's order."""
    f = np.float32
    r = np.asarray(response, dtype=np.float32)
    assert r.ndim == 2 and r.shape[0] == 2
    n = r.shape[1]
    nh = n // 2
    hann, tw = np.asarray(hann, dtype=np.float32), np.asarray(tw, dtype=np.float32).reshape(-1, 2)
    assert hann.shape == (n,) and tw.shape == (nh, 2) and nh > window + 1
    op = resynth_ref._Ops(False)
    i = np.arange(n)
    pen_first = window + 1 if pen_first is None else pen_first
    pen_stop = nh if pen_stop is None else pen_stop
    mean_bins = window if mean_bins is None else mean_bins
    terms = []
    for c in range(2):
        # echo_c: lane t over i = 2m, 2m + 1, m = t, t + lanes, ..
        counts = (np.abs(r[c]) > THRESHOLD) if strict_threshold else (np.abs(r[c]) >= THRESHOLD)
        counts &= i >= echo_first
        with np.errstate(divide="ignore"):
            w = np.where(counts, f(1.0) / i.astype(np.float32), f(0.0)).astype(np.float32)
        terms.append(_fold(_lane_sums(w.reshape(nh, 2), lanes)))
        # the windowed row, packed and transformed; the norms through f64
        xw = (r[c] * np.roll(hann, -hann_shift)).astype(np.float32)
        xr, xi = resynth_ref.rfft(xw, tw, op)
        re, im = xr[:nh].astype(np.float64), xi[:nh].astype(np.float64)
        im[0] = float(xr[nh])                                # bin 0 packs (DC, Nyquist)
        norm = np.sqrt(re * re + im * im).astype(np.float32)
        # mean_k afresh per bin, ascending j from 0.0
        k = np.arange(pen_first, pen_stop)
        s = np.zeros(len(k), dtype=np.float32)
        for j in range(mean_bins):
            s = s + norm[k - mean_bins + mean_shift + j]
        mean = s / f(mean_bins)
        n1 = norm[k]
        d = n1 - mean
        sq = np.where(n1 > mean, d * d, f(0.0)).astype(np.float32)
        if weight_per_term:
            terms.append(_fold(_lane_sums(sq * f(OUTLIER_WEIGHT), lanes)))
        else:
            terms.append(_fold(_lane_sums(sq, lanes)) * f(OUTLIER_WEIGHT))
    t = np.array(terms, dtype=np.float32)
    return ((t[0] - t[1]) + t[2]) - t[3], t


def fitness_device_order(response, hann, tw, lanes=1024, window=OUTLIER_SAMPLES):
    """(fitness, [echo_0, pen_0, echo_1, pen_1]) as f32, in the order fd_fitness.hpp states.  hann [N], tw [N/2, 2] = (cos, -sin): the tables
    of resynth_ref.tables(N, the oracle's cosf).  `lanes` (a power of two) and `window` are parameters for the small cases checked by hand."""
    return _device_order(response, hann, tw, lanes, window)
