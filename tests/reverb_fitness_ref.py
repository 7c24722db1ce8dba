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
`window` is the reference's outlier_samples; the small hand-computed cases of the tests pass a shorter one."""
import numpy as np

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
