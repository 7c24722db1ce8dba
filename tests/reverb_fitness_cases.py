"""Responses [2][32 768] f32 made to separate the device's reverb_fitness (fundsp_amd/csrc/fd_fitness.hpp) from near misses of it, shared by
tests/test_reverb_fitness_order_host.py and tests/test_gpu_reverb_fitness_bits.py.  TEST INFRASTRUCTURE ONLY.

A natural reverb response is silent at its head and empty in its last bins: a score that counts the impulse sample, skips sample 1 or drops
the last bin gives the very same bits on it.  Each case here carries the reason it exists; the conditions it must meet are asserted by the
tests on the response that is actually scored (on the device: the taps through a convolver bank), not assumed of the taps."""
import numpy as np

from reverb_fitness_ref import echo_weights
from test_reverb_fitness_host import synthetic

N = 32768
NAMES = ("threshold", "sparse", "tones", "zero_left", "natural")
SPARSE_FRAMES = (1, 2, 77, N - 1)           # echo_weights of `sparse` channel 0 (frame 0 holds a tap too and must not count)
REASONS = {
    "threshold": "dense samples of magnitude 1e-9 / 4 .. 4e-9, both signs: the |r| >= 1e-9 test decides about half of them, from frame 0 on",
    "sparse": "taps at frames 0, 1, 2, 77 and N - 1 alone: the ends of the echo loop (frame 0 never counts, 1 and N - 1 do); channel 1 "
              "holds the impulse sample only and has no echo at all",
    "tones": "energy at bin 51 (the first scored) and 16383 (the last); channel 1 at bin 49.5, which only the first means read, and a strong "
             "tone mid-band: large penalties, a total that cancels against the echo terms",
    "zero_left": "channel 0 all zeros: its terms are +0.0 exactly, and channel 1's are untouched by it",
    "natural": "decaying noise behind a silent head (test_reverb_fitness_host.synthetic): what a search scores",
}

_CASES = {}


def cases():
    """{name: [2][N] f32}, seeded, computed once and left unchanged"""
    if _CASES:
        return _CASES
    rng = np.random.default_rng(20)
    i = np.arange(N, dtype=np.float64)
    out = {}
    mag = 1.0e-9 * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (2, N)))
    out["threshold"] = (mag * rng.choice([-1.0, 1.0], (2, N))).astype(np.float32)
    sp = np.zeros((2, N), dtype=np.float32)
    sp[0, [0, 1, 2, 77, N - 1]] = [1.0e-4, -7.0e-5, 5.0e-5, -3.0e-5, 2.0e-5]
    sp[1, 0] = 1.0e-4
    out["sparse"] = sp
    decay = np.exp(-i / 6000.0)
    noise = 1.0e-4 * rng.standard_normal((2, N))
    t0 = decay * (np.cos(2.0 * np.pi * 51.0 * i / N) + np.cos(2.0 * np.pi * 16383.0 * i / N))
    t1 = decay * (np.cos(2.0 * np.pi * 49.5 * i / N) + 0.5 * np.cos(2.0 * np.pi * 3000.37 * i / N))
    out["tones"] = (np.stack([t0, t1]) + noise).astype(np.float32)
    zl = synthetic(seed=21)
    zl[0] = 0.0
    out["zero_left"] = zl
    out["natural"] = synthetic()
    for r in out.values():
        assert r.shape == (2, N) and r.dtype == np.float32
        r.setflags(write=False)
    _CASES.update(out)
    return _CASES


def taps():
    """[5, 2, N]: the cases in the order of NAMES, the per-instance responses of a convolver bank"""
    c = cases()
    return np.stack([c[n] for n in NAMES])


def check_conditions(name, r):
    """the conditions of the case `name` on a response r [2][N] that is about to be scored"""
    if name == "threshold":
        for c in range(2):
            n = len(echo_weights(r[c]))
            assert 0.25 * (N - 1) <= n <= 0.75 * (N - 1), (name, c, n)
    elif name == "sparse":
        assert tuple(echo_weights(r[0])) == SPARSE_FRAMES and len(echo_weights(r[1])) == 0, (echo_weights(r[0]), echo_weights(r[1]))
        assert abs(r[0, 0]) >= 1.0e-9 and abs(r[1, 0]) >= 1.0e-9   # frame 0 would count if the loop reached it
    elif name == "zero_left":
        assert not np.abs(r[0]).any()
        assert len(echo_weights(r[1])) > 1000
