"""The time-parallel FixedSvf stage (fundsp_amd/csrc/fd_svf_par.hpp, k_render_ts3p in fd_tsp.hpp) restated in numpy, in the header's
operation ORDER, so that a device launch can be held to it bit for bit.  No device and no compiler are needed here.

    tables   2 LC reference ticks in f64 on zero input from states (1, 0) and (0, 1); every entry rounded to f32 once
    chunks   per 64-frame block, K = 64 / LC passes of the f32 tick from state (0, 0): yz[n] and the end states z_c
    fix-up   y[n] = yz[n] + fma(r[n].x, s.x, r[n].y * s.y)
    carry    s.x' = fma(P00, s.x, P01 * s.y) + z_c.x   (.y: P10, P11, z_c.y)
Every operation is f32 but the table build, and nothing is contracted but the two explicit FMAs (fma32 below rounds once).

All arrays are per voice: `co` is the six coefficient arrays (a1, a2, a3, m0, m1, m2), [V] each; states are [V]; frames are x[V][T].
tests/test_svf_par_ref.py shows that this file IS the header (against a host build of it) and that each single fault of FAULTS changes
bits; tests/test_gpu_svf_par_bits.py holds the kernel to it."""
import numpy as np

F = np.float32
COEF_NAMES = ("a1", "a2", "a3", "m0", "m1", "m2")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def fma32(a, b, c):
    """round_f32(a * b + c), rounded ONCE, for f32 arrays.  The product of two f32 is exact in f64; the f64 sum is not, so its rounding
    error is taken with TwoSum and, where it is non-zero and the sum's last mantissa bit is even, the sum is moved one f64 ulp toward
    the error (round to odd: 53 bits are more than 24 + 2, so the one rounding to f32 that follows -- normal or subnormal -- sees on which
    side of every f32 tie the exact value lies).  Non-finite operands go through untouched."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=F), np.asarray(b, dtype=F), np.asarray(c, dtype=F))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        w = s.view(np.int64).copy()
        fix = np.isfinite(s) & (err != 0) & ((w & 1) == 0)   # (s == 0 with err != 0 cannot happen: a zero sum is exact)
        away = (err > 0) == (s > 0)                          # the error points away from zero: one more in sign-magnitude
        w = np.where(fix, np.where(away, w + 1, w - 1), w)
        return w.view(np.float64).astype(F)


def fma32_double_rounded(a, b, c):
    """What fma32 must NOT be: the sum rounded to f64, then to f32 (tests/test_svf_par_ref.py shows the fmaf test tells them apart)."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def tick(co, s1, s2, v0, two):
    """SvfCore::tick (svf.rs:995-1006): the reference's operations in the reference's order, all voices at once, at the precision of its
    operands (`two` is 2 in that precision).  Returns (y, ic1eq', ic2eq')."""
    a1, a2, a3, m0, m1, m2 = co
    v3 = v0 - s2
    v1 = a1 * s1 + a2 * v3
    v2 = s2 + a2 * s1 + a3 * v3
    return m0 * v0 + m1 * v1 + m2 * v2, two * v1 - s1, two * v2 - s2


def _coefs(co, dtype):
    return [np.asarray(c, dtype=F).astype(dtype) for c in co]


def _zero_input(co, n, s1, s2, two):
    """n ticks on zero input: the outputs [n][V] and the end state, unrounded"""
    r = []
    zero = np.zeros_like(s1)
    for _ in range(n):
        y, s1, s2 = tick(co, s1, s2, zero, two)
        r.append(y)
    return np.stack(r), s1, s2


def tables(co, LC, dtype=np.float64, extra=0):
    """svfp_tables<LC>: rx[LC][V], ry[LC][V], p00, p01, p10, p11 (f32).  `dtype` and `extra` exist for FAULTS only: the ticks in another
    precision, and `extra` more entries of r beyond the chunk (P stays A^LC)."""
    c = _coefs(co, dtype)
    V = len(c[0])
    one, zero, two = np.ones(V, dtype), np.zeros(V, dtype), dtype(2)
    with np.errstate(all="ignore"):
        rx, p00, p10 = _zero_input(c, LC, one, zero, two)
        ry, p01, p11 = _zero_input(c, LC, zero, one, two)
        if extra:
            rx = np.concatenate([rx, _zero_input(c, extra, p00, p10, two)[0]])
            ry = np.concatenate([ry, _zero_input(c, extra, p01, p11, two)[0]])
        return tuple(a.astype(F) for a in (rx, ry, p00, p01, p10, p11))


# Single faults of the order (launch(..., fault=name)): each is a kernel that still "works" -- most stay inside the tolerance bound of
# tests/test_gpu_svf_par.py (tests/test_svf_par_ref.py computes which) -- and none keeps the bits.
FAULTS = {
    "fix_unfused": "fix-up unfused: yz + (rx * s1 + ry * s2)",
    "fix_fma_other_product": "fix-up FMA on the other product: fma(ry, s2, rx * s1)",
    "carry_unfused": "carry unfused: (p00 * s1 + p01 * s2) + z",
    "carry_z_in_fma": "carry adds z inside the FMA: fma(p00, s1, z) + p01 * s2",
    "chunk0_from_state": "chunk 0 run from the carried state instead of zero + fix-up",
    "tables_f32": "tables from an f32 tick instead of f64",
    "carry_next_z": "carry applied with chunk c + 1's z (the last chunk's with chunk 0's)",
    "r_late": "r[n] taken at n + 1",
}


def launch(co, s1, s2, x, LC=32, fault=None):
    """One launch of k_render_ts3p over x[V][T] (T a multiple of 64) from the carried state (s1, s2): returns y[V][T], s1', s2'.
    The tables are rebuilt per call, as the kernel rebuilds them per launch.  `fault`: a key of FAULTS, or None for the stated order."""
    assert fault is None or fault in FAULTS, fault
    co = _coefs(co, F)
    x = np.asarray(x, dtype=F)
    V, T = x.shape
    K = 64 // LC
    assert K * LC == 64 and T % 64 == 0, (LC, T)
    rx, ry, p00, p01, p10, p11 = tables(co, LC, dtype=F if fault == "tables_f32" else np.float64, extra=1 if fault == "r_late" else 0)
    if fault == "r_late":
        rx, ry = rx[1:], ry[1:]
    rxT, ryT = np.ascontiguousarray(rx.T), np.ascontiguousarray(ry.T)   # [V][LC]
    s1, s2 = np.asarray(s1, dtype=F).copy(), np.asarray(s2, dtype=F).copy()
    y = np.empty((V, T), F)
    two = F(2)
    with np.errstate(all="ignore"):
        for t0 in range(0, T, 64):
            yz = np.empty((V, 64), F)
            z = []
            for c in range(K):   # chunk pass
                z1, z2 = np.zeros(V, F), np.zeros(V, F)
                if fault == "chunk0_from_state" and c == 0:
                    z1, z2 = s1, s2
                for n in range(c * LC, (c + 1) * LC):
                    yz[:, n], z1, z2 = tick(co, z1, z2, x[:, t0 + n], two)
                z.append((z1, z2))
            for c in range(K):   # fix-up, the state carried chunk to chunk
                cut = slice(t0 + c * LC, t0 + (c + 1) * LC)
                yzc = yz[:, c * LC:(c + 1) * LC]
                a, b = s1[:, None], s2[:, None]
                if fault == "chunk0_from_state" and c == 0:
                    y[:, cut] = yzc
                    s1, s2 = z[0]
                    continue
                if fault == "fix_unfused":
                    y[:, cut] = yzc + (rxT * a + ryT * b)
                elif fault == "fix_fma_other_product":
                    y[:, cut] = yzc + fma32(ryT, b, rxT * a)
                else:
                    y[:, cut] = yzc + fma32(rxT, a, ryT * b)
                z1, z2 = z[(c + 1) % K] if fault == "carry_next_z" else z[c]
                if fault == "carry_unfused":
                    n1, n2 = (p00 * s1 + p01 * s2) + z1, (p10 * s1 + p11 * s2) + z2
                elif fault == "carry_z_in_fma":
                    n1, n2 = fma32(p00, s1, z1) + p01 * s2, fma32(p10, s1, z2) + p11 * s2
                else:
                    n1, n2 = fma32(p00, s1, p01 * s2) + z1, fma32(p10, s1, p11 * s2) + z2
                s1, s2 = n1, n2
    return y, s1, s2


def serial(co, s1, s2, x, dtype=F):
    """The tick frame by frame from the carried state: what k_render_ts3 computes in tolerance mode (FastOf changes the sines, not
    FixedSvf).  dtype = np.float64 gives the truth the tolerance tests measure against."""
    co = _coefs(co, dtype)
    x = np.asarray(x, dtype=F)
    V, T = x.shape
    s1, s2 = np.asarray(s1, dtype=F).astype(dtype), np.asarray(s2, dtype=F).astype(dtype)
    y = np.empty((V, T), dtype)
    two = dtype(2)
    with np.errstate(all="ignore"):
        for t in range(T):
            y[:, t], s1, s2 = tick(co, s1, s2, x[:, t].astype(dtype), two)
    return y, s1, s2


def chain(fn, co, s1, s2, x, cuts, **kw):
    """`fn` (launch or serial) over consecutive launches of `cuts` frames, the state carried"""
    ys, t0 = [], 0
    for n in cuts:
        y, s1, s2 = fn(co, s1, s2, x[:, t0:t0 + n], **kw)
        ys.append(y)
        t0 += n
    assert t0 == x.shape[1]
    return np.concatenate(ys, axis=1), s1, s2


# carried filter states (ic1eq, ic2eq) for the edge tests: zero, a plain pair, -0.0, subnormal, large, the largest binade, inf, NaN
STATE_ROWS = [(0.0, 0.0), (0.25, -0.125), (-0.0, -0.0), (1e-40, -3e-41), (2.0 ** 96, -2.0 ** 96), (2.0 ** 127, 2.0 ** 127),
              (np.inf, 0.0), (0.0, np.nan)]


def state_rows(V):
    """(s1[V], s2[V]): STATE_ROWS spread over the voices so that every row meets every filter mode of a bank whose modes go v % 9"""
    rows = np.array([STATE_ROWS[(v // 9) % len(STATE_ROWS)] for v in range(V)], dtype=F)
    return rows[:, 0].copy(), rows[:, 1].copy()
