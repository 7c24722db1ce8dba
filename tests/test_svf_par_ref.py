"""tests/svf_par_ref.py IS fundsp_amd/csrc/fd_svf_par.hpp: the numpy restatement of the time-parallel SVF against a host build of the
header (tests/host/svf_par_dump.cpp, host compiler, -O2 -ffp-contract=off), every comparison on uint32 views.  No kernel is launched;
tests/test_gpu_svf_par_bits.py then holds k_render_ts3p to the restatement."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import svf_par_ref as S
from test_svf_par_host import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SR = 48000.0
T = 320
CUTS = (64, 128, 128)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("svf_par_dump") / "svf_par_dump"
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "fundsp_amd", "csrc"), "-o", str(exe),
           os.path.join(ROOT, "tests", "host", "svf_par_dump.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return str(exe)


def run_program(exe, mode, header, arrays, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        np.array(header, dtype=np.int32).tofile(f)
        for a in arrays:
            np.ascontiguousarray(a, dtype=F).tofile(f)
    r = subprocess.run([exe, mode, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(dst, dtype=F)


def header_block(exe, tmp_path, co, s1, s2, x, LC):
    """the header's launch: (y, s1', s2', (rx, ry, p00, p01, p10, p11))"""
    V, n = x.shape
    raw = run_program(exe, "block", [V, n, LC], [np.stack(co, axis=1), np.stack([s1, s2], axis=1), x], tmp_path)
    assert raw.size == V * (n + 2 + 2 * LC + 4)
    y, s, tb = raw[:V * n].reshape(V, n), raw[V * n:V * (n + 2)].reshape(V, 2), raw[V * (n + 2):].reshape(V, 2 * LC + 4)
    return y, s[:, 0], s[:, 1], (tb[:, :LC].T, tb[:, LC:2 * LC].T, tb[:, 2 * LC], tb[:, 2 * LC + 1], tb[:, 2 * LC + 2], tb[:, 2 * LC + 3])


def same_bits(got, want, what):
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = (S.bits(got) != S.bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not diff.any(), f"{what}: {diff.sum()} of {diff.size} differ, first at {tuple(np.argwhere(diff)[0])}"


@functools.lru_cache(maxsize=None)
def grid():
    """the 16 x 16 grid of tests/host/check_svf_par.hip (cutoff 20 Hz .. 0.45 sr, q 0.1 .. 50, gain 2) in all nine modes, coefficients from
    the project's own svf_coefs through the oracle: six [2304] arrays"""
    modes = sorted(O.SVF_MODES, key=O.SVF_MODES.get)
    assert len(modes) == 9
    rows = []
    for mode in modes:
        for v in range(256):
            fc = float(F(20.0 * (0.45 * SR / 20.0) ** ((v % 16) / 15.0)))
            q = float(F(0.1 * 500.0 ** ((v // 16) / 15.0)))
            rows.append(O.svf_coefs(mode, SR, fc, q, 2.0))
    co = np.stack(rows).astype(F)
    assert np.isfinite(co).all()
    return tuple(co[:, j].copy() for j in range(6))


@functools.lru_cache(maxsize=None)
def banks():
    """(co, s1, s2, x, first voice of the FM half): the grid twice -- noise at 0.5 rms per voice, then the FM sine of peak 3.5 -- from a
    non-zero carried state"""
    g = grid()
    n = len(g[0])
    rng = np.random.default_rng(3)
    noise = (0.5 * rng.standard_normal((n, T))).astype(F)
    i = np.arange(T)
    fm = (3.5 * np.sin(2 * np.pi * 220.0 * i / SR + 4.0 * np.sin(2 * np.pi * 330.0 * i / SR))).astype(F)
    x = np.concatenate([noise, np.broadcast_to(fm, (n, T))])
    co = tuple(np.concatenate([c, c]) for c in g)
    s1, s2 = ((0.25 * rng.standard_normal(2 * n)).astype(F) for _ in range(2))
    assert s1.all() and s2.all()
    for a in co + (s1, s2, x):
        a.setflags(write=False)
    return co, s1, s2, x, n


def crafted_triples():
    """Triples whose exact a * b + c lies next to an f32 tie by less than half an f64 ulp of the sum: rounding the sum to f64 first lands
    ON the tie and the second rounding goes to even, whichever side the exact value was on."""
    a, b, c = [], [], []
    # a * b exactly halfway between two f32 (i, j odd: 1 + (i + j) 2^-12 + i j 2^-24 ends in the 2^-24 bit), c = +-2^-60 of its size
    for i, j in ((1, 1), (3, 5), (101, 77), (1023, 511), (2047, 1), (5, 999)):
        for e in (-80, -20, 0, 13, 60):
            for sa in (1.0, -1.0):
                x, y = sa * (1.0 + i * 2.0 ** -12) * 2.0 ** e, 1.0 + j * 2.0 ** -12
                for sc in (1.0, -1.0):
                    a.append(x), b.append(y), c.append(sc * 2.0 ** (e - 60))   # (a power of two: |a b| itself is no f32)
    # the mirror: c carries the value, a * b is half an ulp of it and a sliver (2^-24 +- 2^-60 = (2^36 +- 1) 2^-60, both factor into f32)
    for e in (-90, -7, 0, 31, 90):
        for sg in (1.0, -1.0):
            a.append(sg * 1774001.0 * 2.0 ** (e - 30)), b.append(38737.0 * 2.0 ** -30), c.append(sg * 2.0 ** e)                       # just above the tie
            a.append(sg * 262143.0 * 2.0 ** (e - 30)), b.append(262145.0 * 2.0 ** -30), c.append(sg * (1.0 + 2.0 ** -23) * 2.0 ** e)   # just below it
            a.append(sg * 262143.0 * 2.0 ** (e - 30)), b.append(262145.0 * 2.0 ** -30), c.append(sg * 2.0 ** e)
            a.append(sg * 1774001.0 * 2.0 ** (e - 30)), b.append(38737.0 * 2.0 ** -30), c.append(sg * (1.0 + 2.0 ** -23) * 2.0 ** e)
    out = [np.array(v, dtype=np.float64) for v in (a, b, c)]
    for v in out:
        assert np.array_equal(v.astype(F).astype(np.float64), v)   # every operand IS an f32
    return [v.astype(F) for v in out]


def triples():
    rng = np.random.default_rng(17)
    n = 40000
    u = lambda: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(F)   # the whole exponent range, inf and NaN included
    sets = [(u(), u(), u())]
    with np.errstate(all="ignore"):
        a, b = u(), u()
        sets.append((a, b, (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rng.standard_normal(n) * 2.0 ** -20)).astype(F)))  # cancellation
        a, b = u(), u()
        sets.append((a, b, ((a.astype(np.float64) * b.astype(np.float64)) * np.exp2(rng.integers(-30, 31, n)) * rng.choice([-1.0, 1.0], n)).astype(F)))
        m = lambda k: (1.0 + rng.random(k)).astype(F)
        a, b = m(4000) * F(2.0 ** -70), m(4000) * F(2.0 ** -70) * rng.choice([-1.0, 1.0], 4000).astype(F)       # subnormal results
        sets.append((a, b, (rng.standard_normal(4000) * 2.0 ** -140).astype(F)))
        sets.append((a, b, np.zeros(4000, F)))
    sp = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1e-40, 3.4028235e38, np.inf, -np.inf, np.nan, 1.17549435e-38], dtype=F)   # +-0, inf, NaN, the edges
    g = np.meshgrid(sp, sp, sp, indexing="ij")
    sets.append(tuple(v.ravel() for v in g))
    sets.append(tuple(crafted_triples()))
    return [np.concatenate([s[k] for s in sets]) for k in range(3)]


def test_fma32_equals_fmaf(dump, tmp_path):
    a, b, c = triples()
    assert a.size >= 100000
    want = run_program(dump, "fma", [a.size], [a, b, c], tmp_path)
    with np.errstate(all="ignore"):
        assert np.isnan(want).sum() > 100 and np.isinf(want).sum() > 100 and ((want != 0) & (np.abs(want) < F(1.17549435e-38))).sum() > 1000
    same_bits(S.fma32(a, b, c), want, "fma32 against __builtin_fmaf")
    # ... and the test would notice the form that rounds twice, on the crafted triples and among the random ones
    ca, cb, cc = crafted_triples()
    twice = S.fma32_double_rounded(ca, cb, cc)
    once = S.fma32(ca, cb, cc)
    print(f"\n{a.size} triples; rounding twice changes {(S.bits(twice) != S.bits(once)).sum()} of {ca.size} crafted results")
    assert (S.bits(twice) != S.bits(once)).sum() >= ca.size // 2


@pytest.mark.parametrize("LC", [32, 16])
def test_restatement_is_the_header(dump, tmp_path, LC):
    """tables, all frames and the end state, 4 608 voices x 320 frames from a carried state; and the same frames as 64 + 128 + 128"""
    co, s1, s2, x, _ = banks()
    y, e1, e2, tb = header_block(dump, tmp_path, co, s1, s2, x, LC)
    for name, got, want in zip(("rx", "ry", "p00", "p01", "p10", "p11"), S.tables(co, LC), tb):
        same_bits(got, want, f"LC = {LC}: table {name}")
    ry, r1, r2 = S.launch(co, s1, s2, x, LC=LC)
    same_bits(ry, y, f"LC = {LC}: frames")
    same_bits(r1, e1, f"LC = {LC}: ic1eq")
    same_bits(r2, e2, f"LC = {LC}: ic2eq")
    assert np.isfinite(y).all() and np.abs(y).max() > 1.0
    # launch splits: the header run cut by cut, and the restatement chained over the same cuts
    parts, h1, h2, t0 = [], s1, s2, 0
    for n in CUTS:
        py, h1, h2, _ = header_block(dump, tmp_path, co, h1, h2, x[:, t0:t0 + n], LC)
        parts.append(py)
        t0 += n
    cy, c1, c2 = S.chain(S.launch, co, s1, s2, x, CUTS, LC=LC)
    same_bits(cy, np.concatenate(parts, axis=1), f"LC = {LC}: frames of 64 + 128 + 128")
    same_bits(cy, y, f"LC = {LC}: 64 + 128 + 128 == 320")
    same_bits(np.stack([c1, c2, h1, h2]), np.stack([e1, e2, e1, e2]), f"LC = {LC}: end state of 64 + 128 + 128")


@pytest.mark.parametrize("LC", [32, 16])
def test_edge_states_go_through_the_same_comparison(dump, tmp_path, LC):
    """the carried-state rows of tests/test_gpu_svf_par_bits.py (zero, -0.0, subnormal, 2^96, 2^127, inf, NaN) on every third grid voice:
    frames (which are inf, which NaN), end state"""
    co, _, _, x, _ = banks()
    pick = np.arange(0, len(co[0]), 3)
    co, x = tuple(c[pick] for c in co), x[pick, :128]
    s1, s2 = S.state_rows(len(pick))
    y, e1, e2, _ = header_block(dump, tmp_path, co, s1, s2, x, LC)
    ry, r1, r2 = S.launch(co, s1, s2, x, LC=LC)
    assert np.isinf(y).any() and np.isnan(y).any() and np.isfinite(y).any(axis=1).sum() > len(pick) // 2
    same_bits(ry, y, f"LC = {LC}: frames from the edge states")
    same_bits(np.stack([r1, r2]), np.stack([e1, e2]), f"LC = {LC}: end state from the edge states")


def tolerance_bound_passes(y, ys, truth):
    """the two rules of tests/test_gpu_svf_par.py: per voice err <= R * err_ser + 2^-23 * peak, and bank-wide no worse than the serial tick"""
    err = np.abs(y.astype(np.float64) - truth).max(axis=1)
    err_ser = np.abs(ys.astype(np.float64) - truth).max(axis=1)
    peak = np.abs(truth).max(axis=1)
    return bool((err <= R * err_ser + np.ldexp(peak, -23)).all() and err.max() <= err_ser.max())


def test_every_fault_changes_bits_and_the_tolerance_bound_lets_some_pass():
    """Each single fault of svf_par_ref.FAULTS against the stated order, on the banks above (2 x 2 304 voices x 320 frames, carried
    state), and whether the tolerance bound of tests/test_gpu_svf_par.py (both rules, on the noise bank and on the FM bank) would let
    it pass.  Measured here (samples of 1 474 560, voices of 4 608 whose frames or end state change):

        fault                    passes the bound    samples changed    voices changed
        fix_unfused              yes                        97 612             4 427
        fix_fma_other_product    yes                       159 298             4 568
        carry_unfused            yes                       158 225             3 042
        carry_z_in_fma           yes                       282 558             4 470
        chunk0_from_state        yes                       977 091             4 608
        tables_f32               no                        863 317             4 608
        carry_next_z             no                      1 316 513             4 608
        r_late                   no                      1 461 784             4 608

    Five of the eight pass the bound: that is why the bit tests exist.  (A fused multiply-add that rounds twice instead of once passes
    even the frame comparison above on these inputs; the crafted triples of test_fma32_equals_fmaf are what tells it apart.)"""
    co, s1, s2, x, half = banks()
    truth, _, _ = S.serial(co, s1, s2, x, dtype=np.float64)
    ys, _, _ = S.serial(co, s1, s2, x)
    y, e1, e2 = S.launch(co, s1, s2, x)
    both = lambda yy: all(tolerance_bound_passes(yy[h], ys[h], truth[h]) for h in (slice(0, half), slice(half, None)))
    assert both(y), "the stated order itself is within the bound"
    passing = []
    print()
    for name in S.FAULTS:
        fy, f1, f2 = S.launch(co, s1, s2, x, fault=name)
        frames = S.bits(fy) != S.bits(y)
        voices = frames.any(axis=1) | (S.bits(f1) != S.bits(e1)) | (S.bits(f2) != S.bits(e2))
        ok = both(fy)
        print(f"{name:24s} passes the bound: {'yes' if ok else 'no':3s}  samples changed {frames.sum():8d} of {frames.size}  voices changed {voices.sum():5d} of {len(voices)}")
        assert voices.any(), f"{name} changes no bit: the inputs do not reach it"
        if ok:
            passing.append(name)
    assert passing, "no fault passes the tolerance bound: then the bound alone would do"
