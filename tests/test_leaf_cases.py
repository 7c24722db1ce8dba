"""The leaf table (leaf_cases.py) without a device: it has a row for exactly the kinds register_leaf_kinds registers, and the oracle ALONE meets every
condition tests/test_gpu_leaf_matrix.py relies on -- so a device render that equals the oracle's is a render of finite, still moving samples, not of
a constant that would hide a lost state."""
import os
import re

import numpy as np
import pytest

import leaf_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = sorted(L.TABLE)
DISTINCT = 8
LAST = L.LAUNCHES[-1]


def registered_leaf_kinds():
    src = open(os.path.join(ROOT, "fundsp_amd", "csrc", "fd_kinds_leaf.hip")).read()
    body = src[src.index("void register_leaf_kinds"):]
    return re.findall(r'make_kind<.*>\("(\w+)"\)', body)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def distinct(a):
    """distinct bit patterns of [OUT][frames]; a stream of +-1 alone (mls, a PolyBLEP square at a negative frequency, which has no corrections)
    carries its information in the order: distinct windows of 16 consecutive samples"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if np.all(np.abs(a) == 1.0):
        return max(len({row[i:i + 16].tobytes() for i in range(row.size - 15)}) for row in a)
    return len(np.unique(bits(a)))


def test_the_table_has_a_row_for_exactly_the_registered_leaf_kinds():
    names = registered_leaf_kinds()
    assert len(names) == len(set(names)) >= 59
    assert sorted(names) == KINDS, (sorted(set(names) - set(KINDS)), sorted(set(KINDS) - set(names)))
    for kind, r in L.TABLE.items():
        assert r.kind == kind and r.voices == (L.V_BANK if kind == "biquad_bank" else L.V) and r.voices % r.group == 0


def test_the_launches_are_the_four_lengths_and_the_rates_differ():
    assert [b - a for a, b in L.LAUNCHES] == [141, 1, 64, 83] and 141 == 2 * 64 + 8 + 5 and L.T_RATE == 77 and L.T_ALL == 366
    assert (L.SR, L.SR2) == (48000.0, 44100.0) and L.V == 64 + 3 and L.V_BANK % 8 == 0


@pytest.mark.parametrize("kind", KINDS)
def test_the_oracle_sounds_in_both_executors(kind):
    r = L.TABLE[kind]
    a, b = LAST
    for ex in L.EXECUTORS:
        x, want, again = L.reference(kind, ex)
        ni = 0 if x is None else x.shape[1]
        assert want.shape[0] == r.voices and want.shape[2] == L.T_ALL and (x is None or (np.isfinite(x).all() and x.shape == (r.voices, ni, L.T_ALL)))
        assert np.isfinite(want).all() and np.isfinite(again).all(), f"{kind} {ex}: voices {sorted(set(np.argwhere(~np.isfinite(want))[:, 0]))} leave the finite numbers"
        sounding = 0
        for v in range(r.voices):
            assert distinct(want[v][:, a:b]) >= DISTINCT, f"{kind} {ex} voice {v}: {distinct(want[v][:, a:b])} distinct values in the last launch at SR"
            d = distinct(want[v][:, b:])
            emptied = r.ring_frames and not want[v][:, b:b + 32].any()   # a line emptied by the change of rate: its length in silence is the answer
            assert d >= DISTINCT or emptied, f"{kind} {ex} voice {v}: {d} distinct values after the rate change"
            sounding += d >= DISTINCT
        assert sounding >= (r.voices if not r.ring_frames else 8)
        if x is not None and r.chans[0].__qualname__.startswith("audio"):   # the 1e-30 voice stays in play: tiny, never flushed to a constant zero
            assert 0 < np.abs(x[L.TINY, 0]).max() < 2e-30 and distinct(want[L.TINY][:, a:b]) >= DISTINCT


@pytest.mark.parametrize("kind", KINDS)
def test_the_flags_say_what_the_oracle_does(kind):
    r = L.TABLE[kind]
    p, t = L.reference(kind, "process"), L.reference(kind, "tick")
    assert r.executors_agree == bool(np.array_equal(bits(p[1]), bits(t[1]))), f"{kind}: executors_agree is {r.executors_agree}"
    for x, want, again in (p, t):
        same = bool(np.array_equal(bits(again), bits(want[:, :, :L.CUTS[1]])))
        assert r.reset_restores == same, f"{kind}: reset_restores is {r.reset_restores}"
    assert p[0] is t[0] or np.array_equal(p[0], t[0])      # both executors hear the same inputs
    assert not p[1].flags.writeable


def test_rows_that_tell_the_executors_apart():
    """the rows whose two oracle renders differ are the ones a kernel instantiated with the wrong MODE cannot pass"""
    apart = sorted(k for k, r in L.TABLE.items() if not r.executors_agree)
    assert apart == sorted(["sine", "saw", "square", "triangle", "adsr_live", "lfo_exp", "lfo_sine_hz", "lfo2_exp", "shape"])
    assert [k for k, r in L.TABLE.items() if not r.reset_restores] == ["adsr_live"]


@pytest.mark.parametrize("kind", [k for k in KINDS if L.TABLE[k].ring_frames])
def test_every_ring_fits_its_longest_delay_at_both_rates(kind):
    r = L.TABLE[kind]
    for sr in (L.SR, L.SR2):
        assert 1 <= r.longest(sr) <= r.ring_frames, f"{kind} at {sr}: {r.longest(sr)} positions in a ring of {r.ring_frames}"
    assert r.longest(L.SR) != r.longest(L.SR2) or kind.startswith("tap")    # the change of rate re-sizes the line (taps: a power of two either way)


def test_ring_rows_are_the_kinds_with_rings():
    assert sorted(k for k in KINDS if L.TABLE[k].ring_frames) == ["allnest_delay", "delay", "pluck", "tap", "tap_linear"]


def test_shape_and_svf_rows_cover_every_case():
    s = L.TABLE["shape"].slots
    assert sorted(set(s[":shape"].astype(int))) == sorted(L.O.SHAPES[c[0]] for c in L.SHAPE_CASES)
    assert sorted(set(L.TABLE["fixed_svf"].slots[":mode"].astype(int))) == list(range(9))
    for k in ("fbiquad_hz", "dbiquad_hz"):
        assert len(set(zip(L.TABLE[k].slots[":mode"], L.TABLE[k].slots["0:shape"]))) == 4 * len(L.SHAPE_CASES)


def test_the_adsr_gate_has_edges_on_and_inside_the_launches():
    g = L.row_inputs("adsr_live")[:, 0]
    edges = {int(i) + 1 for v in range(L.V) for i in np.flatnonzero(g[v, 1:] != g[v, :-1])}
    assert set(L.CUTS[1:]) <= edges and any(e not in L.CUTS for e in edges)


# ---- a defect of the oracle that the matrix found, pinned against the reference's arithmetic restated here ------------------------------------
@pytest.mark.parametrize("dirty", [False, True], ids=["fb", "dirty"])
def test_an_adaptive_shape_inside_a_nonlinear_biquad_keeps_the_smoothing_of_its_construction_rate(dirty):
    """FixedFbBiquad / FixedDirtyBiquad::set_sample_rate set the rate and the coefficients and nothing else (biquad.rs:678-681, 898-901): the
    Adaptive shape inside keeps pow(0.5, 1 / (timescale * DEFAULT_SR)) from Adaptive::new (shape.rs:174-182), at 48 kHz as at 44.1 kHz.  Shaper does
    pass the rate on (shape.rs:232-234).  The oracle used to move the smoothing of both."""
    f32, O = np.float32, L.O
    h, ts, center, q = f32(1.5), f32(0.05), 700.0, 2.0
    x = L.audio()(2, 300, L.rng_of("pin"))[0]
    tanh = lambda v: f32(O.lib().o_math_tanhf(float(v)))
    for sr in (48000.0, 44100.0, 96000.0):
        n = O.nlbiquad(dirty, 1, "lowpass", "adaptive_tanh", float(h), float(ts), center, q)
        n.set_sample_rate(sr)
        a1, a2, b0, b1, b2 = O.biquad_coefs("lowpass", sr, center, q)
        sm = f32(0.5 ** (1.0 / (float(ts) * O.DEFAULT_SR)))
        st, s1, s2 = [f32(0.0), f32(0.0)], f32(0.0), f32(0.0)      # Adaptive::new: state 0.0 (no reset here)

        def adaptive(i, v):
            st[i] = sm * st[i] + (f32(1.0) - sm) * (f32(1.0e-6) + v * v)
            return tanh(v / np.sqrt(st[i]) * h)
        want = np.zeros(x.size, dtype=f32)
        for t, x0 in enumerate(x):
            y0 = b0 * x0 + s1
            if dirty:       # biquad.rs:903-914
                s1, s2 = adaptive(0, s2 + b1 * x0 - y0 * a1), adaptive(1, b2 * x0 - y0 * a2)
            else:           # :683-690
                fb = adaptive(0, y0)
                s1, s2 = s2 + b1 * x0 - fb * a1, b2 * x0 - fb * a2
            want[t] = y0
        assert np.array_equal(bits(n.render_ticks(x)[0]), bits(want)), f"nonlinear biquad, dirty={dirty}, at {sr}"
    # ... while Shaper<Adaptive<Tanh>> follows the rate
    for sr in (48000.0, 44100.0):
        n = O.shape("adaptive_tanh", float(h), float(ts))
        n.set_sample_rate(sr)
        sm, st = f32(0.5 ** (1.0 / (float(ts) * sr))), f32(0.0)
        want = np.zeros(x.size, dtype=f32)
        for t, v in enumerate(x):
            st = sm * st + (f32(1.0) - sm) * (f32(1.0e-6) + v * v)
            want[t] = tanh(v / np.sqrt(st) * h)
        assert np.array_equal(bits(n.render_ticks(x)[0]), bits(want)), f"Shaper at {sr}"
