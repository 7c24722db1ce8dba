"""The tables of fdn_frames_cases.py cover what test_gpu_fdn_frames_matrix.py claims -- checked on the host, so that an edit which thins
them fails where every change is tested, not only on a GPU."""
import itertools

import numpy as np

import fdn_frames_cases as K
import oracle as O


def test_generic_table_covers_all_15_instantiations():
    assert len(K.GENERIC_CASES) == 15
    assert {(r[0], r[1]) for r in K.GENERIC_CASES} == set(itertools.product(K.LINES, (1, 2, 3)))
    for n, taps, w, nin, nout in K.GENERIC_CASES:
        assert len(w) == taps and len(set(w)) == taps and abs(sum(w)) < 1.0          # distinct taps, a damped loop
    for n in K.LINES:   # a Join and a MultiJoin per lines value (the one step where the executors differ in arithmetic)
        assert {r[4] for r in K.GENERIC_CASES if r[0] == n} == {1, 2}
    assert {(r[3], r[4]) for r in K.GENERIC_CASES} == set(K.IO)


def test_filtered_table_covers_all_20_instantiations_and_every_pair_of_branches():
    rows = K.FILTERED_CASES
    assert len(rows) == 20
    assert {(r[0], r[1]) for r in rows} == set(itertools.product(K.LINES, (0, 1, 2, 3)))
    names = ("filter", "place", "gain", "per")
    values = dict(filter=K.FILTERS, place=("line", "loop"), gain=(True, False), per=(True, False))
    col = dict(filter=2, place=3, gain=4, per=5)
    for a, b in itertools.combinations(names, 2):
        seen = {(r[col[a]], r[col[b]]) for r in rows}
        want = set(itertools.product(values[a], values[b])) - {(None, "loop")}       # fdn2 without a filter does not exist
        assert seen == want, (a, b, want - seen)
    assert {(r[1], r[2]) for r in rows} == set(itertools.product((0, 1, 2, 3), K.FILTERS))   # every taps value meets every filter kind
    assert {(r[0], r[3]) for r in rows} == set(itertools.product(K.LINES, ("line", "loop")))  # every lines value meets both places
    assert {(r[6], r[7]) for r in rows} == set(K.IO)


def test_every_short_ring_has_a_line_at_128_samples_and_one_that_fills_the_ring():
    for n in K.LINES:
        s = K.short_ring(n)
        assert len(s) == n == len(set(s)) and s[0] == 128 and s[1] == 255 and all(129 <= k <= 254 for k in s[2:])
        assert n == 2 or len(set(s) & K.mirror_top_delays(K.CUTS, 256)) >= 2        # a read that reaches the mirror's last used slot
        for sr in (K.SR, K.SR_GENERIC):   # whole samples at the bank's rate, through the f32 seconds the reference takes
            lens, cap = K.ring_of(K.seconds(s, sr), sr)
            assert list(lens - 1) == s and cap == 256 and lens.min() == 129 and lens.max() == cap
        per = K.per_instance_samples(s)
        assert per.shape == (K.V, n) and per.min() == 128 and per.max() == 255
        assert np.all(per[K.ALL_SHORTEST] == 128) and list(per[0]) == s and len({tuple(r) for r in per}) == K.V
    assert len({K.DENORMAL, K.IMPULSE, K.ALL_SHORTEST, K.FLUSH_EDGE, 0}) == 5 and K.V == 5 and 1.2e-38 < K.FLUSH_EDGE_SCALE < 32 * 1.2e-38
    assert K.CUTS[0] == 0 and K.CUTS[-1] == K.T == 64 * 30 + 13 and K.T // 256 == 7
    sizes = np.diff(K.CUTS)
    assert 1 in sizes and any(c % 64 for c in K.CUTS[1:-1]) and K.RESET_FRAMES < K.T


def test_capacity_step_tables():
    for table, at in ((K.STEP_GENERIC, 5), (K.STEP_FILTERED, 8)):
        assert {(r[0], r[1]) for r in table} == {(2, 2), (32, 3)}
        seen = {2: set(), 32: set()}      # per lines value: two lines hold one side of the step per row
        for r in table:
            s = K.step_ring(r[0], r[at])
            assert len(s) == r[0] == len(set(s)) and min(s) == 128 and max(s) <= 511
            assert r[0] == 2 or len(set(s) & K.mirror_top_delays(K.CUTS_STEP, 512)) >= 2
            for sr in (K.SR, K.SR_GENERIC):
                lens, cap = K.ring_of(K.seconds(s, sr), sr)
                assert list(lens - 1) == s and cap == 512                            # 257 slots already take the next power of two
            seen[r[0]] |= set(s) & {128, 256, 511}
        assert seen == {2: {128, 256, 511}, 32: {128, 256, 511}}
    assert K.T_STEP >= 3 * 512 and K.CUTS_STEP[-1] == K.T_STEP and 1 in np.diff(K.CUTS_STEP)


def test_reverb_table_reaches_every_capacity_it_claims():
    for nsec in (1, 2):
        rows = [r for r in K.REVERB_CASES if r[0] == nsec]
        assert sorted(r[1] for r in rows) == list(K.REVERB_CAPS) == list(range(9, 19))
        for _, log2, room, sr, tick in rows:
            lens = K.reverb_lens(nsec, room, sr)
            cap = 1 << log2
            assert len(lens) == 32 and cap // 2 < lens.max() <= cap and lens.min() > 128, (nsec, log2, lens.min(), lens.max())
            assert K.reverb_lens(nsec, room, O.DEFAULT_SR).min() > 128                # the bank is created at DEFAULT_SR
            cuts = K.reverb_cuts(cap)
            assert cuts[-1] == cap + 3 * 64 + 13 and cap - 64 < cuts[2] < cap and (cuts[2] - cuts[1]) % 64 and cuts[1] % 64
    assert sum(1 for r in K.REVERB_CASES if r[0] == 2 and r[4]) == 2                  # reverb4_stereo's MultiJoin in the tick executor, twice
    assert set(K.REVERB_UNREACHABLE) | set(K.REVERB_CAPS) == set(range(8, 19))


def test_a_256_slot_ring_is_out_of_reach_of_both_reverbs():
    """every delay in 128 .. 255 samples needs longest / shortest < 2; the tables span more (the arithmetic of the GPU test's docstring)"""
    for nsec, room in ((1, 10.0), (2, 15.0)):
        d = (K.reverb_lens(nsec, room, 1e6) - 1).astype(np.float64)                  # (a rate at which rounding does not matter)
        assert d.max() / d.min() > 255.5 / 127.5
