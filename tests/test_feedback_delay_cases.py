"""The tables of feedback_delay_cases.py cover what test_gpu_feedback_delay_matrix.py claims, and the oracle alone meets every side condition
the GPU test relies on (finite, a tail that sounds, an input that straddles the flush threshold) -- checked on the host, so that an edit which
thins a table or moves a row off its edge fails where every change is tested, not only on a GPU."""
import itertools

import numpy as np
import pytest

import fdn_frames_cases as K
import feedback_delay_cases as FC

ORACLE_SOUNDS = 1e-7     # 100 x the bar the GPU test applies to the device's samples (SOUNDS = 1e-9)
ALL_ROWS = [(t, i) for t in ("short", "step") for i in range(len(FC.TABLES[t][0]))]
ALL_IDS = [f"{t}-{FC.row_id(FC.TABLES[t][0][i])}" for t, i in ALL_ROWS]


# ---- the tables --------------------------------------------------------------------------------------------------------------------------------
def test_short_ring_table_holds_every_instantiation_twice():
    count = {}
    for r in FC.SHORT:
        count[(r[0], r[4])] = count.get((r[0], r[4]), 0) + 1
    assert count == {nk: 2 for nk in itertools.product((1, 2), (0, 1, 2, 3))} and len(FC.SHORT) == 16


def test_short_ring_table_holds_every_pair_of_branches_the_grammar_allows():
    col = dict(filter=lambda r: FC.kind(r[3]), place=lambda r: r[2], line_gain=lambda r: r[5], outer=lambda r: r[6], per=lambda r: FC.is_per(r[7]),
               reverse=lambda r: r[1])
    values = dict(filter=(None, "lowpole", "svf"), place=("line", "loop"), line_gain=(True, False), outer=(True, False), per=(True, False),
                  reverse=(True, False))
    excluded = {("filter", "place"): {(None, "loop")}, ("place", "outer"): {("loop", True)}}   # the loop form needs a filter and has no outer gain
    for a, b in itertools.combinations(col, 2):
        rows = [r for r in FC.SHORT if r[0] == 2] if "reverse" in (a, b) else FC.SHORT         # reverse() exists with two channels only
        seen = {(col[a](r), col[b](r)) for r in rows}
        want = set(itertools.product(values[a], values[b])) - excluded.get((a, b), set())
        assert seen == want, (a, b, want - seen, seen - want)
    for r in FC.SHORT + FC.STEP:
        N, rev, place, filt, taps, lg, og, delays = r
        assert not (place == "loop" and (filt is None or og)) and not (N == 1 and rev) and np.shape(delays)[-1] == N
        assert filt is not None or taps or lg or og                                             # something damps the loop
    for t, i in FC.LINE_GAIN_SCALE:                                                             # (only rows that nothing but that gain damps)
        r = FC.TABLES[t][0][i]
        assert r[4] == 0 and r[5] and not r[6] and not FC.is_per(r[7]) and np.all(FC.row_params(t, i)["line_gain"] < 0.31)


def test_every_taps_value_meets_every_filter_kind():
    seen = {(r[4], FC.kind(r[3])) for r in FC.SHORT + FC.STEP}
    assert seen == set(itertools.product((0, 1, 2, 3), (None, "lowpole", "svf")))
    assert {r[3] for r in FC.SHORT} == {None, "lowpole", "lowpass", "bell", "highshelf"}


def test_mirror_top_delays_are_what_the_tables_use():
    assert {143, 207} <= K.mirror_top_delays(K.CUTS, 256) and {220, 399} <= K.mirror_top_delays(K.CUTS_STEP, 512)
    assert not {128, 255} & K.mirror_top_delays(K.CUTS, 256)               # (the edge case of test_gpu_feedback_delay.py reaches no such slot)
    for per, top in ((FC.PER1, {143, 207}), (FC.PER2, {143, 207}), (FC.PER_STEP, {220, 399})):
        assert len(per) == FC.V == 5 and top <= {k for r in per[1:3] for k in r}                 # in instances 1 and 2
        assert set(per[K.ALL_SHORTEST]) == {K.SHORTEST} and len(set(per)) == FC.V
    assert len({0, K.DENORMAL, K.IMPULSE, K.ALL_SHORTEST, FC.FLUSH_EDGE}) == 5


@pytest.mark.parametrize("table,index", ALL_ROWS, ids=ALL_IDS)
def test_every_row_has_the_len_and_cap_it_is_about(table, index):
    rows, cap_claimed, T, cuts = FC.TABLES[table]
    N, rev, place, filt, taps, lg, og, delays = rows[index]
    p = FC.row_params(table, index)
    lens, cap = FC.row_ring(p)
    assert np.array_equal(lens - 1, np.asarray(delays)) and cap == cap_claimed and lens.min() >= K.SHORTEST + 1 and lens.max() <= cap
    assert cuts[-1] == T and T >= 7 * cap
    if FC.is_per(delays):   # both edges in one launch: an instance with every line at 128 samples, another with the line that fills the shared capacity
        assert lens.shape == (FC.V, N) and np.all(lens[K.ALL_SHORTEST] == K.SHORTEST + 1) and lens[0].max() == cap
        assert lens.min() == K.SHORTEST + 1 and {int(k) - 1 for k in lens[1:3].ravel()} & K.mirror_top_delays(cuts, cap)
    elif table == "short":
        assert lens.min() == K.SHORTEST + 1 or lens.max() == cap                              # one channel: one edge per row
        assert N == 1 or (lens.min() == K.SHORTEST + 1 and lens.max() == cap)
    if table == "step":
        assert (index in FC.STEP_FIRST_LENGTH_OF_512) == (257 in lens) and (index in FC.STEP_FULL) == (512 in lens)
        assert N == 1 or lens.min() == K.SHORTEST + 1


def test_the_short_rows_of_one_channel_hold_both_edges_for_every_taps_value():
    for taps in (0, 1, 2, 3):
        seen = set()
        for r in FC.SHORT:
            if r[0] == 1 and r[4] == taps:
                seen |= {int(k) for k in np.asarray(r[7]).ravel()}
        assert {128, 255} <= seen, (taps, seen)


def test_step_table():
    assert [(r[0], r[4]) for r in FC.STEP] == [(1, 2), (1, 1), (2, 3), (2, 0), (2, 2)]
    assert set(FC.STEP_FIRST_LENGTH_OF_512) | set(FC.STEP_FULL) == set(range(len(FC.STEP)))
    assert K.T_STEP >= 3 * 512 and 1 in np.diff(K.CUTS_STEP)


def test_the_ladder_reaches_every_capacity():
    assert list(FC.LADDER) == list(range(8, 19))
    for log2 in FC.LADDER:
        cap = 1 << log2
        lens, got = FC.row_ring(FC.ladder_params(log2))
        assert got == cap and list(lens) == [K.SHORTEST + 1, cap]
        cuts = K.reverb_cuts(cap)
        assert cuts[-1] == cap + 205 and cap - 64 < cuts[2] < cap and cuts[1] % 64 and (cuts[2] - cuts[1]) % 64
    assert [(r[0], r[1]) for r in FC.NETWORK_LADDER] == [(10, 2), (14, 2), (18, 32)]
    for row in FC.NETWORK_LADDER:
        log2, lines = row[:2]
        d = FC.network_delays(log2, lines)
        lens, got = K.ring_of(FC.network_params_of(row)["delays"], FC.SR)
        assert got == 1 << log2 and list(lens - 1) == d and len(set(d)) == lines and d[0] == K.SHORTEST and d[1] == (1 << log2) - 1
    assert FC.NETWORK_LADDER[2][2:] == ("lowpass", "line", 3, False, 2, 2)
    assert FC.LARGEST_RING_BYTES == 33562624 < 2 ** 31                  # (the ring steps form their offsets in 32 bits)
    assert max(K.reverb_cuts(1 << 18)) == 262349


# ---- the oracle alone --------------------------------------------------------------------------------------------------------------------------
def test_the_flush_edge_scale_falls_through_the_threshold():
    for T in (FC.SHORT_T, FC.STEP_T):
        s, stop = FC.flush_edge_scale(T), 2 * T // 3
        assert s.dtype == np.float32 and s[0] == np.float32(1e-35) and np.all(np.diff(s.astype(np.float64)) < 0)
        assert 0.99e-38 < float(s[stop]) < 1.01e-38 < float(FC.SMALLEST_NORMAL) < float(s[stop // 2])
        x = FC.matrix_signal(2, T, 1)
        assert not x[FC.FLUSH_EDGE][:, stop:].any() and np.array_equal(x[K.IMPULSE][:, :2], [[1.0, 0.0]] * 2) and not x[K.IMPULSE][:, 1:].any()


@pytest.mark.parametrize("table,index", ALL_ROWS, ids=ALL_IDS)
def test_oracle_side_conditions_of_the_matrix_rows(table, index):
    """what the GPU test then asks of the device's samples, asked of the oracle with a hundredfold margin; and the FLUSH_EDGE instance's output
    straddles the threshold: samples right above it, and a share of zeros that is neither everything nor nothing"""
    T = FC.TABLES[table][2]
    p, x, want = FC.reference(table, index)
    assert want.shape == x.shape and np.isfinite(want).all()
    peak = float(np.abs(want[K.IMPULSE][:, 2 * T // 3:]).max())                                  # the maximum over the bank's channels
    assert peak > ORACLE_SOUNDS, peak
    assert not np.any((want != 0) & (np.abs(want) < FC.SMALLEST_NORMAL))                        # the oracle flushes: Feedback::new
    edge = want[FC.FLUSH_EDGE][:, :2 * T // 3]
    low = int(np.count_nonzero((edge != 0) & (np.abs(edge) < 8 * FC.SMALLEST_NORMAL)))
    share = np.count_nonzero(edge) / edge.size
    print(f"{table} {FC.row_id(FC.TABLES[table][0][index])}: impulse tail {peak:.3g}, {low} samples under 8 * 2^-126, non-zero share {share:.3f}")
    assert low >= 50 and 0.25 < share < 0.95, (low, share)


@pytest.mark.parametrize("log2", FC.LADDER)
def test_oracle_side_conditions_of_the_ladder(log2):
    p, x, want = FC.ladder_reference(log2)
    tail = np.abs(want[:, :, 1 << log2:]).max(axis=2)
    print(f"2^{log2}: the frames from cap on peak at {tail.min():.3g} at least")
    assert np.isfinite(want).all() and tail.min() > ORACLE_SOUNDS, tail


@pytest.mark.parametrize("index", range(len(FC.NETWORK_LADDER)), ids=[f"2^{r[0]}-{r[1]}lines" for r in FC.NETWORK_LADDER])
def test_oracle_side_conditions_of_the_network_ladder(index):
    p, x, want = FC.network_reference(index)
    tail = np.abs(want[:, :, 1 << FC.NETWORK_LADDER[index][0]:]).max(axis=2)
    print(f"{FC.NETWORK_LADDER[index][:2]}: the frames from cap on peak at {tail.min():.3g} at least")
    assert np.isfinite(want).all() and tail.min() > ORACLE_SOUNDS, tail
