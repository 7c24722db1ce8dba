"""reverb3_stereo's lane = frame kernel (fd_reverb3.hip: k_rv3_render<0 | 1>, k_rv3_migrate, k_rv3_zero) at every ring capacity an audio rate
reaches, on the ring's edges and across changes of rate, bit for bit against the oracle's Reverb node -- C, per sample, no code shared with
the kernel -- driven through the same set_sample_rate / reset / launch cuts.  tests/test_gpu_reverb3.py renders at 48 and 44.1 kHz only: one
capacity (2048), no line near either end of the ring, rate changes between rings of one size.  The tables are reverb3_cases.py, checked
without a device by test_reverb3_cases.py (there also: rv3_make_const itself against the restated arithmetic).

(a) every row of the rate table -- capacities 512 .. 16384, each with its full ring (longest distance == cap - 64: the oldest slot is read
    right before it is overwritten) and, from 1024 on, its emptiest; 14 057 Hz with a line at 129 samples, the shortest accepted: the next
    block's prefetch sits 65 slots behind this block's write window -- lowpole filter, five instances (the second workgroup has one live
    wave; one instance among the denormals, which this translation unit keeps; one unit impulse), planar, process; the row's cuts place a
    block at wp == 64 and one at cap - 64, launches beginning at wp == 37 and cap - 10, block heads whose read of the longest / the shortest
    allpass line starts in slot cap - 1 and runs through the whole mirror, launches of 1, 1 and 62 frames.  Then reset() and cap + 100
    frames again: the pre rings keep their write position (205 mod 512), so the two halves of the wide condition disagree.
(b) the full-ring rows and the 14 057 Hz row once more with highshelf_hz(5000, 1, 0.8912509) in the loop (k_rv3_render<1>) and once in the
    tick executor, voice-minor; one row with 70 instances voice-minor (the planar staging copy).
(c) changes of rate between rings of different capacity, stopped off the grid past two wraps, at wold == 0, and after 70 frames; two changes
    in a row, a change after reset(), to the same rate, by half a hertz, a clone after a change; two pairs with the SVF.
(d) the refusals at 14 056 Hz and 50 MHz, first thing and in mid-tail; the bank goes on at its old rate.
(e) Bank.from_graph at 22 050 Hz against the run-time compiled lane-per-voice node.

No tolerance appears in this file."""
import functools

import numpy as np
import pytest

import oracle as O
import reverb3_cases as K
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from fundsp_amd import graph as GR
from test_gpu_fdn import run
from test_gpu_parity import assert_bit_equal
from test_gpu_reverb3 import oracle_rv3, signal

pytestmark = pytest.mark.gpu
# A tail that "still sounds" is one of normal numbers with all 24 bits of mantissa in play (test_gpu_fdn_frames_matrix.py)
SOUNDS = 1e-9
TIME, DIFFUSION, CUTOFF = 2.0, 0.6, 1800.0
SHELF = (5000.0, 1.0, 0.8912509)           # examples/keys.rs:134: highshelf_hz(5000.0, 1.0, db_amp(-1.0))
RATE_IDS = [f"{int(r[0])}Hz-cap{r[3]}" for r in K.RATES]
EDGE_IDS = [f"{int(r[0])}Hz-cap{r[3]}" for r in K.EDGE_RATES]


def frozen(a):
    a.setflags(write=False)
    return a


def make_oracle(filt, sr, diffusion=DIFFUSION):
    if filt == "lowpole":
        return oracle_rv3(TIME, diffusion, CUTOFF, sr)
    n = O.reverb3_stereo(TIME, diffusion, lambda: O.highshelf_hz(*SHELF))
    n.set_sample_rate(sr)
    return n


def make_bank(gpu, filt, V, sr=None, diffusion=DIFFUSION):
    if filt == "lowpole":
        b = gpu.Bank.reverb3_stereo(V, TIME, diffusion, CUTOFF)
    else:
        b = gpu.Bank.reverb3_stereo(V, TIME, diffusion, SHELF[0], svf="highshelf", q=SHELF[1], gain=SHELF[2])
    if sr is not None:
        b.set_sample_rate(sr)
    return b


def oracle_render(n, x, cuts, mode):
    return np.concatenate([n.render_blocks(x[:, a:e]) if mode == MODE_PROCESS else n.render_ticks(x[:, a:e]) for a, e in zip(cuts[:-1], cuts[1:])], axis=1)


@functools.lru_cache(maxsize=None)
def row_reference(rate, filt, mode, with_reset):
    """(input, the oracle's render of every instance over the row's cuts, and of the first cap + 100 frames after reset()): computed once per
    row, filter and executor, shared by the layouts"""
    c = K.make_const(rate)
    cuts, T = K.cuts(c), K.total(c["cap"])
    x = signal(K.V, T, 900 + c["cap"] // 256 + int(rate) % 97)
    want, again = [], []
    rs = K.reset_cuts(c["cap"])
    for v in range(K.V):
        n = make_oracle(filt, rate)
        want.append(oracle_render(n, x[v], cuts, mode))
        if with_reset:
            n.reset()
            again.append(oracle_render(n, x[v][:, :rs[-1]], rs, mode))
    return frozen(x), frozen(np.stack(want)), frozen(np.stack(again)) if with_reset else None


def check_row(gpu, row, filt, layout, mode, with_reset):
    rate, shortest, longest, cap, why = row
    c = K.make_const(rate)
    assert (c["shortest"], c["longest"], c["cap"]) == (shortest, longest, cap)          # the case is about these numbers
    cuts, T = K.cuts(c), K.total(cap)
    x, want, again = row_reference(rate, filt, mode, with_reset)
    b = make_bank(gpu, filt, K.V, rate)
    assert b.inputs() == 2 and b.outputs() == 2
    got = run(b, x, layout, mode, list(cuts))
    assert b.get_option("last_kernel") == 6
    what = f"reverb3_stereo {filt} at {rate} Hz (cap {cap}, distances {shortest} .. {longest})"
    for v in range(K.V):
        assert_bit_equal(got[v], want[v], f"{what} instance {v}")
    assert np.isfinite(got).all()
    assert np.abs(got[K.IMPULSE][:, 2 * T // 3:]).max() > SOUNDS and np.abs(got[0][:, cuts[-2]:]).max() > SOUNDS    # no comparison of zeros
    assert 0.0 < np.abs(got[K.DENORMAL]).max() < 1e-30                                  # the quiet instance stays where it is: nothing was flushed
    if with_reset:
        b.reset()
        rs = K.reset_cuts(cap)
        back = run(b, x[:, :, :rs[-1]], layout, mode, list(rs))
        for v in range(K.V):
            assert_bit_equal(back[v], again[v], f"{what} after reset() instance {v}")


# ---- (a) every rate row --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", K.RATES, ids=RATE_IDS)
def test_every_ring_capacity_and_edge(gpu, row):
    check_row(gpu, row, "lowpole", LAYOUT_PLANAR, MODE_PROCESS, True)


# ---- (b) both kernels and layouts on the edge rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("row", K.EDGE_RATES, ids=EDGE_IDS)
def test_edge_rows_with_the_svf_in_the_loop(gpu, row):
    check_row(gpu, row, "highshelf", LAYOUT_PLANAR, MODE_PROCESS, False)


@pytest.mark.parametrize("row", K.EDGE_RATES, ids=EDGE_IDS)
def test_edge_rows_tick_executor_voice_minor(gpu, row):
    check_row(gpu, row, "lowpole", LAYOUT_VOICE_MINOR, MODE_TICK, False)


def test_full_1024_ring_with_70_instances_through_the_staging_copy(gpu):
    row = [r for r in K.FULL_RATES if r[3] == 1024][0]
    rate, cap = row[0], row[3]
    c = K.make_const(rate)
    cuts, T, V = K.cuts(c), K.total(cap), 70
    x = signal(V, T, 77)
    a = make_bank(gpu, "lowpole", V, rate)
    b = make_bank(gpu, "lowpole", V, rate)
    vm = run(a, x, LAYOUT_VOICE_MINOR, MODE_PROCESS, list(cuts))      # >= 64 instances: through the planar staging copy
    pl = run(b, x, LAYOUT_PLANAR, MODE_PROCESS, list(cuts))
    assert a.get_option("last_kernel") == 6 and b.get_option("last_kernel") == 6
    assert_bit_equal(vm, pl, "voice-minor (staged) == planar")
    for v in (0, 63, 64, 69):
        assert_bit_equal(vm[v], oracle_render(make_oracle("lowpole", rate), x[v], cuts, MODE_PROCESS), f"instance {v} of {V} at {rate} Hz")
    assert np.abs(vm[69][:, cuts[-2]:]).max() > SOUNDS


# ---- (c) rate changes across capacities ----------------------------------------------------------------------------------------------
def moved_signal(V, T1, total, seed):
    """noise up to T1 (the quiet instance and the impulse as in signal()), then silence"""
    x = signal(V, total, seed)
    x[0, :, :T1] = (np.random.default_rng(seed + 1).random((2, T1), dtype=np.float32) * 2 - 1).astype(np.float32)
    x[:, :, T1:] = 0.0
    return x


def play(gpu, filt, V, script, x, layout=LAYOUT_PLANAR, mode=MODE_PROCESS):
    """The same script for a bank and for one oracle node per instance.  Steps: ("rate", sr) | ("refused", sr) -- the bank must refuse, the
    oracle is never asked | ("reset",) | ("clone",) -- from here on a clone is rendered as well and must equal the original |
    ("render", cuts) -- consumes the next cuts[-1] frames of x.  Returns the renders of the bank, checked against the oracle's."""
    bank, clone = make_bank(gpu, filt, V, diffusion=K.DIFFUSION_MOVED), None
    nodes = [make_oracle(filt, O.DEFAULT_SR, K.DIFFUSION_MOVED) for _ in range(V)]
    at, renders = 0, []
    for step in script:
        if step[0] == "rate":
            for b in (bank, clone):
                if b is not None:
                    b.set_sample_rate(step[1])
            for n in nodes:
                n.set_sample_rate(step[1])
        elif step[0] == "refused":
            was = bank.sample_rate
            with pytest.raises(gpu.FdspError, match="128 samples.*14057 Hz.*2\\^20 samples"):
                bank.set_sample_rate(step[1])
            assert bank.sample_rate == was
        elif step[0] == "reset":
            bank.reset()
            for n in nodes:
                n.reset()
        elif step[0] == "clone":
            clone = bank.clone()
        else:
            cuts = step[1]
            part = x[:, :, at:at + cuts[-1]]
            at += cuts[-1]
            got = run(bank, part, layout, mode, list(cuts))
            assert bank.get_option("last_kernel") == 6
            for v in range(V):
                assert_bit_equal(got[v], oracle_render(nodes[v], part[v], cuts, mode), f"render {len(renders)} of {script}: instance {v}")
            if clone is not None:
                assert_bit_equal(run(clone, part, layout, mode, list(cuts)), got, f"render {len(renders)} of {script}: the clone")
            renders.append(got)
    assert at == x.shape[2]
    return renders


def change_script(a, b, stop):
    ca, cb = K.make_const(a), K.make_const(b)
    T1 = K.first_render(stop, ca["cap"])
    first = (0, T1) if T1 < 128 else (0, 64 * 2 + 5, T1)
    return [("rate", a), ("render", first), ("rate", b), ("render", K.after_cuts(cb))], T1, T1 + K.after_cuts(cb)[-1]


def sounds_at_once(part):
    """what survived the move sounds in the first block (a fresh node would be silent: the input is)"""
    return np.abs(part[0][:, :64]).max() > SOUNDS


PAIR_IDS = [f"{int(a)}to{int(b)}" for a, b in K.MIGRATE_PAIRS]


@pytest.mark.parametrize("stop", K.STOPS)
@pytest.mark.parametrize("pair", K.MIGRATE_PAIRS, ids=PAIR_IDS)
def test_rate_change_between_rings_of_different_capacity(gpu, pair, stop):
    script, T1, total = change_script(*pair, stop)
    x = moved_signal(3, T1, total, 400 + T1 % 89)
    first, after = play(gpu, "lowpole", 3, script, x)
    assert sounds_at_once(after), f"{pair} {stop}: silent after the change"
    assert np.abs(x[:, :, T1:]).max() == 0.0


@pytest.mark.parametrize("pair", [K.MIGRATE_PAIRS[0], K.MIGRATE_PAIRS[2]], ids=[PAIR_IDS[0], PAIR_IDS[2]])
def test_rate_change_with_the_svf_in_the_loop(gpu, pair):
    """the coefficients follow the rate, ic1eq / ic2eq stay"""
    script, T1, total = change_script(*pair, "unaligned")
    x = moved_signal(3, T1, total, 500)
    first, after = play(gpu, "highshelf", 3, script, x, LAYOUT_VOICE_MINOR, MODE_TICK)
    assert sounds_at_once(after)


A, B = 48000.0, 16000.0
KA, KB = K.make_const(A), K.make_const(B)
CA, CB = KA["cap"], KB["cap"]
T1_AB = K.first_render("unaligned", CA)
FIRST_AB = (0, 64 * 2 + 5, T1_AB)
SEQUENCES = {
    "two-changes-no-render-between": [("rate", A), ("render", FIRST_AB), ("rate", B), ("rate", A), ("render", K.after_cuts(KA))],
    "there-and-on-to-a-third": [("rate", A), ("render", FIRST_AB), ("rate", B), ("rate", 96000.0), ("render", K.after_cuts(K.make_const(96000.0)))],
    "change-straight-after-reset": [("rate", A), ("render", FIRST_AB), ("reset",), ("rate", B), ("render", K.after_cuts(KB))],
    "half-a-hertz-down-same-distances": [("rate", A), ("render", FIRST_AB), ("rate", A - 0.5), ("render", K.after_cuts(KA))],
    "half-a-hertz-up": [("rate", A), ("render", FIRST_AB), ("rate", A + 0.5), ("render", K.after_cuts(KA))],
    "clone-after-a-change": [("rate", A), ("render", FIRST_AB), ("rate", B), ("clone",), ("render", K.after_cuts(KB)), ("rate", A), ("render", K.after_cuts(KA))],
    "clone-before-a-change": [("rate", B), ("render", (0, 2 * CB + 87)), ("clone",), ("rate", A), ("render", K.after_cuts(KA))],
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_rate_change_sequences(gpu, name):
    script = SEQUENCES[name]
    T1 = script[1][1][-1]
    x = moved_signal(3, T1, sum(s[1][-1] for s in script if s[0] == "render"), 600)
    renders = play(gpu, "lowpole", 3, script, x)
    assert all(sounds_at_once(r) for r in renders[1:])     # (after reset() the input diffusers alone are left -- and sound)


def test_a_change_to_the_same_rate_does_nothing(gpu):
    x = moved_signal(3, T1_AB, T1_AB + 64 * 9 + 3, 700)
    script = [("rate", A), ("render", FIRST_AB), ("rate", A), ("render", (0, 64 * 9 + 3))]
    moved = play(gpu, "lowpole", 3, script, x)
    twin = play(gpu, "lowpole", 3, [script[0], script[1], script[3]], x)
    assert_bit_equal(moved[1], twin[1], "set_sample_rate to the rate the bank has")
    assert sounds_at_once(moved[1])


# ---- (d) the refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [K.REFUSED_LOW, K.REFUSED_HIGH], ids=["14056Hz", "50MHz"])
def test_refused_rates_leave_the_bank_where_it_was(gpu, bad):
    assert not K.make_const(bad)["ok"]
    rest = (0, 64 * 4 + 7)
    x = moved_signal(3, rest[-1] + T1_AB, T1_AB + 2 * rest[-1], 800)
    # first thing (the bank stays at the rate it was created at), and in mid-tail; the oracle is never asked
    script = [("refused", bad), ("render", rest), ("rate", A), ("render", FIRST_AB), ("refused", bad), ("render", rest)]
    renders = play(gpu, "lowpole", 3, script, x)
    assert sounds_at_once(renders[2])


def test_the_lowest_accepted_rate_is_accepted(gpu):
    assert K.make_const(K.ACCEPTED_LOW)["ok"] and K.ACCEPTED_LOW == K.REFUSED_LOW + 1
    b = make_bank(gpu, "lowpole", 2)
    b.set_sample_rate(K.ACCEPTED_LOW)               # (rendered as the first row of the rate table)
    assert b.sample_rate == K.ACCEPTED_LOW
    with pytest.raises(gpu.FdspError, match="14057 Hz"):
        b.set_sample_rate(K.REFUSED_LOW)


# ---- (e) through from_graph ------------------------------------------------------------------------------------------------------------
def test_from_graph_at_22050_hz_equals_the_run_time_compiled_node(gpu):
    sr = 22050.0
    c = K.make_const(sr)
    assert c["cap"] == 1024
    V, T = 4, c["cap"] + 64 * 3 + 13                # one wrap of the 1024-slot ring
    mk = lambda: GR.reverb3_stereo(TIME, DIFFUSION, lambda: GR.lowpole_hz(CUTOFF))
    fast = gpu.Bank.from_graph(mk(), V, sample_rate=sr)
    slow = gpu.Bank.from_graph(mk(), V, ring_frames=2048, sample_rate=sr, fdn_kernel=False)
    assert fast.kind == "reverb3_stereo" and slow.kind.startswith("jit_")
    x = signal(V, T, 61)
    cuts = [0, c["cap"] - 91, c["cap"] - 10, T]
    a = run(fast, x, LAYOUT_VOICE_MINOR, MODE_PROCESS, cuts)
    b = run(slow, x, LAYOUT_VOICE_MINOR, MODE_PROCESS, cuts)
    assert fast.get_option("last_kernel") == 6 and slow.get_option("last_kernel") != 6
    assert_bit_equal(a, b, "lane-per-frame kernel vs run-time compiled lane-per-voice node at 22 050 Hz")
    assert np.abs(a[0][:, c["cap"]:]).max() > SOUNDS
    for v in range(V):
        assert_bit_equal(a[v], oracle_render(make_oracle("lowpole", sr), x[v], cuts, MODE_PROCESS), f"instance {v} at 22 050 Hz")
