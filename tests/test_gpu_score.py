"""Scores (fdsp_bank_set_score): a pool of voices, each playing one note after another, scheduled on the device in one launch.

Note k on voice v must play exactly like a Sequencer event whose unit is a FRESH unit of the bank's graph with voice v's seed and note k's
parameters: every voice's output is compared bit for bit with the oracle's Sequencer (tests/oracle.py, one event per note), and with the
engine's own one-event-per-voice scheduler as a second referee.  Shapes: 70 voices (one full wave and one partial), nine blocks and a
ragged tail, three to six notes per voice; the score (tests/score_cases.py) contains by construction a legato pair, three notes inside
one sequencer block, a note shorter than a SIMD item, a note of exactly one aligned block, one spanning the launch, a voice without
notes, a note after the launch, off-grid times, both fade curves, fades of zero and of the full duration."""
import numpy as np
import pytest

import oracle as O
from fundsp_amd import FADE_POWER, MODE_PROCESS, MODE_TICK
from fundsp_amd import workloads as W
from score_cases import SPLIT, SR, T, V, Score, build_score, pool_output
from test_gpu_config4 import tables  # noqa: F401  (fixture: the oracle's wavetables installed on the device)
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
MODES = [MODE_PROCESS, MODE_TICK]
LK_SCORE = 9
_cache = {}


def fm_note_params(n, seed):
    """Per-note f, m, fc, q in the ranges of W.fm_svf_params"""
    u = np.random.default_rng(seed).random((4, n))
    f = 55.0 * np.exp2(5.0 * u[0])
    return dict(f=f.astype(np.float32), m=(0.5 + 7.5 * u[1]).astype(np.float32),
                fc=np.minimum(f * np.exp2(4.0 * u[2]), 0.45 * SR).astype(np.float32), q=(0.5 + 3.5 * u[3]).astype(np.float32))


def fm_rows(pn):
    S = W.FM_SLOTS
    return {S["f_const"]: pn["f"], S["f_mul"]: pn["f"], S["m_mul"]: pn["m"], S["f_add"]: pn["f"], S["cutoff"]: pn["fc"], S["q"]: pn["q"]}


def fm_case():
    """The score, the voices' own parameters and seeds, the notes' parameters"""
    if "fm" not in _cache:
        sc = build_score(501)
        _cache["fm"] = (sc, W.fm_svf_params(V, SR), fm_note_params(sc.n, 502))
    return _cache["fm"]


def fm_oracle(mode):
    """(expected [V][1][T], the Sequencer's clock afterwards): one event per note, a fresh unit with the note's parameters and the voice's seed"""
    key = ("fm_oracle", mode)
    if key not in _cache:
        sc, p, pn = fm_case()
        seq = O.Sequencer(0, 1, SR)
        for k in range(sc.n):
            f, m = float(pn["f"][k]), float(pn["m"][k])
            n = O.sine_hz(f) * f * m + f >> O.sine() >> O.lowpass_hz(float(pn["fc"][k]), float(pn["q"][k]))
            n.set_seed(int(p["seed"][sc.voice[k]]))
            seq.push(sc.start[k], sc.end[k], int(sc.fade[k]), sc.fin[k], sc.fout[k], n)
        _, per = seq.render(T, process=(mode == MODE_PROCESS))
        want = pool_output(sc, per, V)
        want.setflags(write=False)
        _cache[key] = (want, seq.time())
    return _cache[key]


def fm_bank():
    sc, p, pn = fm_case()
    b = W.make_fm_svf_bank(V, SR, params=p)
    b.set_score(sc.voice, sc.start, sc.end, sc.fin, sc.fout, sc.fade, params=fm_rows(pn))
    return b


def voices_of(out):
    """[outputs][frames][voices] on the device -> [voices][outputs][frames] on the host"""
    return out.cpu().numpy().transpose(2, 0, 1)


@pytest.mark.parametrize("mode", MODES)
def test_fm_score_against_the_oracle(gpu, mode):
    sc, _, _ = fm_case()
    want, clock = fm_oracle(mode)
    b = fm_bank()
    got = voices_of(b.process_events(T, mode=mode))
    assert b.get_option("last_kernel") == LK_SCORE
    for v in range(V):
        assert_bit_equal(got[v], want[v], f"score voice {v}")
    assert b.events_time() == clock
    t = sc.tag
    assert np.any(got[0] != 0) and not np.any(got[4] != 0) and not np.any(got[5] != 0)   # whole launch | no notes | after the launch
    s3 = int(round(sc.start[t["shorter_than_simd_item"]] * SR))
    assert np.all(got[2][0, s3:s3 + 3] != 0) and got[2][0, s3 + 3] == 0 and got[2][0, s3 - 1] == 0


@pytest.mark.parametrize("mode", MODES)
def test_fused_mix_equals_the_sum_of_the_voices(gpu, mode):
    b, b2 = fm_bank(), fm_bank()
    per = b.process_events(T, mode=mode)
    fused = b2.process_events_mix(T, mode=mode)
    assert b2.get_option("last_kernel") == LK_SCORE
    assert_bit_equal(fused.cpu().numpy(), gpu.sum_voices(per).cpu().numpy(), "process_events_mix vs sum_voices(process_events)")
    assert b2.events_time() == b.events_time()
    assert_bit_equal(b2.get_state(), b.get_state(), "voice state after the fused launch")


@pytest.mark.parametrize("mode", MODES)
def test_split_launches_equal_one_launch(gpu, mode):
    """Nothing but the clock carries over: the notes straddling a launch boundary go on with the state they have, the one that starts
    exactly on a boundary starts there"""
    import torch

    want, clock = fm_oracle(mode)
    one = voices_of(fm_bank().process_events(T, mode=mode))
    b = fm_bank()
    got = voices_of(torch.cat([b.process_events(n, mode=mode) for n in SPLIT], dim=1))
    for v in range(V):
        assert_bit_equal(got[v], one[v], f"split launches, voice {v}")
        assert_bit_equal(got[v], want[v], f"split launches vs the oracle, voice {v}")
    assert b.events_time() == clock


def test_waves_inside_their_notes_take_the_packed_path(gpu):
    """Blocks in which every lane of a wave is inside a note it has begun, no fade running, render through the packed two-frame path.  The
    first wave enters that state after its notes' first block, leaves it while its lanes change note one after the other (legato, at
    staggered times, some with fades) and enters it again with the second notes; the partial second wave starts late and off the grid."""
    Vs, Ts = 64 + 20, 64 * 12 + 29
    rng = np.random.default_rng(541)
    p = W.fm_svf_params(Vs, SR)
    change = rng.integers(64 * 4, 64 * 6, 64).astype(np.float64) + np.where(np.arange(64) % 3 == 0, 0.2, 0.0)
    voice = np.concatenate([np.arange(64), np.arange(64), np.arange(64, Vs)])
    start = np.concatenate([np.zeros(64), change, np.full(Vs - 64, 100.3)]) / SR
    end = np.concatenate([change / SR, np.full(64, (Ts + 50.0) / SR), np.full(Vs - 64, (Ts + 50.0) / SR)])
    end[:64] = start[64:128]                                          # legato: the same bits
    fin = np.concatenate([np.zeros(64), np.where(np.arange(64) % 4 == 0, 30.0, 0.0), np.zeros(Vs - 64)]) / SR
    fout = np.concatenate([np.where(np.arange(64) % 5 == 0, 50.0, 0.0), np.zeros(Vs)]) / SR
    fade = (np.arange(voice.size) % 2).astype(np.int32)
    pn = fm_note_params(voice.size, 542)
    b = W.make_fm_svf_bank(Vs, SR, params=p)
    b.set_score(voice, start, end, fin, fout, fade, params=fm_rows(pn))
    got = voices_of(b.process_events(Ts))
    seq = O.Sequencer(0, 1, SR)
    for k in range(voice.size):
        f, m = float(pn["f"][k]), float(pn["m"][k])
        n = O.sine_hz(f) * f * m + f >> O.sine() >> O.lowpass_hz(float(pn["fc"][k]), float(pn["q"][k]))
        n.set_seed(int(p["seed"][voice[k]]))
        seq.push(start[k], end[k], int(fade[k]), fin[k], fout[k], n)
    _, per = seq.render(Ts, process=True)
    want = pool_output(Score(voice, start, end, fin, fout, fade, {}), per, Vs)
    for v in range(Vs):
        assert_bit_equal(got[v], want[v], f"sustained score voice {v}")
    assert b.events_time() == seq.time()


@pytest.mark.parametrize("mode", MODES)
def test_one_event_per_voice_scheduler_as_referee(gpu, mode):
    """No oracle: the same N notes as N one-event voices through set_events on a fresh bank, parameters by set_param, seeds the owning
    score voices'"""
    sc, p, pn = fm_case()
    ref = gpu.Bank("fm_svf", sc.n)
    for name, values in fm_rows(pn).items():
        ref.set_param(name, values)
    ref.set_sample_rate(SR)
    ref.set_seed(p["seed"][sc.voice])
    ref.set_events(sc.start, sc.end, sc.fin, sc.fout, sc.fade)
    per = voices_of(ref.process_events(T, mode=mode))
    want = pool_output(sc, per, V)
    got = voices_of(fm_bank().process_events(T, mode=mode))
    for v in range(V):
        assert_bit_equal(got[v], want[v], f"score voice {v} vs its notes as one-event voices")


@pytest.mark.parametrize("mode", MODES)
def test_one_note_per_voice_without_rows_equals_set_events(gpu, mode):
    rng = np.random.default_rng(503)
    p = W.fm_svf_params(V, SR)
    start = (rng.integers(0, T // 2, V) + rng.random(V) * 0.4 - 0.2).clip(0) / SR
    end = start + rng.integers(40, T, V) / SR
    fin, fout = rng.integers(0, 40, V) / SR, rng.integers(0, 40, V) / SR
    fade = rng.integers(0, 2, V).astype(np.int32)
    a, b = W.make_fm_svf_bank(V, SR, params=p), W.make_fm_svf_bank(V, SR, params=p)
    a.set_events(start, end, fin, fout, fade)
    order = rng.permutation(V)                                      # unsorted input is accepted
    b.set_score(order, start[order], end[order], fin[order], fout[order], fade[order])
    assert_bit_equal(b.process_events(T, mode=mode).cpu().numpy(), a.process_events(T, mode=mode).cpu().numpy(), "score of one note per voice vs events")
    assert b.events_time() == a.events_time()


@pytest.mark.parametrize("mode", MODES)
def test_run_time_compiled_graph_with_hash_and_ring(gpu, mode):
    """noise() >> lowpass_hz(fc, 1) >> (pass() & delay(0.002)), cutoff per note: every note restarts the noise sequence and starts from an
    empty delay ring, like the oracle's fresh units"""
    from fundsp_amd import graph as GR

    Vj = 70
    sc = build_score(511, voices=Vj)
    rng = np.random.default_rng(512)
    fc = (300.0 * np.exp2(5.0 * rng.random(sc.n))).astype(np.float32)
    seeds = np.arange(Vj, dtype=np.uint64) * 7 + 3
    g = GR.noise() >> GR.lowpass_hz(1000.0, 1.0) >> (GR.pass_() & GR.delay(0.002))
    cutoff = [n for n, _, _ in g.slot_values() if n.endswith(":cutoff")]
    assert len(cutoff) == 1
    b = gpu.Bank.from_graph(g, Vj, ring_frames=128, sample_rate=SR)
    b.set_seed(seeds)
    b.set_score(sc.voice, sc.start, sc.end, sc.fin, sc.fout, sc.fade, params={cutoff[0]: fc})
    got = voices_of(b.process_events(T, mode=mode))
    assert b.get_option("last_kernel") == LK_SCORE
    seq = O.Sequencer(0, 1, SR)
    for k in range(sc.n):
        n = O.noise() >> O.lowpass_hz(float(fc[k]), 1.0) >> (O.pass_() & O.delay(0.002))
        n.set_seed(int(seeds[sc.voice[k]]))
        seq.push(sc.start[k], sc.end[k], int(sc.fade[k]), sc.fin[k], sc.fout[k], n)
    _, per = seq.render(T, process=(mode == MODE_PROCESS))
    want = pool_output(sc, per, Vj)
    for v in range(Vj):
        assert_bit_equal(got[v], want[v], f"compiled graph, score voice {v}")
    assert b.events_time() == seq.time()
    # ... and the Sequencer's output in one launch
    b2 = gpu.Bank.from_graph(g, Vj, ring_frames=128, sample_rate=SR)
    b2.set_seed(seeds)
    b2.set_score(sc.voice, sc.start, sc.end, sc.fin, sc.fout, sc.fade, params={cutoff[0]: fc})
    import torch

    fused = b2.process_events_mix(T, mode=mode).cpu().numpy()
    summed = gpu.sum_voices(torch.from_numpy(np.ascontiguousarray(got.transpose(1, 2, 0))).cuda()).cpu().numpy()
    assert_bit_equal(fused, summed, "compiled graph: fused score mix vs sum_voices")


def test_kind_with_an_input_in_two_launches(gpu):
    """A kind with an input (lowpass >> tanh shaper >> highpass over a per-voice noise stream), both filters' cutoff and q per note, two
    launches; spot voices against the oracle.  (The many-note score runs on this kind and not on saw_moog_adsr_pan because adsr_live
    keeps its gate memory across reset() in the reference itself: tests/test_score_host.py.)"""
    import torch

    Vg, T1 = 64 + 6, 64 * 4
    sc = build_score(521, voices=Vg)
    rng = np.random.default_rng(522)
    rows = {"0.0:cutoff": (200.0 * np.exp2(5.0 * rng.random(sc.n))).astype(np.float32), "0.0:q": (0.5 + 3.0 * rng.random(sc.n)).astype(np.float32),
            "1:cutoff": (50.0 * np.exp2(4.0 * rng.random(sc.n))).astype(np.float32), "1:q": (0.5 + rng.random(sc.n)).astype(np.float32)}
    b = gpu.Bank("svf_shape_svf", Vg)
    for name, value in (("0.0:mode", O.SVF_MODES["lowpass"]), ("1:mode", O.SVF_MODES["highpass"]), ("0.1:shape", O.SHAPES["tanh"]), ("0.1:shape_p0", 1.0)):
        b.set_param(name, np.full(Vg, float(value), dtype=np.float32))
    b.set_sample_rate(SR)
    b.set_score(sc.voice, sc.start, sc.end, sc.fin, sc.fout, sc.fade, params=rows)
    x = (rng.random((Vg, 1, T), dtype=np.float32) * 2 - 1).astype(np.float32)
    d = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0))).cuda()
    got = voices_of(torch.cat([b.process_events(T1, d[:, :T1].contiguous()), b.process_events(T - T1, d[:, T1:].contiguous())], dim=1))
    spot = sorted(set(range(0, Vg, 5)) | {1, 2, 6, 7, 8})
    notes = np.flatnonzero(np.isin(sc.voice, spot))
    seq = O.Sequencer(1, 1, SR)
    for k in notes:
        n = O.lowpass_hz(float(rows["0.0:cutoff"][k]), float(rows["0.0:q"][k])) >> O.shape("tanh", 1.0, 0.0) >> \
            O.highpass_hz(float(rows["1:cutoff"][k]), float(rows["1:q"][k]))
        seq.push(sc.start[k], sc.end[k], int(sc.fade[k]), sc.fin[k], sc.fout[k], n)
    _, per = seq.render(T, True, inputs=x[sc.voice[notes]])
    full = np.zeros((sc.n, 1, T), dtype=np.float32)
    full[notes] = per
    want = pool_output(sc, full, Vg)
    for v in spot:
        assert_bit_equal(got[v], want[v], f"score voice {v} of a kind with an input")
    assert np.abs(got).max() > 0.01


def test_gated_voices_one_note_each_in_two_launches(gpu, tables):
    """saw >> moog * adsr_live >> pan with a gate stream, f / fc / q / pan per note, two launches, stereo out: one note per voice -- the
    first note a unit plays is where reset() and a fresh unit agree for adsr_live -- in shuffled order; spot voices against the oracle"""
    import torch
    from test_gpu_config4 import config4_oracle_voice

    Vg, T1 = 64 + 6, 64 * 4
    rng = np.random.default_rng(531)
    start = (rng.integers(0, T // 2, Vg) + rng.random(Vg) * 0.4 - 0.2).clip(0) / SR
    end = start + rng.integers(3, T, Vg) / SR
    fin, fout = np.minimum(rng.integers(0, 40, Vg) / SR, end - start), np.minimum(rng.integers(0, 40, Vg) / SR, end - start)
    fade = rng.integers(0, 2, Vg).astype(np.int32)
    pv, pn = W.saw_moog_params(Vg, SR), W.saw_moog_params(Vg, SR, voice0=1000)
    adsr = (0.005, 0.01, 0.6, 0.01)
    b = W.make_saw_moog_bank(Vg, SR, params=pv, adsr=adsr)
    order = rng.permutation(Vg)
    b.set_score(order, start[order], end[order], fin[order], fout[order], fade[order], params={W.C4_SLOTS[k]: pn[k][order] for k in ("f", "fc", "q", "pan")})
    gate = np.zeros((Vg, 1, T), dtype=np.float32)
    for v in range(Vg):
        gate[v, 0] = ((np.arange(T) + 11 * v) % 97) >= 9            # low -> high every 97 frames: adsr_live attacks inside the notes
    g = torch.from_numpy(np.ascontiguousarray(gate.transpose(1, 2, 0))).cuda()
    got = voices_of(torch.cat([b.process_events(T1, g[:, :T1].contiguous()), b.process_events(T - T1, g[:, T1:].contiguous())], dim=1))
    spot = list(range(0, Vg, 5))
    seq = O.Sequencer(1, 2, SR)
    for v in spot:
        pk = {key: pn[key] for key in ("f", "fc", "q", "pan")}
        pk["seed"] = pv["seed"]
        seq.push(start[v], end[v], int(fade[v]), fin[v], fout[v], config4_oracle_voice(pk, v, adsr))
    _, per = seq.render(T, True, inputs=gate[spot])
    for i, v in enumerate(spot):
        assert_bit_equal(got[v], per[i], f"gated score voice {v}")
    assert np.abs(got).max() > 0.01


def test_refusals_leave_the_bank_as_it_was(gpu):
    sc, p, pn = fm_case()
    want, _ = fm_oracle(MODE_PROCESS)
    b = fm_bank()
    E = gpu.FdspError
    EINVAL = gpu._lib.EINVAL

    def refused(match, voice, start, end, **kw):
        with pytest.raises(E, match=match) as e:
            b.set_score(voice, start, end, **kw)
        assert e.value.code == EINVAL

    refused(r"note 2 overlaps note 0 on voice 3", [3, 1, 3], [0.0, 0.0, 0.009], [0.01, 0.01, 0.02])
    refused(rf"note 1: voice {V} is out of range", [0, V], [0.0, 0.0], [0.01, 0.01])
    refused(r"note 1: fade times", [0, 1], [0.0, 0.0], [0.01, 0.01], fade_in=[0.0, 0.02])
    refused(r"unknown slot: 1:nope", [0], [0.0], [0.01], params={"1:nope": [1.0]})
    refused(r"slot '1:ic1eq' is no f32 parameter", [0], [0.0], [0.01], params={"1:ic1eq": [1.0]})
    with pytest.raises(E, match="0 to 16 slots") as e:
        gpu._lib.check(gpu.lib().fdsp_bank_set_score(b._h, 0, None, None, None, 17, None, None))
    assert e.value.code == EINVAL
    # the bank still holds the score it had, untouched
    got = voices_of(b.process_events(T))
    for v in range(V):
        assert_bit_equal(got[v], want[v], f"after the refusals, voice {v}")


def test_effect_banks_play_no_scores(gpu):
    import ctypes as C

    L = gpu.lib()
    h = C.c_void_p()
    gpu._lib.check(L.fdsp_reverb_stereo_create(2, 10.0, 1.0, 0.5, C.byref(h)))
    try:
        voice, ev = (C.c_int * 1)(0), (C.c_double * 4)(0.0, 0.01, 0.0, 0.0)
        assert L.fdsp_bank_set_score(h, 1, voice, ev, None, 0, None, None) == gpu._lib.EINVAL
        assert b"effect banks" in L.fdsp_last_error()
    finally:
        L.fdsp_bank_destroy(h)


def test_events_after_a_score_and_clones(gpu):
    sc, p, _ = fm_case()
    want, clock = fm_oracle(MODE_PROCESS)
    b = fm_bank()
    c = b.clone()                                                   # a clone plays the score
    got = voices_of(c.process_events(T))
    for v in range(V):
        assert_bit_equal(got[v], want[v], f"clone, voice {v}")
    assert c.events_time() == clock
    # set_events afterwards removes the score: the bank plays the events, like a bank that never had one
    start, end = np.arange(V) * 3.0 / SR, (np.arange(V) * 3.0 + 200.0) / SR
    b.set_events(start, end, 10.0 / SR, 0.0, FADE_POWER)
    ref = W.make_fm_svf_bank(V, SR, params=p)
    ref.set_events(start, end, 10.0 / SR, 0.0, FADE_POWER)
    assert_bit_equal(b.process_events(T).cpu().numpy(), ref.process_events(T).cpu().numpy(), "events after a score")
    assert b.get_option("last_kernel") != LK_SCORE
    # ... and an empty score removes everything the scheduler had
    b.set_score([], [], [])
    with pytest.raises(gpu.FdspError):
        b.process_events(64)
