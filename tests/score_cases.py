"""Scores for tests/test_gpu_score.py and the CPU tests: a random score that contains, by construction, every case the score kernels
treat differently, and the expected output of a voice pool built from per-event outputs (the oracle's Sequencer, or the engine's own
one-event-per-voice scheduler).  numpy only."""
import numpy as np

SR = 48000.0
V, T = 70, 64 * 9 + 21              # one full wave and one partial; nine blocks and a ragged tail
SPLIT = (64 * 5, 64 * 4, 21)        # the same frames in three launches


class Score:
    """voice, start, end, fade_in, fade_out (seconds), fade per note; `tag` names the notes placed by construction"""

    def __init__(self, voice, start, end, fin, fout, fade, tag):
        self.voice = np.asarray(voice, dtype=np.int32)
        self.start, self.end = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
        self.fin, self.fout = np.asarray(fin, dtype=np.float64), np.asarray(fout, dtype=np.float64)
        self.fade = np.asarray(fade, dtype=np.int32)
        self.tag = tag
        self.n = self.voice.size


def build_score(seed, voices=V, frames=T):
    """Times are made in SAMPLES and divided by SR at the end; a legato successor takes its predecessor's end bit for bit."""
    rng = np.random.default_rng(seed)
    rows, tag = [], {}      # (voice, start, dur, fin, fout, fade, legato_with_previous)

    def note(name, voice, start, dur, fin=0.0, fout=0.0, fade=1, legato=False):
        if name:
            tag[name] = len(rows)
        rows.append((voice, float(start), float(dur), float(fin), float(fout), int(fade), legato))

    note("whole_launch", 0, 0.0, frames + 100)                     # spans the whole launch (and is sustained from block 1 on)
    note("legato_a", 1, 10.0, 50.0, fout=20.0, fade=0)
    note("legato_b", 1, 60.0, 80.0, fin=8.0, legato=True)          # end == start
    note("in_block_a", 2, 64 + 2.0, 5.0)                            # three notes inside one sequencer block
    note("shorter_than_simd_item", 2, 64 + 10.0, 3.0)
    note("in_block_c", 2, 64 + 20.0, 20.0, fin=20.0, fade=0)       # ... the last one fading in over its whole length
    note("one_aligned_block", 3, 128.0, 64.0)
    # voice 4: no notes
    note("after_the_launch", 5, frames + 10.0, 50.0)
    note("straddles_split_1", 6, SPLIT[0] - 20.0, 40.0, fin=30.0)                    # must not restart at the launch boundary
    note("straddles_split_2", 6, SPLIT[0] + SPLIT[1] - 16.0, 30.0, fout=30.0, fade=0)
    note("starts_on_split", 7, float(SPLIT[0]), 100.0)                                # begins exactly on a boundary
    note("full_fade_in", 8, 30.0, 90.0, fin=90.0, fade=1)
    note("full_fade_out", 8, 130.0, 70.0, fout=70.0, fade=0)
    note("both_full_fades", 8, 200.3, 150.0, fin=150.0, fout=150.0)
    for v in range(9, voices):
        n = int(rng.integers(3, 7))
        t = float(rng.integers(0, 40))
        for k in range(n):
            r = rng.random()
            dur = float(rng.integers(3, 21)) if r < 0.4 else float(rng.integers(21, 200))
            legato = k > 0 and rng.random() < 0.25
            if not legato:
                t += float(rng.integers(1, 60)) if k else 0.0
            off = (rng.random() * 0.4 - 0.2) if rng.random() < 0.6 else 0.0       # off the sample grid by up to 0.2 sample
            q = rng.random(2)
            fin = 0.0 if q[0] < 0.3 else (dur if q[0] < 0.45 else float(rng.integers(0, int(dur))))
            fout = 0.0 if q[1] < 0.3 else (dur if q[1] < 0.45 else float(rng.integers(0, int(dur))))
            note(None, v, max(t + off, 0.0), dur, fin, fout, int(rng.integers(0, 2)), legato)
            t += dur + 1.0                                                       # (a gap of at least 0.6 sample after the offsets)
    voice = np.array([r[0] for r in rows], dtype=np.int32)
    start = np.array([r[1] for r in rows]) / SR
    end = np.array([r[1] + r[2] for r in rows]) / SR
    for i, r in enumerate(rows):
        if r[6]:
            assert voice[i - 1] == voice[i]
            start[i] = end[i - 1]                                                 # legato: the same bits
            end[i] = start[i] + r[2] / SR
    dur = end - start
    fin = np.minimum(np.array([r[3] for r in rows]) / SR, dur)
    fout = np.minimum(np.array([r[4] for r in rows]) / SR, dur)
    for i, r in enumerate(rows):                                                  # "the full duration" means exactly the duration
        if r[3] == r[2]:
            fin[i] = dur[i]
        if r[4] == r[2]:
            fout[i] = dur[i]
    fade = np.array([r[5] for r in rows], dtype=np.int32)
    sc = Score(voice, start, end, fin, fout, fade, tag)
    check_score(sc, voices)
    return sc


def check_score(sc, voices):
    """The overlap rule of fdsp_bank_set_score, and that the cases promised by construction are in the score"""
    assert sc.voice.min() >= 0 and sc.voice.max() < voices
    for v in range(voices):
        i = np.flatnonzero(sc.voice == v)
        i = i[np.argsort(sc.start[i], kind="stable")]
        assert np.all(sc.end[i][:-1] <= sc.start[i][1:]), f"voice {v} overlaps"
    assert np.all(sc.fin <= sc.end - sc.start) and np.all(sc.fout <= sc.end - sc.start)
    t = sc.tag
    if t:
        assert sc.end[t["legato_a"]] == sc.start[t["legato_b"]]
        assert not np.any(sc.voice == 4)
        assert {0, 1} <= set(sc.fade.tolist())
        assert np.any(sc.fin == 0) and np.any(sc.fin == sc.end - sc.start) and np.any(sc.fout == sc.end - sc.start)
        assert np.any(np.abs(sc.start * SR - np.round(sc.start * SR)) > 0.05)


def pool_output(sc, per, voices):
    """per [notes][outputs][frames] = every note's own contribution -> [voices][outputs][frames]: a voice starts as +0.0 and takes its
    notes' samples wherever their bits differ from +0.0 (the windows are disjoint)"""
    per = np.ascontiguousarray(per, dtype=np.float32)
    out = np.zeros((voices,) + per.shape[1:], dtype=np.float32)
    ob, pb = out.view(np.uint32), per.view(np.uint32)
    hits = np.zeros(out.shape, dtype=np.int32)
    for k in range(sc.n):
        m = pb[k] != 0
        hits[sc.voice[k]] += m
        ob[sc.voice[k]][m] = pb[k][m]
    assert hits.max() <= 1, "two notes of one voice sound in the same frame"
    return out
