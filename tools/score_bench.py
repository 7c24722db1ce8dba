"""Scores (fdsp_bank_set_score) against the only way to render notes without them -- one voice per note through fdsp_bank_set_events --
and what the note-switch code costs a sustained launch.  Run on the GPU box:

    python tools/score_bench.py --out profiles/score_bench.json
    FUNDSP_HIP_LIB=<an older build's libfundsp_hip.so> python tools/score_bench.py --skip-score --out <file>    # the events legs alone
    FUNDSP_HIP_LIB=<the parent commit's library> python tools/score_bench.py --skip-notes --out parent.json       # the serial legs of a build
    python tools/score_bench.py --serial-from parent.json --out profiles/score_bench.json                        #   without "score_exec", carried along

Method: the FM + SVF kind (BASELINE config 3), fdsp_bank_process_events_mix, the launch's own HIP event pair (fdsp_bank_last_kernel_ms:
kernel plus the partial-mix tree), one warm-up launch, then 20 timed launches -- median, min and max -- with the clock rewound before each.

Notes: 64 lanes of back-to-back notes over 96 000 frames (2 s at 48 kHz), 60 .. 300 frames each (1.25 .. 6.25 ms), gaps of 0 .. 20 frames,
16-frame fades, f / m / fc / q per note: about 32 000 notes, at most 64 sounding at once.  The same notes are played
  (a) as a score on pools of 64, 1 024 and 8 192 voices (fundsp_amd.score.assign_voices allots them: the lowest free voice, so the
      larger pools play on the same 64 voices and their other waves idle), and
  (b) as one voice per note: a bank of N voices with fdsp_bank_set_events, every lane walking all 96 000 frames.
  N x T = 3.1 G voice-frames and a 194 MB partial-mix buffer for (b): fits any MI355X and keeps the 21 launches well under a minute.
Sustained: 65 536 voices x 12 000 frames, one note per voice covering the launch.  As events the launch is sustained and
fdsp_bank_process_events_mix hands it to the pipeline render kernel; `events_kernel` is the same bank with ONE voice fading through the
launch, which keeps it in the scheduler kernel (that one wave goes frame by frame) -- the like-for-like partner of the score kernel,
which has no such shortcut and whose first block runs frame by frame (every note begins there).
Note path ("score_exec" = SCORE_NOTES, key "score_notes"): score (a) on pools of 64 and 8 192 voices (the second renders through the
chunked scratch: 8 192 frames per chunk) and the sustained score, same method, same run; before anything is timed the [1][96 000] mix of
the two executors is compared bit for bit.  `spread_ms` = max - min of the serial leg: the note path counts as faster only beyond it."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fundsp_amd as F  # noqa: E402
from fundsp_amd import workloads as W  # noqa: E402

SR = 48000.0
LANES, T_NOTES = 64, 96000
V_SUS, T_SUS = 65536, 12000
FADE = 16
REPS = 20


def make_notes(seed=1):
    rng = np.random.default_rng(seed)
    start, end = [], []
    for _ in range(LANES):
        t = int(rng.integers(0, 200))
        while True:
            n = int(rng.integers(60, 301))
            if t + n > T_NOTES:
                break
            start.append(t)
            end.append(t + n)
            t += n + int(rng.integers(0, 21))
    start, end = np.array(start, dtype=np.float64), np.array(end, dtype=np.float64)
    u = rng.random((4, start.size))
    f = 55.0 * np.exp2(5.0 * u[0])
    rows = dict(f=f.astype(np.float32), m=(0.5 + 7.5 * u[1]).astype(np.float32), fc=np.minimum(f * np.exp2(4.0 * u[2]), 0.45 * SR).astype(np.float32),
                q=(0.5 + 3.5 * u[3]).astype(np.float32))
    return start, end, rows


def fm_rows(rows):
    S = W.FM_SLOTS
    return {S["f_const"]: rows["f"], S["f_mul"]: rows["f"], S["m_mul"]: rows["m"], S["f_add"]: rows["f"], S["cutoff"]: rows["fc"], S["q"]: rows["q"]}


def timed(bank, frames, out):
    def once():
        bank.events_rewind(0.0)
        bank.process_events_mix(frames, out=out)
        torch.cuda.synchronize()
        return bank.last_kernel_ms()

    once()
    ms = sorted(once() for _ in range(REPS))
    return dict(median_ms=float(np.median(ms)), min_ms=ms[0], max_ms=ms[-1], last_kernel=bank.get_option("last_kernel"))


def packed_share(voice, start, end, pool):
    """Share of (wave, block) pairs of the launch that take the packed path: every lane of the wave inside a note it has begun for the whole
    block, no fade running -- the kernel's own conditions, counted here on the sample grid"""
    blocks = T_NOTES // 64
    steady = np.zeros((pool, blocks), dtype=bool)
    first = np.ceil((start + FADE) / 64.0).astype(np.int64)          # first block that starts at or after the end of the fade-in
    first = np.maximum(first, np.floor(start / 64.0).astype(np.int64) + 1)
    last = np.floor((end - FADE) / 64.0).astype(np.int64)             # blocks [first, last) end before the fade-out begins
    for v, a, b in zip(voice, first, last):
        if b > a:
            steady[v, a:b] = True
    waves = -(-pool // 64)
    pad = np.zeros((waves * 64, blocks), dtype=bool)
    pad[:pool] = steady
    return float(pad.reshape(waves, 64, blocks).all(axis=1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-score", action="store_true", help="the events legs alone (a library without fdsp_bank_set_score)")
    ap.add_argument("--skip-notes", action="store_true", help="no note-path legs (a library without the score_exec option)")
    ap.add_argument("--serial-from", default=None, help="a result file of an earlier build (--skip-notes), kept under score_notes.serial_of_other_build")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "score_bench needs a HIP device"
    from fundsp_amd.score import assign_voices

    res = dict(method=f"fm_svf, process_events_mix, HIP event pair of the launch, 1 warm-up + {REPS} launches: median / min / max", sample_rate=SR)
    start, end, rows = make_notes()
    n = start.size
    res["notes"] = dict(count=int(n), frames=T_NOTES, lanes=LANES, mean_length_frames=float((end - start).mean()), fade_frames=FADE)
    mix = torch.empty((1, T_NOTES), dtype=torch.float32, device="cuda")
    if not a.skip_score:
        res["score"] = {}
        for pool in (64, 1024, 8192):
            voice = assign_voices(start, end, pool)
            b = W.make_fm_svf_bank(pool, SR)
            b.set_score(voice, start / SR, end / SR, FADE / SR, FADE / SR, F.FADE_SMOOTH, params=fm_rows(rows))
            r = timed(b, T_NOTES, mix)
            r.update(voices_used=int(voice.max()) + 1, packed_share_of_wave_blocks=packed_share(voice, start, end, pool))
            res["score"][str(pool)] = r
            print("score", pool, r, flush=True)
            del b
    if not a.skip_score and not a.skip_notes:
        nt = res["score_notes"] = {}
        for pool in (64, 8192):
            voice = assign_voices(start, end, pool)
            b = W.make_fm_svf_bank(pool, SR)
            b.set_score(voice, start / SR, end / SR, FADE / SR, FADE / SR, F.FADE_SMOOTH, params=fm_rows(rows))
            if pool == 64:                                             # the two executors at the bench's own size, before anything is timed
                want = b.clone().process_events_mix(T_NOTES).cpu().numpy()
                c = b.clone()
                c.set_option("score_exec", F.SCORE_NOTES)
                got = c.process_events_mix(T_NOTES).cpu().numpy()
                nt["mix_bit_equal_to_serial"] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
                assert nt["mix_bit_equal_to_serial"], "score_exec 1 and 0 differ at the bench's size"
                del c
            b.set_option("score_exec", F.SCORE_NOTES)
            b.mix_reserve(T_NOTES)
            r = timed(b, T_NOTES, mix)
            serial = res["score"][str(pool)]
            r.update(chunk_frames=b.get_option("score_scratch_frames"), serial_median_ms=serial["median_ms"], serial_spread_ms=serial["max_ms"] - serial["min_ms"],
                     speedup=serial["median_ms"] / r["median_ms"])
            nt[str(pool)] = r
            print("score, one lane per note", pool, r, flush=True)
            del b
    b = F.Bank("fm_svf", n)                                            # (b) one voice per note
    for name, values in fm_rows(rows).items():
        b.set_param(name, values)
    b.set_sample_rate(SR)
    b.set_seed(np.arange(n, dtype=np.uint64))
    b.set_events(start / SR, end / SR, FADE / SR, FADE / SR, F.FADE_SMOOTH)
    res["one_voice_per_note"] = timed(b, T_NOTES, mix)
    print("one voice per note", res["one_voice_per_note"], flush=True)
    del b
    # sustained: one note per voice covering the launch
    mix = torch.empty((1, T_SUS), dtype=torch.float32, device="cuda")
    res["sustained"] = dict(voices=V_SUS, frames=T_SUS)
    b = W.make_fm_svf_bank(V_SUS, SR)
    b.set_events(np.full(V_SUS, -1.0), np.full(V_SUS, 10.0))
    res["sustained"]["events"] = timed(b, T_SUS, mix)                   # the shortcut to the render kernel
    fin = np.zeros(V_SUS)
    fin[0] = 5.0
    b.set_events(np.full(V_SUS, -1.0), np.full(V_SUS, 10.0), fade_in=fin)
    res["sustained"]["events_kernel"] = timed(b, T_SUS, mix)            # held in the scheduler kernel by one fading voice
    if not a.skip_score:
        b.set_score(np.arange(V_SUS), np.full(V_SUS, 0.0), np.full(V_SUS, 10.0))
        res["sustained"]["score"] = timed(b, T_SUS, mix)
        if not a.skip_notes:                                            # one note per voice: nothing to parallelise, and the voice-out scratch to fill
            b.set_option("score_exec", F.SCORE_NOTES)
            b.mix_reserve(T_SUS)
            res["score_notes"]["sustained"] = timed(b, T_SUS, mix)
            res["score_notes"]["sustained"]["chunk_frames"] = b.get_option("score_scratch_frames")
    print("sustained", res["sustained"], flush=True)
    if "score_notes" in res:
        res["score_notes"]["one_voice_per_note_median_ms"] = res["one_voice_per_note"]["median_ms"]
        if a.serial_from:
            with open(a.serial_from) as fh:
                other = json.load(fh)
            res["score_notes"]["serial_of_other_build"] = dict(score=other.get("score"), one_voice_per_note=other.get("one_voice_per_note"),
                                                               sustained=other.get("sustained"))
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
