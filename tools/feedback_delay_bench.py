"""Feedback delay banks (Bank.feedback_tree, the lane-per-frame kernel k_fb_frames) against the run-time compiled rendering of the same graph
(Bank.from_graph, one lane per voice), both in one process: 2 048 instances x 48 000 frames at 48 kHz, device events around every launch
on one stream, one warm-up, the median of 20 launches with their minimum and maximum.  Four rows:

    echo            feedback(delay(0.5) * 0.5)
    ping_pong       feedback((delay(0.5) | delay(0.5)) >> reverse() * db_amp(-6.0))
    comb_lowpole    feedback2(delay(0.01), lowpole_hz(2000.0) * 0.9)
    echo_per_voice  feedback(delay(t_v) * 0.5), t_v = 0.25 .. 0.5 s over the instances

Both layouts are measured (planar is the lane-per-frame kernels' native one, voice-minor the compiled kernels').  A row passes when the new
bank's median lies below the compiled route's MINIMUM in that layout.  Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import fundsp_amd as F  # noqa: E402
from fundsp_amd import graph as G  # noqa: E402

SR = 48000.0


def graphs(V):
    tv = np.linspace(0.25, 0.5, V, dtype=np.float32)
    return {
        "echo": G.feedback(G.delay(0.5) * 0.5),
        "ping_pong": G.feedback((G.delay(0.5) | G.delay(0.5)) >> G.reverse(2) * G._db_amp(-6.0)),
        "comb_lowpole": G.feedback2(G.delay(0.01), G.lowpole_hz(2000.0) * 0.9),
        "echo_per_voice": G.feedback(G.delay(tv) * 0.5),
    }


def event_ms(bank, x, y, frames, layout, reps, stream):
    """device time of `reps` launches after one warm-up, each between two events on `stream`"""
    import torch

    kw = dict(layout=layout, stream=stream.cuda_stream)
    if layout == F.LAYOUT_PLANAR:
        kw["frame_stride"] = frames
    ms = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        bank.process(frames, x, y, **kw)
        b.record(stream)
        b.synchronize()
        if r > 0:
            ms.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def row(name, g, V, T, reps, stream, layouts):
    import torch

    fast = F.Bank.feedback_tree(g, V, sample_rate=SR)
    slow = F.Bank.from_graph(g, V, sample_rate=SR)
    assert fast.kind == "feedback_delay" and slow.kind.startswith("jit_"), (fast.kind, slow.kind)
    n = g.nin
    out = dict(row=name, channels=n, instances=V, frames=T)
    for layout, lname in layouts:
        shape = (V, n, T) if layout == F.LAYOUT_PLANAR else (n, T, V)
        with torch.cuda.stream(stream):
            x = torch.rand(shape, dtype=torch.float32, device="cuda") * 2 - 1
            y = torch.empty(shape, dtype=torch.float32, device="cuda")
        stream.synchronize()
        a = event_ms(fast, x, y, T, layout, reps, stream)
        b = event_ms(slow, x, y, T, layout, reps, stream)
        out[lname] = dict(feedback_delay=a, compiled=b, speedup_median=round(b["median_ms"] / a["median_ms"], 1),
                          passes=bool(a["median_ms"] < b["min_ms"]))
        del x, y
    fast.close()
    slow.close()
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="echo,ping_pong,comb_lowpole,echo_per_voice")
    ap.add_argument("--layouts", default="planar,voice_minor")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    layouts = [(F.LAYOUT_PLANAR if k == "planar" else F.LAYOUT_VOICE_MINOR, k) for k in a.layouts.split(",")]
    stream = torch.cuda.Stream()
    gs = graphs(a.instances)
    rows = [row(k, gs[k], a.instances, a.frames, a.reps, stream, layouts) for k in a.rows.split(",")]
    line = json.dumps(dict(tool="feedback_delay_bench", sample_rate=SR, reps=a.reps, timing="device events, one warm-up, median of reps with min - max",
                           acceptance="feedback_delay median < compiled min", rows=rows))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
