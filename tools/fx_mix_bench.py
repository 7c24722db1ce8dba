"""The mix step of the effect banks, fused against unfused, in one run on one card: 2 048 instances x 48 000 frames of

    reverb_stereo(10, 1, 0.5)  |  reverb3_stereo(2.0, 0.6, lowpole 1 800 Hz)  |  the 16-line generic fdn of the prelude example

in both layouts.  Unfused voice-minor = process + sum_voices, unfused planar = process + sum_instances (the code as it was before the
fused call existed), fused = process_mix in the layout.  Device events around the calls, one warm-up, then the median of `--reps` (20)
with min and max.  `--sweep` also times the fused calls with the scratch chunk a 16 / 64 / 256 MiB budget gives.  Prints one JSON line.

Bytes per instance-frame beside the render's own ring traffic, c = 4 * channels (stereo in and out: ci = co = 8):
    unfused voice-minor  transpose in 2 ci, render ci + co, transpose out 2 co, sum_voices co         = 3 ci + 4 co
    fused voice-minor    transpose in 2 ci, render ci + co, partials read co                          = 3 ci + 2 co
    unfused planar       render ci + co, sum_instances co                                             = ci + 2 co
    fused planar         render ci + co, partials read co (a launch beyond one chunk: + 2 ci, the chunk's input rows move over)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import fundsp_amd as F  # noqa: E402


def delays(n):
    return [float(np.float32(0.010 + 0.020 * ((i * 0.6180339887) % 1.0))) for i in range(n)]


def timed(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def case(name, make, V, T, reps, sweep):
    import torch

    b = make()
    b.set_sample_rate(48000.0)
    b.set_option("timing", 0)
    ni, no = b.inputs(), b.outputs()
    ci, co = 4 * ni, 4 * no
    row = dict(case=name, instances=V, frames=T, inputs=ni, outputs=no)
    auto_chunk = max(64, min(1 << 21, (256 << 20) // (V * (ni + no) * 4) // 64 * 64))   # the library's automatic chunk (fd_fxbank.hip)
    s = torch.cuda.current_stream().cuda_stream
    mix = torch.empty((no, T), dtype=torch.float32, device="cuda")
    for layout, lname in ((F.LAYOUT_VOICE_MINOR, "voice_minor"), (F.LAYOUT_PLANAR, "planar")):
        vm = layout == F.LAYOUT_VOICE_MINOR
        x = torch.rand((ni, T, V) if vm else (V, ni, T), dtype=torch.float32, device="cuda") * 2 - 1
        y = torch.empty((no, T, V) if vm else (V, no, T), dtype=torch.float32, device="cuda")

        def unfused():
            b.process(T, x, y, layout=layout, frame_stride=None if vm else T, stream=s)
            if vm:
                F.sum_voices(y, stream=s)
            else:
                F.sum_instances(y, stream=s)

        def fused():
            b.process_mix(T, x, out=mix, layout=layout, frame_stride=None if vm else T, stream=s)

        b.set_option("fx_mix_chunk_frames", 0)
        b.mix_reserve(T)
        u, f = timed(unfused, reps), timed(fused, reps)
        r = dict(unfused=u, fused=f, fused_over_unfused=round(f["median_ms"] / u["median_ms"], 3),
                 bytes_per_instance_frame=dict(unfused=3 * ci + 4 * co if vm else ci + 2 * co, fused=3 * ci + 2 * co if vm or T > auto_chunk else ci + 2 * co))
        if sweep:
            r["chunk_budget_sweep"] = {}
            for mib in (16, 64, 256):
                chunk = max(64, min(1 << 21, (mib << 20) // (V * (ni + no) * 4) // 64 * 64))
                b.set_option("fx_mix_chunk_frames", chunk)
                b.mix_reserve(T)
                r["chunk_budget_sweep"][f"{mib}MiB"] = dict(chunk_frames=chunk, **timed(fused, reps))
            b.set_option("fx_mix_chunk_frames", 0)
        row[lname] = r
        del x, y
    b.close()
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="time the fused calls with the chunk of a 16 / 64 / 256 MiB scratch budget as well")
    ap.add_argument("--only", default="", help="run the shapes whose name contains this")
    a = ap.parse_args()
    V, T = a.instances, a.frames
    makes = [("reverb_stereo(10, 1, 0.5)", lambda: F.Bank.reverb_stereo(V, 10.0, 1.0, 0.5)),
             ("reverb3_stereo(2.0, 0.6, lowpole 1800)", lambda: F.Bank.reverb3_stereo(V, 2.0, 0.6, 1800.0)),
             ("fdn<16> fir3 mono (prelude example)", lambda: F.Bank.fdn(V, 16, delays(16), 3, (0.2, 0.4, 0.2), 1, 1))]
    print(json.dumps(dict(tool="fx_mix_bench", reps=a.reps, rows=[case(n, m, V, T, a.reps, a.sweep) for n, m in makes if a.only in n])))


if __name__ == "__main__":
    main()
