"""Kernel time of the filtered / per-instance FDN networks (Bank.fdn_network) on 2 048 instances x 48 000 frames, planar, against the
unfiltered fdsp_fdn_create network of the same N and delays and against the run-time compiled (fdn_kernel=False) rendering of the same
graph, all in one run.  Prints one JSON line.

    (a) 16 lines, mono:   fdn2(stacki(|i| delay(t_i) >> fir(.2, .4, .2)), stacki(|i| lowpole_hz(c_i) * g_i))
    (b) 32 lines, stereo: fdn(stacki(|i| delay(t_i * room_v) >> fir(.2, .4, .2) >> lowpass_hz(c_i * k_v, q) * g_i)), per-voice parameters

The compiled route renders `--jit-frames` frames and is scaled to 48 000.  Bandwidth share: the algorithmic bytes 8 N + 4 (nin + nout) per
instance-frame over an 8 TB/s HBM peak."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import fundsp_amd as F  # noqa: E402
from fundsp_amd import graph as G  # noqa: E402

PEAK = 8e12


def delays(n):
    return [float(np.float32(0.010 + 0.020 * ((i * 0.6180339887) % 1.0))) for i in range(n)]


def kernel_ms(bank, frames, nin, nout, reps):
    import torch

    V = bank.voices
    x = torch.rand((V, nin, frames), dtype=torch.float32, device="cuda") * 2 - 1
    y = torch.empty((V, nout, frames), dtype=torch.float32, device="cuda")
    bank.set_option("timing", 1)
    best = None
    for r in range(reps + 1):
        bank.process(frames, x, y, layout=F.LAYOUT_PLANAR, frame_stride=frames)
        bank.synchronize()
        ms = bank.last_kernel_ms()
        if r > 0:
            best = ms if best is None else min(best, ms)
    return best


def case(name, n, nin, nout, graph, plan_kw, V, T, jit_frames, reps):
    net = F.Bank.from_graph(graph, V, sample_rate=48000.0)
    assert net.kind == "fdn_network", net.kind
    plain = F.Bank.fdn(V, n, delays(n), 3, (0.2, 0.4, 0.2), nin, nout)
    plain.set_sample_rate(48000.0)
    jit = F.Bank.from_graph(graph, V, sample_rate=48000.0, fdn_kernel=False)
    k = kernel_ms(net, T, nin, nout, reps)
    p = kernel_ms(plain, T, nin, nout, reps)
    j = kernel_ms(jit, jit_frames, nin, nout, 1) * (T / jit_frames)
    bytes_ = (8 * n + 4 * (nin + nout)) * V * T
    return dict(case=name, lines=n, inputs=nin, outputs=nout, instances=V, frames=T, kernel_ms=round(k, 3),
                hbm_share=round(bytes_ / (k * 1e-3) / PEAK, 3), unfiltered_fdn_ms=round(p, 3), ratio_to_unfiltered=round(k / p, 3),
                compiled_ms_scaled=round(j, 1), compiled_frames=jit_frames, speedup_vs_compiled=round(j / k, 1), **plan_kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=48000)
    ap.add_argument("--jit-frames", type=int, default=4800)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    V, T = a.instances, a.frames
    f32 = np.float32
    d16 = delays(16)
    ga = (G.split(16) >> G.fdn2(G.stacki(16, lambda i: G.delay(d16[i]) >> G.fir(0.2, 0.4, 0.2)),
                                G.stacki(16, lambda i: G.lowpole_hz(2000.0 + 150.0 * i) * float(f32(0.98) - f32(0.002) * i))) >> G.join(16))
    d32 = delays(32)
    room = np.linspace(1.0, 1.5, V, dtype=f32)
    kc = np.linspace(0.5, 1.5, V, dtype=f32)
    gb = (G.multisplit(2, 16) >> G.fdn(G.stacki(32, lambda i: G.delay((room * f32(d32[i])).astype(f32)) >> G.fir(0.2, 0.4, 0.2)
                                                >> G.lowpass_hz((kc * f32(3000.0 + 100.0 * i)).astype(f32), 0.9) * 0.97)) >> G.multijoin(2, 16))
    rows = [case("a_loop_lowpole_16_mono", 16, 1, 1, ga, dict(place="loop", filter="lowpole", per_voice=False), V, T, a.jit_frames, a.reps),
            case("b_line_svf_32_stereo", 32, 2, 2, gb, dict(place="line", filter="lowpass", per_voice=True), V, T, a.jit_frames, a.reps)]
    print(json.dumps(dict(tool="fdn_network_bench", rows=rows)))


if __name__ == "__main__":
    main()
