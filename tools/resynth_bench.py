"""Kernel time of the resynthesizer banks (Bank.resynth): 2 048 instances x 48 000 frames at N = 256, 1024, 4096, 1->1 and 2->2 (pass), the
reference's criterion shape (1 instance, 44 100 frames, N = 1024), and the numpy restatement of one instance for scale.  Device events around
each launch (the bank's "timing" option), one warm-up, median of --reps.  Writes profiles/resynth_bench.json (or --out) and prints it.

Algorithmic work per frame (one hop H = N/4 of output per instance and output channel): the source's real FFT, an N/2-point complex FFT
(5 (N/2) log2(N/2) flops) + the split (~10 N/2 flops) + the window (N), and the output's N-point inverse (5 N log2 N flops) + / N (N); the
overlap-add is 8 flops per output sample.  Per instance-sample and output: (flops per frame) / H + 8.  Algorithmic HBM bytes per instance-sample:
4 (inputs + outputs) for the signal, plus the frame ring per output: N floats written per frame of H = N/4 samples (16 bytes per sample) and
4 reads of each sample (16 bytes), plus the input ring per input: one write and N/H = 4 windowed reads per sample (20 bytes).  Bounds: VALU f32
at 78.6 T op/s without FMA (256 CUs x 4 SIMD x 32 lanes x 2.4 GHz, one operation per lane and cycle), HBM at 8 TB/s.

--closure times the closure path instead (Bank.resynth_fn, fd_resynth_fn.hpp) and writes profiles/resynth_fn_bench.json: the pass functor next
to the stock `pass` bank of the same shape in the same run, 1->1 and 1->2, and the STATE = 2 one-pole smoother 1->1.  The closure path moves
the spectra through HBM: per frame (inputs + outputs) x (N/2 + 1) x 8 bytes written and read once, i.e. 64 (inputs + outputs) (N/2 + 1) / N
more bytes per instance-sample (1->1: 60 -> about 124, a factor 2.07)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fundsp_amd as F  # noqa: E402

PEAK_HBM = 8e12
PEAK_VALU = 256 * 4 * 32 * 2.4e9   # f32 operations per second without FMA (one lane-op per lane and cycle, 32-wide SIMDs)


def flops_per_sample(N, I, O):
    H = N // 4
    fwd = 5 * (N // 2) * math.log2(N // 2) + 10 * (N // 2) + N
    inv = 5 * N * math.log2(N) + N
    return O * ((fwd + inv) / H + 8)


def bytes_per_sample(N, I, O):
    return 4 * (I + O) + O * (16 + 16) + I * (4 + 16)


def bytes_per_sample_fn(N, I, O):
    return bytes_per_sample(N, I, O) + 64.0 * (I + O) * (N // 2 + 1) / N


PASS_FN = ("struct BenchPass{O} {{ static constexpr int PARAMS = 0, STATE = 0;\n"
           " template <class W> static __device__ void bin(W& fft, int i) {{ {body} }} }};\n")
SMOOTH_FN = ("struct BenchSmooth { static constexpr int PARAMS = 1, STATE = 2;\n"
             " template <class W> static __device__ void bin(W& fft, int i) {\n  const Cf x = fft.at(0, i); const float a = fft.param(0);\n"
             "  fft.state(0) = fft.state(0) + (x.re - fft.state(0)) * a; fft.state(1) = fft.state(1) + (x.im - fft.state(1)) * a;\n"
             "  fft.set(0, i, Cf{fft.state(0), fft.state(1)}); } };\n")


def closure_rows(reps):
    rows = []
    V, T = 2048, 48000
    for N in (256, 1024, 4096):
        for I, O in ((1, 1), (1, 2)):
            b = F.Bank.resynth(V, N, I, O, source=[0] * O)
            stock = kernel_ms(b, T, I, reps)
            b.close()
            body = " ".join(f"fft.set({o}, i, fft.at(0, i));" for o in range(O))
            b = F.Bank.resynth_fn(V, N, f"BenchPass{O}", PASS_FN.format(O=O, body=body), I, O)
            fn = kernel_ms(b, T, I, reps)
            b.close()
            by = bytes_per_sample_fn(N, I, O) * V * T
            rows.append(dict(shape=f"{V}x{T} N={N} {I}->{O} pass", stock_ms=round(stock, 4), functor_ms=round(fn, 4), functor_over_stock=round(fn / stock, 3),
                             bytes_per_sample_stock=bytes_per_sample(N, I, O), bytes_per_sample_functor=round(bytes_per_sample_fn(N, I, O), 1),
                             functor_hbm_bound_ms=round(by / PEAK_HBM * 1e3, 4), functor_fraction_of_hbm_bound=round(by / PEAK_HBM * 1e3 / fn, 3)))
        b = F.Bank.resynth_fn(V, N, "BenchSmooth", SMOOTH_FN, state=2, a=0.25)
        ms = kernel_ms(b, T, 1, reps)
        b.close()
        rows.append(dict(shape=f"{V}x{T} N={N} 1->1 smoother (STATE = 2)", functor_ms=round(ms, 4)))
    return rows


def kernel_ms(bank, frames, I, reps):
    import torch

    V = bank.voices
    x = torch.rand((I, frames, V), dtype=torch.float32, device="cuda") * 2 - 1
    bank.set_option("timing", 1)
    y = bank.process(frames, x)
    bank.synchronize()
    ms = []
    for _ in range(reps):
        bank.process(frames, x, y)
        bank.synchronize()
        ms.append(bank.last_kernel_ms())
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--closure", action="store_true", help="time the closure path (Bank.resynth_fn) next to the stock pass bank")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "resynth_fn_bench.json" if a.closure else "resynth_bench.json")
    if a.closure:
        out = dict(tool="tools/resynth_bench.py --closure", reps=a.reps, rows=closure_rows(a.reps))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return
    rows = []
    for N in (256, 1024, 4096):
        for I, O in ((1, 1), (2, 2)):
            V, T = 2048, 48000
            b = F.Bank.resynth(V, N, I, O)
            ms = kernel_ms(b, T, I, a.reps)
            b.close()
            samples = V * T
            fl, by = flops_per_sample(N, I, O) * samples, bytes_per_sample(N, I, O) * samples
            t_valu, t_hbm = fl / PEAK_VALU * 1e3, by / PEAK_HBM * 1e3
            rows.append(dict(shape=f"{V}x{T} N={N} {I}->{O}", ms=round(ms, 4), gflop=round(fl / 1e9, 2), gbytes=round(by / 1e9, 3),
                             valu_bound_ms=round(t_valu, 4), hbm_bound_ms=round(t_hbm, 4),
                             binding="valu" if t_valu >= t_hbm else "hbm", fraction_of_bound=round(max(t_valu, t_hbm) / ms, 3)))
    b = F.Bank.resynth(1, 1024)
    ms = kernel_ms(b, 44100, 1, a.reps)
    b.close()
    rows.append(dict(shape="criterion 1x44100 N=1024 1->1", ms=round(ms, 4)))
    import oracle as O
    import resynth_ref as R

    x = np.random.default_rng(0).uniform(-1, 1, (1, 1, 44100)).astype(np.float32)
    tabs = R.tables(1024, O.lib().o_math_cosf)
    t0 = time.perf_counter()
    R.render(x, 1024, tabs=tabs)
    rows.append(dict(shape="numpy restatement, 1x44100 N=1024 1->1, one thread", ms=round((time.perf_counter() - t0) * 1e3, 2)))
    out = dict(tool="tools/resynth_bench.py", reps=a.reps, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
