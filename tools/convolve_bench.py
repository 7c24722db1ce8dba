"""Kernel time of the convolver banks (Bank.convolve): 2 048 instances x 48 000 frames, 1 and 2 channels, shared and per-instance responses of
4 800 / 48 000 / 96 000 taps; 64-frame launches of the 48 000-tap bank (mean and worst launch: a block boundary lands in one launch out of
B / 64); one instance x 44 100 frames.  Device events around each launch (the bank's "timing" option), one warm-up, median of --reps.  Next to
each shape: a yardstick a PyTorch user would write, torch.fft.rfft / irfft over the whole launch (length T + M, batched over the instances) on the
same GPU in the same run -- no streaming state and no bit contract, so a comparison, not a gate.  Writes profiles/convolve_bench.json (or --out).

Algorithmic work per output sample and channel (B = block length, P = ceil(M / B)): tail 8 P operations per bin and block over B + 1 bins =
8 P (B + 1) / B; head 2 * (B + 1) / 2 on average (min(r, M - 1) + 1 taps); transforms per block: forward 5 B log2 B + 10 B, inverse
5 (2B) log2 (2B) + 2B, both / B.  HBM bytes per output sample and channel as the kernels move them: signal 8, input ring 4 written + 4 read by
the forward + 4 read by the output, spectra 8 (B + 1) / B written, the tail's reads (P + J - 1) / J spectra of 8 (B + 1) bytes per block (J = 8
boundaries share a walk; fewer per launch when a launch reaches fewer), Z 16 (B + 1) / B, pend 4 + 4.  Shared response spectra are read through
the caches and not counted; per-instance ones add P * 8 (B + 1) / (J B).  Bounds: VALU f32 at 78.6 T op/s without FMA, HBM at 8 TB/s."""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fundsp_amd as F  # noqa: E402

PEAK_HBM = 8e12
PEAK_VALU = 256 * 4 * 32 * 2.4e9
J = 8


def ops_per_sample(M, B):
    P = -(-M // B)
    tail = 8 * P * (B + 1) / B
    head = min(B, M) + 1
    fft = (5 * B * math.log2(B) + 10 * B + 5 * 2 * B * math.log2(2 * B) + 2 * B) / B
    return tail + head + fft


def bytes_per_sample(M, B, per, j=J):
    P = -(-M // B)
    s = 8 + 12 + 8 * (B + 1) / B + (P + j - 1) / j * 8 * (B + 1) / B + 16 * (B + 1) / B + 8
    return s + (P * 8 * (B + 1) / (j * B) if per else 0)


def launch_ms(bank, frames, C, reps, each=False):
    import torch

    x = torch.rand((C, frames, bank.voices), dtype=torch.float32, device="cuda") * 2 - 1
    bank.set_option("timing", 1)
    y = bank.process(frames, x)
    bank.synchronize()
    ms = []
    for _ in range(reps):
        bank.process(frames, x, y)
        bank.synchronize()
        ms.append(bank.last_kernel_ms())
    return ms if each else float(np.median(ms))


def torch_ms(V, C, T, M, reps):
    import torch

    x = torch.rand((V * C, T), dtype=torch.float32, device="cuda")
    h = torch.rand((C, M), dtype=torch.float32, device="cuda").repeat(V, 1)
    n = T + M
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(reps + 1):
        ev[0].record()
        y = torch.fft.irfft(torch.fft.rfft(x, n=n) * torch.fft.rfft(h, n=n), n=n)[:, :T]
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            ms.append(ev[0].elapsed_time(ev[1]))
        del y
    return float(np.median(ms))


def smi():
    try:
        return subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=20).stdout.strip().splitlines()
    except Exception as e:   # noqa: BLE001 -- the note is optional
        return [f"rocm-smi not available: {e}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convolve_bench.json"))
    ap.add_argument("--quick", action="store_true", help="shared responses and one channel only")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    rows = []
    V, T = 2048, 48000
    for M in (4800, 48000, 96000):
        for C in ((1,) if a.quick else (1, 2)):
            for per in ((False,) if a.quick else (False, True)):
                h = (rng.uniform(-1, 1, ((V, C, M) if per else (C, M))) * np.exp(-np.arange(M) / (M / 5))).astype(np.float32)
                b = F.Bank.convolve(V, h, per_instance=per)
                B = b.block_length
                ms = launch_ms(b, T, C, a.reps)
                b.close()
                n = V * C * T
                op, by = ops_per_sample(M, B) * n, bytes_per_sample(M, B, per) * n
                tv, th = op / PEAK_VALU * 1e3, by / PEAK_HBM * 1e3
                rows.append(dict(shape=f"{V}x{T} M={M} C={C} {'per-instance' if per else 'shared'}", B=B, ms=round(ms, 3), gop=round(op / 1e9, 1),
                                 gbytes=round(by / 1e9, 2), valu_bound_ms=round(tv, 3), hbm_bound_ms=round(th, 3), binding="valu" if tv >= th else "hbm",
                                 fraction_of_bound=round(max(tv, th) / ms, 3), torch_fft_ms=round(torch_ms(V, C, T, M, 5), 3) if not per else None))
    M = 48000
    h = (rng.uniform(-1, 1, (1, M)) * np.exp(-np.arange(M) / (M / 5))).astype(np.float32)
    b = F.Bank.convolve(V, h)
    ms = launch_ms(b, 64, 1, 64 * 4, each=True)
    b.close()
    rows.append(dict(shape=f"{V}x64-frame launches M={M} C=1 shared", B=b.block_length, mean_ms=round(float(np.mean(ms)), 4), median_ms=round(float(np.median(ms)), 4),
                     worst_ms=round(float(np.max(ms)), 4), launches=len(ms)))
    b = F.Bank.convolve(1, h)
    rows.append(dict(shape=f"1x44100 M={M} C=1", B=b.block_length, ms=round(launch_ms(b, 44100, 1, a.reps), 4), torch_fft_ms=round(torch_ms(1, 1, 44100, M, 5), 4)))
    b.close()
    out = dict(tool="tools/convolve_bench.py", reps=a.reps, device_state=smi(), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
