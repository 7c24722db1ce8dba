"""Kernel time of the routed convolver banks (Bank.convolve(.., source=[0, 0]): one input through two responses) against the two banks a caller
had before them: (a) the 2 -> 2 stack bank of the same two responses fed the input twice -- the plain bank's kernels, which the routed banks
leave as they were -- and (b) the 1 -> 1 bank of one of the responses, the floor.  2 048 instances x 48 000 frames, voice-minor, 4 800 and
48 000 taps, shared and per-instance responses.  The method of tools/convolve_bench.py: device events around each launch (the bank's
"timing" option), one warm-up, median of --reps with min .. max.  Writes profiles/convolve_routed_bench.json (or --out).

`accepted`: the routed median is not above the stack bank's median by more than the stack bank's own min .. max spread in the same run.
--trace-shape runs three launches of the routed and of the stack bank at 48 000 taps, shared, and nothing else: the run to put under a
kernel trace."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fundsp_amd as F  # noqa: E402


def launch_ms(bank, frames, reps):
    import torch

    x = torch.rand((bank.inputs(), frames, bank.voices), dtype=torch.float32, device="cuda") * 2 - 1
    bank.set_option("timing", 1)
    y = bank.process(frames, x)
    bank.synchronize()
    ms = []
    for _ in range(reps):
        bank.process(frames, x, y)
        bank.synchronize()
        ms.append(bank.last_kernel_ms())
    return dict(median=round(float(np.median(ms)), 3), min=round(float(np.min(ms)), 3), max=round(float(np.max(ms)), 3))


def state_bytes(V, I, C, B, max_len):
    """the formula of fd_convolve.hpp without the response tables"""
    Pcap = -(-max_len // B)
    KB = min(max((256 << 20) // (V * C * (B + 1) * 8), 8), 64)
    Rx = 1
    while Rx < (KB + 1) * B:
        Rx *= 2
    return V * (I * (Rx * 4 + (Pcap + KB) * (B + 1) * 8) + C * (KB * (B + 1) * 8 + (KB + 1) * B * 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convolve_routed_bench.json"))
    ap.add_argument("--trace-shape", action="store_true", help="three launches of the routed and the stack bank at 48 000 taps, shared; no file")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    V, T = 2048, 48000
    if a.trace_shape:
        h = (rng.uniform(-1, 1, (2, 48000)) * np.exp(-np.arange(48000) / 9600)).astype(np.float32)
        for source in ([0, 0], None):
            b = F.Bank.convolve(V, h, source=source)
            print(source, launch_ms(b, T, 2))
            b.close()
        return
    rows = []
    for M in (4800, 48000):
        for per in (False, True):
            h = (rng.uniform(-1, 1, ((V, 2, M) if per else (2, M))) * np.exp(-np.arange(M) / (M / 5))).astype(np.float32)
            banks = dict(routed_1to2=lambda: F.Bank.convolve(V, h, per_instance=per, source=[0, 0]),
                         stack_2to2=lambda: F.Bank.convolve(V, h, per_instance=per),
                         floor_1to1=lambda: F.Bank.convolve(V, np.ascontiguousarray(h[..., :1, :]), per_instance=per))
            row = dict(shape=f"{V}x{T} M={M} {'per-instance' if per else 'shared'}")
            for name, make in banks.items():
                b = make()
                row["B"] = b.block_length
                row[name + "_ms"] = launch_ms(b, T, a.reps)
                row[name + "_state_bytes"] = state_bytes(V, b.inputs(), b.outputs(), b.block_length, M)
                b.close()
            r, s = row["routed_1to2_ms"], row["stack_2to2_ms"]
            row["routed_over_stack"] = round(r["median"] / s["median"], 4)
            row["routed_over_floor"] = round(r["median"] / row["floor_1to1_ms"]["median"], 4)
            row["accepted"] = bool(r["median"] <= s["median"] + (s["max"] - s["min"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = dict(tool="tools/convolve_routed_bench.py", reps=a.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
