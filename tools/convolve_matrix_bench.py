"""Kernel time of the summing convolver banks (Bank.convolve(.., source=[0, 1, 0, 1], target=[0, 0, 1, 1]): the true-stereo response
`(ll + rl) ^ (lr + rr)`, 2 inputs, 4 responses, 2 outputs) against what a caller had before them: the routed 2 -> 4 bank of the same four
responses (source=[0, 0, 1, 1]: ll, lr, rl, rr) followed by the addition of the pairs in a second pass.  2 048 instances x 48 000 frames,
voice-minor, 4 800 and 48 000 taps, shared responses.  Both sides run in the same process, each between two device events on the stream
of the launches (the routed side's events enclose the bank's launch AND the adding pass), one warm-up, median of --reps with min .. max.
Writes profiles/convolve_matrix_bench.json (or --out).

--trace-shape runs three launches of each side at 48 000 taps and nothing else: the run to put under a kernel trace."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fundsp_amd as F  # noqa: E402

TIN, TOUT = [0, 1, 0, 1], [0, 0, 1, 1]     # rows ll, rl, lr, rr
ROUTED = [0, 0, 1, 1]                      # rows ll, lr, rl, rr


def timed(step, reps):
    import torch

    step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median=round(float(np.median(ms)), 3), min=round(float(np.min(ms)), 3), max=round(float(np.max(ms)), 3))


def sides(V, T, h4):
    """(summing step, routed-plus-add step, banks); h4 rows ll, lr, rl, rr"""
    import torch

    x = torch.rand((2, T, V), dtype=torch.float32, device="cuda") * 2 - 1
    summing = F.Bank.convolve(V, np.ascontiguousarray(h4[[0, 2, 1, 3]]), source=TIN, target=TOUT)
    routed = F.Bank.convolve(V, h4, source=ROUTED)
    y2 = torch.empty((2, T, V), dtype=torch.float32, device="cuda")
    y4 = torch.empty((4, T, V), dtype=torch.float32, device="cuda")
    z2 = torch.empty((2, T, V), dtype=torch.float32, device="cuda")

    def step_summing():
        summing.process(T, x, y2)

    def step_routed():
        routed.process(T, x, y4)
        torch.add(y4[:2], y4[2:], out=z2)      # ll + rl, lr + rr

    return step_summing, step_routed, (summing, routed), (y2, z2)


def state_bytes(V, I, O, B, max_len):
    """the formula of fd_convolve.hpp without the response tables"""
    Pcap = -(-max_len // B)
    KB = min(max((256 << 20) // (V * O * (B + 1) * 8), 8), 64)
    Rx = 1
    while Rx < (KB + 1) * B:
        Rx *= 2
    return V * (I * (Rx * 4 + (Pcap + KB) * (B + 1) * 8) + O * (KB * (B + 1) * 8 + (KB + 1) * B * 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convolve_matrix_bench.json"))
    ap.add_argument("--trace-shape", action="store_true", help="three launches of each side at 48 000 taps; no file")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    V, T = 2048, 48000
    rows = []
    for M in ((48000,) if a.trace_shape else (4800, 48000)):
        h4 = (rng.uniform(-1, 1, (4, M)) * np.exp(-np.arange(M) / (M / 5))).astype(np.float32)
        s_sum, s_routed, banks, outs = sides(V, T, h4)
        if a.trace_shape:
            print("summing", timed(s_sum, 2), "routed + add", timed(s_routed, 2))
            return
        row = dict(shape=f"{V}x{T} M={M} shared, true stereo 2 -> 2 of 4 responses", B=banks[0].block_length)
        row["summing_ms"] = timed(s_sum, a.reps)
        row["routed_plus_add_ms"] = timed(s_routed, a.reps)
        banks[1].set_option("timing", 1)
        s_routed()
        banks[1].synchronize()
        row["routed_bank_alone_ms_one_launch"] = round(banks[1].last_kernel_ms(), 3)
        row["summing_state_bytes"] = state_bytes(V, 2, 2, banks[0].block_length, M)
        row["routed_state_bytes"] = state_bytes(V, 2, 4, banks[1].block_length, M)
        # both from a reset: the sides differ in where the additions are rounded only (the float64 bound of tests/test_convolve_matrix_ref.py)
        for b in banks:
            b.reset()
        s_sum()
        s_routed()
        row["max_abs_difference_of_the_sides"] = float((outs[0] - outs[1]).abs().max())
        row["max_abs_output"] = float(outs[0].abs().max())
        row["summing_over_routed_plus_add"] = round(row["summing_ms"]["median"] / row["routed_plus_add_ms"]["median"], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
        for b in banks:
            b.close()
    out = dict(tool="tools/convolve_matrix_bench.py", reps=a.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
