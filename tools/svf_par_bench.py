"""tools/svf_par_bench.py -- the strong-scaling shards of the headline (8 192 and 16 384 config-3 voices x 48 000 frames) in tolerance
mode with "svf_exec" = 0 (the time-split kernel's serial filter wave: the baseline, an unchanged code object) and 1 (the time-parallel
filter stage, fd_tsp.hpp), alternating launch by launch in one process after a warm-up.

  tools/svf_par_bench.py [--launches 50] [--repeats 3] [--sizes 8192,16384] [--label TEXT] [--out profiles/svf_par_bench.json]
      times every launch with the bank's HIP event pair; per size and executor the mean of each repeat and their spread, then
      the full-second deviation of both tolerance-mode executors from the exact bank (max and rms).  --out: the JSON is merged
      into that file under --label (one entry per library variant measured).
  tools/svf_par_bench.py --trace
      a few launches of each and nothing else: the program to put behind `rocprofv3 --kernel-trace --stats --` for kernel times
      (tools/rocprof_summary.py reads the result)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fundsp_amd as F
from fundsp_amd import workloads as W

T, SR = 48000, 48000.0


def bank(V, math, svf_exec):
    b = W.make_fm_svf_bank(V, SR)
    b.set_option("math", math)
    b.set_option("svf_exec", svf_exec)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="8192,16384")
    ap.add_argument("--label", default="default")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-deviation", action="store_true")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    res = {"method": f"fm_svf, FDSP_MATH_FAST, {T} frames per launch, HIP event pair of every launch; svf_exec 0 and 1 alternate launch by launch "
                     f"after 3 warm-up launches each; {a.repeats} repeats of {a.launches} launches per executor",
           "library": os.path.basename(F._lib.SO_PATH), "sizes": {}}
    for V in sizes:
        out = torch.empty((1, T, V), dtype=torch.float32, device="cuda")
        banks = [bank(V, F.MATH_FAST, F.SVF_SERIAL), bank(V, F.MATH_FAST, F.SVF_PARALLEL)]
        n = 3 if a.trace else a.launches
        for b in banks:
            for _ in range(3):
                b.process(T, None, out, layout=F.LAYOUT_VOICE_MINOR, mode=F.MODE_PROCESS)
        kernels = [b.get_option("last_kernel") for b in banks]
        runs = [[], []]
        for _ in range(1 if a.trace else a.repeats):
            ms = [[], []]
            for _ in range(n):
                for i, b in enumerate(banks):
                    b.process(T, None, out, layout=F.LAYOUT_VOICE_MINOR, mode=F.MODE_PROCESS)
                    ms[i].append(b.last_kernel_ms())
            for i in range(2):
                runs[i].append(ms[i])
        del banks
        row = {}
        for i, name in enumerate(("svf_exec_0", "svf_exec_1")):
            means = [float(np.mean(r)) for r in runs[i]]
            flat = np.concatenate(runs[i])
            row[name] = {"last_kernel": kernels[i], "mean_ms": float(np.mean(means)), "repeat_means_ms": means,
                         "spread_of_repeats_ms": float(max(means) - min(means)), "min_ms": float(flat.min()), "max_ms": float(flat.max()),
                         "std_of_launches_ms": float(flat.std())}
        row["reduction_ms"] = row["svf_exec_0"]["mean_ms"] - row["svf_exec_1"]["mean_ms"]
        print(f"{V} voices: svf_exec 0 (kernel {kernels[0]}) {row['svf_exec_0']['mean_ms']:.4f} ms +- {row['svf_exec_0']['spread_of_repeats_ms']:.4f} | "
              f"svf_exec 1 (kernel {kernels[1]}) {row['svf_exec_1']['mean_ms']:.4f} ms +- {row['svf_exec_1']['spread_of_repeats_ms']:.4f} | "
              f"reduction {row['reduction_ms']:.4f} ms", flush=True)
        if not a.trace and not a.no_deviation:  # the first second of fresh banks against the exact bank
            exact = torch.empty_like(out)
            bank(V, F.MATH_EXACT, F.SVF_SERIAL).process(T, None, exact, layout=F.LAYOUT_VOICE_MINOR, mode=F.MODE_PROCESS)
            for name, ex in (("svf_exec_0", F.SVF_SERIAL), ("svf_exec_1", F.SVF_PARALLEL)):
                bank(V, F.MATH_FAST, ex).process(T, None, out, layout=F.LAYOUT_VOICE_MINOR, mode=F.MODE_PROCESS)
                d = (out.double() - exact.double()).abs()
                row[name]["vs_exact_max"] = float(d.max())
                row[name]["vs_exact_rms"] = float((d * d).mean().sqrt())
                del d
                print(f"  {name} vs the exact bank over the second: max {row[name]['vs_exact_max']:.3e} rms {row[name]['vs_exact_rms']:.3e}", flush=True)
            del exact
        res["sizes"][str(V)] = row
        del out
        torch.cuda.empty_cache()
    if a.trace:
        return
    print(json.dumps({a.label: res}))
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            doc = json.load(open(a.out))
        doc[a.label] = res
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
