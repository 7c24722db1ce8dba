#!/usr/bin/env python3
"""The search of the reference's examples/optimize.rs on a bank of candidates: a population of 32-entry delay tables for
reverb4_stereo_delays(times, 100.0), scored by reverb_fitness, kept or replaced by the example's acceptance rule.

Per round: ONE Bank.set_delays upload of the whole population, ONE Bank.reverb_fitness call (render of the impulse responses + scoring, all
on the device), one [population] read-back.  Delays are drawn from 0.030-0.070 s like generate_reverb (reverb.rs:17-28).

NOT the reference's trajectories: the example mutates a funutd `Dna` with funutd's `Rnd`; that crate is not restated here.  Mutation is
numpy's generator instead -- each candidate is its parent with every delay redrawn with probability --rate.  What is the example's is the
loop (optimize.rs:94-131): every member's candidate per round in parallel, a candidate replaces its parent when its fitness is higher or
with probability exp((candidate - parent) / temperature), temperature = 1000 / round; the best table so far is printed at every
improvement.  (The example's repeat penalty has weight 0.0, :22: nothing to restate.)

    python tools/reverb_search.py --population 96 --rounds 50
    python tools/reverb_search.py --bench            # timings of a round for 2 048 and 96 candidates, and of one candidate on one host thread
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LO, HI, TIME = 0.030, 0.070, 100.0


def mutate(rng, parents, rate):
    d = parents.copy()
    m = rng.random(d.shape) < rate
    d[m] = (LO + (HI - LO) * rng.random(int(m.sum()))).astype(np.float32)
    return d


def search(population, rounds, rate, seed):
    import torch

    import fundsp_amd as F

    rng = np.random.default_rng(seed)
    parents = (LO + (HI - LO) * rng.random((population, 32))).astype(np.float32)
    bank = F.Bank.reverb4_stereo_delays(population, parents, TIME)
    bank.fitness_reserve()
    fit = bank.reverb_fitness().cpu().numpy().astype(np.float64)
    best = float(fit.max())
    print(f"round 0: best fitness {best:.3f}")
    for r in range(1, rounds + 1):
        cand = mutate(rng, parents, rate)
        bank.set_delays(cand)
        f = bank.reverb_fitness().cpu().numpy().astype(np.float64)
        temperature = 1000.0 / r
        accept = (f > fit) | (rng.random(population) < np.exp(np.minimum(0.0, (f - fit) / temperature)))   # optimize.rs:121-124
        parents[accept], fit[accept] = cand[accept], f[accept]
        if fit.max() > best:
            best = float(fit.max())
            i = int(fit.argmax())
            print(f"round {r}: best fitness {best:.3f}\n  delays = [{', '.join(repr(float(x)) for x in parents[i])}]")
    torch.cuda.synchronize()
    return parents[int(fit.argmax())], best


def median_ms(fn, n=20):
    """device events around fn(), one warm-up, the median of n"""
    import torch

    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def bench():
    import torch

    import fundsp_amd as F

    N = 32768
    rng = np.random.default_rng(1)
    for V in (2048, 96):
        d = (LO + (HI - LO) * rng.random((V, 32))).astype(np.float32)
        bank = F.Bank.reverb4_stereo_delays(V, d, TIME)
        bank.fitness_reserve()
        x = torch.zeros((V, 2, N), dtype=torch.float32, device="cuda")
        x[:, :, 0] = 1.0
        y = torch.empty_like(x)
        whole = median_ms(lambda: bank.reverb_fitness())
        render = median_ms(lambda: bank.process(N, x, out=y, layout=F.LAYOUT_PLANAR, frame_stride=N))
        score = []                                  # the library's own event pair around the scoring kernels of a call
        for _ in range(21):
            bank.reverb_fitness()
            score.append(bank.get_option("fitness_score_us") / 1e3)
        score = float(np.median(score[1:]))
        t0 = time.perf_counter()
        for _ in range(5):
            bank.set_delays(d)
        upload = (time.perf_counter() - t0) / 5 * 1e3
        print(f"{V} candidates: reverb_fitness call {whole:.3f} ms (impulse fill, 2 resets, render, scoring); the render alone {render:.3f} ms; "
              f"the scoring kernels alone {score:.3f} ms; impulse fill and resets by difference {whole - render - score:.3f} ms; "
              f"set_delays of the population {upload:.3f} ms host wall")
        del bank, x, y
    # one candidate on one host thread: what the example's rayon loop parallelises
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as O
    from reverb_fitness_ref import fitness_f32_serial, fitness_f64

    def one(row):
        g = O.impulse(2) >> O.reverb4_stereo_delays([float(v) for v in row], TIME)
        g.set_sample_rate(44100.0)
        return g.render_blocks(length=N)

    d = (LO + (HI - LO) * rng.random(32)).astype(np.float32)
    one(d)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        r = one(d)
        t1 = time.perf_counter()
        fitness_f32_serial(r)
        t.append((t1 - t0, time.perf_counter() - t1))
    t = np.median(np.array(t), axis=0) * 1e3
    print(f"host, one thread, one candidate: oracle render {t[0]:.1f} ms + fitness_f32_serial {t[1]:.1f} ms")
    r = one(np.array(O.REVERB4_DELAYS, dtype=np.float32))
    print(f"reverb4_stereo_delays(REVERB4_DELAYS, 100.0) at 44.1 kHz: fitness_f64 {fitness_f64(r)[0]:.4f}, fitness_f32_serial {float(fitness_f32_serial(r)[0]):.4f} "
          f"(the reference's comment: \"Fitness -4546\")")
    stock = F.Bank.reverb4_stereo_delays(1, np.array(O.REVERB4_DELAYS, dtype=np.float32), TIME)
    print(f"  the device: {float(stock.reverb_fitness().cpu()[0]):.4f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--population", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rate", type=float, default=0.1, help="probability that a delay of a candidate is redrawn")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--bench", action="store_true")
    a = ap.parse_args()
    if a.bench:
        bench()
    else:
        table, best = search(a.population, a.rounds, a.rate, a.seed)
        print(f"best fitness {best:.3f}")
