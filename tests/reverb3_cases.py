"""The case tables of tests/test_gpu_reverb3_matrix.py: reverb3_stereo's lane = frame kernel (fd_reverb3.hip) at every ring capacity an audio
rate reaches, on the ring's edges, and across changes of rate.  Kept apart from the GPU test so that tests/test_reverb3_cases.py can check,
without a device, that the tables claim what is true: the delay arithmetic below restates rv3_make_const (fd_reverb3_const.hpp) operand for
operand, and tests/host/check_reverb3_const.hip prints what rv3_make_const itself computes.  Host arithmetic only."""
import math

LDELAYS = (401, 421, 443, 463, 487, 503, 523, 547, 563, 587, 607, 619, 643, 661, 683, 701,          # reverb.rs:163-166
           727, 743, 761, 787, 809, 823, 839, 863, 883, 907, 929, 947, 967, 983, 1009, 1021)
RDELAYS = (419, 433, 457, 479, 491, 509, 541, 557, 577, 593, 613, 631, 653, 673, 691, 719,          # :167-170
           733, 757, 773, 797, 811, 829, 853, 877, 887, 911, 937, 953, 977, 997, 1013, 1033)
BDELAYS = (1087, 1091, 1093, 1097, 1103, 1109, 1117, 1123)                                          # :171
SHORTEST_LEGAL = 129            # every read distance must exceed two blocks
LONGEST_LEGAL = 1 << 20


def c_round(v):
    """std::round of a non-negative double: half away from zero (v - floor(v) is exact)"""
    f = math.floor(v)
    return int(f) + 1 if v - f >= 0.5 else int(f)


def samples(at_default, sr):
    return c_round((float(at_default) / 44100.0) * float(sr))      # Delay::new(t) at DEFAULT_SR, then set_sample_rate (delay.rs:105-112)


def distances(sr):
    """(dap0[8][4], dap1[8][4], dblk[8]): the read distances of the 72 main rings at `sr`"""
    dap0 = [[samples(LDELAYS[b + j * 8] - 1, sr) + 1 for j in range(4)] for b in range(8)]
    dap1 = [[samples(RDELAYS[b + j * 8] - 1, sr) + 1 for j in range(4)] for b in range(8)]
    dblk = [samples(BDELAYS[7 - b], sr) + (1 if b == 0 else 0) for b in range(8)]
    return dap0, dap1, dblk


def make_const(sr):
    """What rv3_make_const decides at `sr`: a dict of the distances, the extremes, cap and ring_stride -- with ok False (and no ring) where
    it refuses"""
    dap0, dap1, dblk = distances(sr)
    every = [d for row in dap0 for d in row] + [d for row in dap1 for d in row] + dblk
    c = dict(dap0=dap0, dap1=dap1, dblk=dblk, shortest=min(every), longest=max(every), all=every)
    c["ok"] = not (c["shortest"] <= 128 or c["longest"] > LONGEST_LEGAL)
    if c["ok"]:
        cap = 256
        while cap < c["longest"] + 64:
            cap <<= 1
        c["cap"], c["ring_stride"] = cap, 72 * (cap + 64)
    return c


# ---- the rate table: (rate, shortest, longest, cap, why) -------------------------------------------------------------------------------
# FIRST: the longest distance is cap / 2 - 63, the smallest one that needs this capacity (the ring is as empty as it gets)
FULL, FIRST, PLAIN, FLOOR = "longest == cap - 64", "longest == cap / 2 - 63", "a rate people use", "shortest accepted distance"
RATES = [
    (14057.0, 129, 359, 512, FLOOR),
    (17554.0, 160, 448, 512, FULL),
    (17593.0, 161, 449, 1024, FIRST),
    (37679.0, 343, 960, 1024, FULL),
    (37680.0, 343, 961, 2048, FIRST),
    (77891.0, 707, 1984, 2048, FULL),
    (77930.0, 708, 1985, 4096, FIRST),
    (96000.0, 872, 2446, 4096, PLAIN),
    (158300.0, 1437, 4032, 4096, FULL),
    (158317.0, 1437, 4033, 8192, FIRST),
    (192000.0, 1742, 4890, 8192, PLAIN),
    (319140.0, 2896, 8128, 8192, FULL),
    (384000.0, 3484, 9780, 16384, PLAIN),
    (640840.0, 5814, 16320, 16384, FULL),
]
FULL_RATES = [r for r in RATES if r[4] == FULL]
EDGE_RATES = [r for r in RATES if r[4] in (FULL, FLOOR)]         # (b): both kernels and both layouts
REFUSED_LOW, REFUSED_HIGH, ACCEPTED_LOW = 14056.0, 5e7, 14057.0
# every rate the host program prints: the tables, the refusals, and the rates of the migrate pairs
MIGRATE_PAIRS = [(48000.0, 16000.0), (16000.0, 96000.0), (96000.0, 17554.0), (44100.0, 14057.0)]
HOST_RATES = sorted({r[0] for r in RATES} | {REFUSED_LOW, REFUSED_HIGH, 48000.0, 48000.5, 47999.5, 44100.0, 22050.0, 16000.0} | {s for p in MIGRATE_PAIRS for s in p})

V, DENORMAL, IMPULSE = 5, 1, 2                                    # instances as test_gpu_reverb3.signal makes them


def total(cap):
    return 3 * cap + 64 * 3 + 13


def short_line(c):
    """the shortest of the 64 allpass lines"""
    return min(d for row in c["dap0"] + c["dap1"] for d in row)


def cuts(c):
    """The launches of a row, in frames since the reset or rate change that zeroed wp (so wp = frame mod cap):

      0 .. cap - 91            a ragged launch: 64 k + 37 frames; its first block is slow (wp < 64), the rest wide
      cap - 91 .. cap - 10     begins in mid-block: a wide block off the 64-grid, then 17 frames slot by slot
      cap - 10 .. cap + 37     the window straddles the wrap
      cap + 37 .. cap + hs     begins at wp == 37: a full block of which lanes 0 .. 26 write the mirror
      cap + hs .. cap + hl     hs = d_short - 1: the shortest allpass line's read starts at slot cap - 1 and runs through the mirror to cap + 62
      cap + hl .. 2 cap        hl = d_long - 1: the same for block 0's delay, the longest line (d == cap - 64: a 65-frame launch up to the wrap)
      2 cap .. + 1, + 1, + 62  three launches shorter than a block in a row
      2 cap + 64 .. 3 cap      begins at wp == 64, the first wide block, and runs aligned through the last one at wp == cap - 64
      3 cap .. T               64 * 3 + 13 frames"""
    cap, hs, hl = c["cap"], short_line(c) - 1, c["dblk"][0] - 1
    return (0, cap - 91, cap - 10, cap + 37, cap + hs, cap + hl, 2 * cap, 2 * cap + 1, 2 * cap + 2, 2 * cap + 64, 3 * cap, total(cap))


def reset_cuts(cap):
    """after reset(): the first cap + 100 frames again, cut inside the block whose window wraps (fdn_frames_cases.reverb_cuts)"""
    return (0, cap - 91, cap - 10, cap + 100)


def launches(cs):
    return list(zip(cs[:-1], cs[1:]))


def blocks(cs, cap):
    """(frame, wp, size) of every block of every launch"""
    return [(t, t % cap, min(64, e - t)) for a, e in launches(cs) for t in range(a, e, 64)]


def is_wide(wp, size, cap, wq=64):
    """the kernel's choice of block body (the pre rings' half holds for wq: 64 .. 448)"""
    return size == 64 and wp >= 64 and wp + 64 <= cap and wq >= 64 and wq + 64 <= 512


# ---- (c) rate changes: where the first render stops ------------------------------------------------------------------------------------
STOPS = ("unaligned", "wold0", "early")


def first_render(stop, cap_from):
    """frames rendered at the first rate: past two wraps and off the 64-grid | exactly two wraps (wold == 0: the feedback sample sits in slot
    cap - 1) | 70 frames (wold < every distance: no line has given anything yet, z is still zero)"""
    return {"unaligned": 2 * cap_from + 64 + 23, "wold0": 2 * cap_from, "early": 70}[stop]


def loop_trip(c):
    """frames until a sample that enters block 0's delay line first reaches the output, which is block 7's: the eight block delays (an allpass
    passes its input on at once, scaled by eta)"""
    return sum(c["dblk"])


# The rate-change cases run at diffusion 1 (eta = 0.9).  What a change of rate moves -- every allpass's pending sample and the feedback sample,
# which enters block 0 -- is heard at the output only after the block delays in between, and on the direct way a block scales it by
# a * eta^8: 0.38 at eta = 0.9 (4.5e-4 over eight blocks: twenty bits above the rounding of a tail of the same size), but 0.08 at the
# diffusion 0.6 of the other cases (1.7e-9 over eight blocks: below it).
DIFFUSION_MOVED = 1.0


def after_cuts(c_to):
    """the launches at the second rate: a ragged one first, then on until the moved feedback sample has gone round the whole loop and the new
    ring has wrapped"""
    return (0, 64 * 3 + 1, loop_trip(c_to) + c_to["cap"] + 64 * 3 + 9)
