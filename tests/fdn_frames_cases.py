"""The case tables of tests/test_gpu_fdn_frames_matrix.py: every instantiation of the three lane = frame Hadamard kernels (fd_fdn.hip,
fd_fdnx.hip) on the ring's edges.  Kept apart from the GPU test so that tests/test_fdn_frames_cases.py can check, without a device, that the
tables still cover what they claim.  Host arithmetic only: delays in samples, ring lengths, capacities."""
import numpy as np

f32 = np.float32

LINES = (2, 4, 8, 16, 32)
IO = ((1, 1), (2, 2), (2, 1), (1, 2))                   # (inputs, outputs): split / multisplit in front, join / multijoin behind
SR = 48000.0            # the filtered networks are created at this rate (Bank.fdn_network takes one)
SR_GENERIC = 44100.0    # Bank.fdn creates its bank at DEFAULT_SR and checks the 128-sample rule THERE, so a generic network with a 128-sample
                        # line exists at 44.1 kHz only: its delays are k / 44100 s.  What the kernel sees (len, cap) is the same.

# ---- the short ring: (a), (b) --------------------------------------------------------------------------------------------------------
V = 5                                                   # one workgroup of four waves and one with a single live wave
T = 64 * 30 + 13
CUTS = (0, 64, 141, 142, 475, 64 * 12 + 475, T)         # launches of 64, 77, 1, 333, 768 and 690 frames: the 256-slot window wraps 7 times
DENORMAL, IMPULSE, ALL_SHORTEST = 1, 2, 3               # instances: input in the denormal range | a unit impulse | (per instance) all lines at D = 128
# ... and one whose noise straddles the smallest normal number (1.18e-38).  Join / MultiJoin over a power of two lines differ between the
# executors ONLY there: process scales every term by 1 / n first (a term under n * 1.18e-38 flushes to zero), tick divides the sum.
FLUSH_EDGE, FLUSH_EDGE_SCALE = 4, 3e-38
SHORTEST, RESET_FRAMES = 128, 700


def mirror_top_delays(cuts, cap):
    """The delays whose 64-slot read window starts, at the head of some full block of these launches, in the ring's LAST slot: lane 63 then
    reads mirror slot cap + 62, the highest one any read reaches (a window starts at cap - 1 at the latest, so slot cap + 63 is written but
    never read).  A line with such a delay is the one that notices a mirror that is a slot short."""
    heads = {h for a, e in zip(cuts[:-1], cuts[1:]) for h in range(a, e - 63, 64)}
    return {d for d in range(SHORTEST, cap) if any((h - d) % cap == cap - 1 for h in heads)}


def _spread(lo, hi, count, taken):
    out = []
    for k in np.linspace(lo, hi, count).round():
        k = int(k)
        while k in taken or k in out:
            k += 1
        out.append(k)
    return out


def short_ring(n):
    """delays in samples: line 0 the shortest legal one, line 1 fills the 256-slot ring (len == cap); from four lines on, two whose reads
    reach the top of the mirror zone under CUTS (143, 207: mirror_top_delays); the rest distinct over 129 .. 254"""
    fixed = [SHORTEST, 255] + ([143, 207] if n >= 4 else [])
    return fixed + _spread(129, 253, n - len(fixed), fixed)


def step_ring(n, second):
    """(c): the shortest line, `second`, and for 32 lines both sides of the step (256: len = cap/2 + 1; 511: len == cap), two lines that
    reach the top of the mirror zone under CUTS_STEP (220, 399) and the rest in between"""
    if n == 2:
        return [SHORTEST, second]
    fixed = [SHORTEST, 256, 511, 220, 399]
    return fixed + _spread(131, 509, n - len(fixed), fixed)


def seconds(k, sr):
    """k samples at sr as the f32 seconds the reference's delay(t: f32) takes (prelude.rs:893), as a double"""
    return np.asarray(f32(np.asarray(k, dtype=np.float64) / sr), dtype=np.float64)


def ring_of(delays, sr):
    """(len per line, cap) as the host side of the kernels computes them: len = round(t * sr) + 1 (delay.rs:104-112), cap = the power of
    two >= the longest len and >= 256 (shared by the bank)"""
    lens = np.floor(np.asarray(delays, dtype=np.float64) * sr + 0.5).astype(np.int64) + 1
    cap = 256
    while cap < int(lens.max()):
        cap <<= 1
    return lens, cap


def per_instance_samples(base):
    """[V, n] delays in samples of a per-instance bank: instance 0 the table itself (it holds the len == cap line), ALL_SHORTEST every line at
    128, the others the table's distance to 128 scaled -- in samples, so they stay integers"""
    b = np.asarray(base, dtype=np.int64)
    rows = [b if v == 0 else (np.full_like(b, SHORTEST) if v == ALL_SHORTEST else SHORTEST + ((b - SHORTEST) * (11 - 2 * v)) // 11) for v in range(V)]
    return np.stack(rows)


# (a) k_fdn_frames_generic<lines, taps>: all 15.  FIR weights distinct from tap to tap (swapped taps show), |sum| < 1, the sign alternates.
GENERIC_W = {1: (0.93,), 2: (0.55, 0.4), 3: (0.21, 0.45, 0.27)}
GENERIC_CASES = []      # lines, taps, weights, inputs, outputs
for _i, (_n, _k) in enumerate((n, k) for n in LINES for k in (1, 2, 3)):
    GENERIC_CASES.append((_n, _k, tuple((-w if _i % 2 else w) for w in GENERIC_W[_k]), *IO[_i % 4]))

# (b) k_fdn_frames_filtered<lines, taps>: all 20.  The kernel's run-time branches (filter kind, place, line gain, shared / per-instance
# parameters) are spread so that every pair of their values occurs (the loop form needs a filter: (None, "loop") does not exist), every taps
# value meets every filter kind and every lines value both places.  A line without a Fir node keeps its gain (nothing else damps it).
FILTERS = (None, "lowpole", "lowpass", "highshelf")
_FILTERED = [  # lines, taps, filter, place, line gain, per-instance
    (2, 0, None, "line", True, False),
    (2, 1, "lowpole", "loop", False, True),
    (2, 2, "lowpass", "line", True, True),
    (2, 3, "highshelf", "loop", False, False),
    (4, 0, "lowpole", "line", True, False),
    (4, 1, "lowpass", "loop", True, False),
    (4, 2, "highshelf", "line", False, True),
    (4, 3, None, "line", False, True),
    (8, 0, "lowpass", "loop", True, True),
    (8, 1, "highshelf", "line", False, False),
    (8, 2, None, "line", True, True),
    (8, 3, "lowpole", "loop", True, False),
    (16, 0, "highshelf", "loop", True, True),
    (16, 1, None, "line", False, False),
    (16, 2, "lowpole", "line", False, True),
    (16, 3, "lowpass", "loop", False, False),
    (32, 0, None, "line", True, True),
    (32, 1, "lowpole", "loop", True, True),
    (32, 2, "lowpass", "line", False, False),
    (32, 3, "highshelf", "line", True, False),
]
FILTERED_CASES = [r + IO[i % 4] for i, r in enumerate(_FILTERED)]   # .. , inputs, outputs

# (c) the capacity step: len = 257 takes cap to 512, len = 512 fills it.  Two lines hold one side each.
T_STEP = 64 * 60 + 13                                                       # 7.5 wraps of 512 slots
CUTS_STEP = (0, 128, 269, 270, 923, 64 * 24 + 923, T_STEP)                  # the pattern above, twice as long: 128, 141, 1, 653, 1536, 1394
STEP_GENERIC = [   # lines, taps, weights, inputs, outputs, the second line's delay
    (2, 2, (0.55, 0.4), 1, 1, 256),
    (2, 2, (0.55, 0.4), 2, 2, 511),
    (32, 3, (-0.21, -0.45, -0.27), 2, 1, 256),
]
STEP_FILTERED = [  # lines, taps, filter, place, line gain, per-instance, inputs, outputs, the second line's delay
    (2, 2, "lowpole", "loop", True, False, 1, 2, 256),
    (2, 2, "lowpole", "loop", True, False, 2, 1, 511),
    (32, 3, "lowpass", "line", False, False, 2, 2, 256),
]

# (e) k_fdn_render_frames<CAP_LOG2, NSEC>: NSEC = 1 reverb_stereo(room, room / 5, 0.5), NSEC = 2 reverb4_stereo(room, 2.0) -- reverb_stereo's
# loop gain is 0.001 ^ (0.003 * room / time) (prelude.rs:1746), so its time grows with the room and every ring recirculates at 0.9.  Both banks are
# created at DEFAULT_SR and then moved to `sr`; every line has to hold 128 samples at both rates.  2^8 cannot be reached by either (the
# longest line is more than twice the shortest: see the GPU test's docstring), 2^9 .. 2^18 are.
REVERB_DAMPING, REVERB_V = 0.5, 2


def reverb_time(nsec, room):
    return room / 5.0 if nsec == 1 else 2.0


REVERB_CAPS = tuple(range(9, 19))
REVERB_UNREACHABLE = (8,)
REVERB_CASES = [  # NSEC, CAP_LOG2, room size, sample rate, tick executor too
    (1, 9, 1.0, 48000.0, False),
    (1, 10, 2.0, 48000.0, False),
    (1, 11, 4.0, 48000.0, False),
    (1, 12, 8.0, 48000.0, False),
    (1, 13, 16.0, 48000.0, False),
    (1, 14, 32.0, 48000.0, False),
    (1, 15, 64.0, 48000.0, False),
    (1, 16, 128.0, 48000.0, False),
    (1, 17, 256.0, 48000.0, False),
    (1, 18, 512.0, 48000.0, False),
    # reverb4_stereo never shrinks below room size 15: the small rings are low sample rates
    (2, 9, 15.0, 3000.0, True),
    (2, 10, 15.0, 6000.0, False),
    (2, 11, 15.0, 12000.0, False),
    (2, 12, 15.0, 24000.0, False),
    (2, 13, 15.0, 48000.0, True),
    (2, 14, 30.0, 48000.0, False),
    (2, 15, 60.0, 48000.0, False),
    (2, 16, 120.0, 48000.0, False),
    (2, 17, 240.0, 48000.0, False),
    (2, 18, 480.0, 48000.0, False),
]


def reverb_lens(nsec, room, sr):
    """ring lengths of the 32 lines, from the delay tables the oracle renders with: reverb_stereo delay(DELAYS[i] * room / 10) in f64
    (prelude.rs:1739-1751), reverb4_stereo delay((d_i as f32 * max(room as f32, 15) / 10) as f64) (:1909-1913, 1924)"""
    import oracle as O

    if nsec == 1:
        return O.reverb_stereo_params(room, reverb_time(1, room), REVERB_DAMPING, sr)[1].astype(np.int64) + 1
    else:
        d = (np.array(O.REVERB4_DELAYS, dtype=f32) * (max(f32(room), f32(15.0)) / f32(10.0))).astype(np.float64)
    return np.floor(d * sr + 0.5).astype(np.int64) + 1


def reverb_cuts(cap):
    """T = cap + 3 * 64 + 13 frames; the second launch is ragged and ends inside the block whose write window wraps (slots cap - 27 ..),
    the third begins there (at slot cap - 10)"""
    return (0, cap - 91, cap - 10, cap + 3 * 64 + 13)
