"""The case tables of tests/test_gpu_feedback_delay_matrix.py: every instantiation of k_fb_frames<NL, K> (fd_fbdelay.hip) on the ring's edges,
the capacity step, and every ring capacity 2^8 .. 2^18 -- the last also for k_fdn_frames_filtered, which takes its capacity at run time like
k_fb_frames does.  Kept apart from the GPU test so that tests/test_feedback_delay_cases.py can check, without a device, that the tables cover
what they claim and that the oracle alone meets every side condition.  The launch patterns, the instance numbers and the ring arithmetic are
those of fdn_frames_cases.py; parameters, inputs and the oracle's trees come from the helpers of test_gpu_feedback_delay.py."""
import functools

import numpy as np

import fdn_frames_cases as K
import test_gpu_feedback_delay as FD
from fundsp_amd import MODE_PROCESS
from test_gpu_fdn_network import oracle_network
from test_gpu_fdn_network import params as network_params

f32 = np.float32
SR, V = K.SR, K.V
assert SR == FD.SR
FLUSH_EDGE = 4          # the instance whose noise sinks through the flush threshold; 0: plain noise, K.DENORMAL, K.IMPULSE, K.ALL_SHORTEST
FLUSH_EDGE_TOP, FLUSH_EDGE_DECADES = 1e-35, 3.0
SMALLEST_NORMAL = f32(2.0 ** -126)
SVF = ("lowpass", "bell", "highshelf")


def kind(filt):
    """the kernel's filter branch: none | lowpole | SVF (the FixedSvf modes differ in coefficients only)"""
    return "svf" if filt in SVF else filt


# ---- (a) the short ring: all eight instantiations, each twice --------------------------------------------------------------------------
# Per-instance delays in samples, one row per instance.  Instance 0 holds the line that fills the 256-slot ring (len == cap), instances 1 and
# 2 the two delays whose reads reach the top of the mirror zone under K.CUTS (143, 207: K.mirror_top_delays), K.ALL_SHORTEST every line at 128.
PER1 = ((255,), (143,), (207,), (128,), (191,))
PER2 = ((128, 255), (143, 207), (207, 143), (128, 128), (255, 128))
# channels, reverse(), place, filter, taps, line gain, outer gain, delays ([N]: one table row for the bank | [V][N]: one per instance).
# The kernel's run-time branches are spread so that every pair of their values the grammar allows occurs (the loop form needs a filter and has
# no outer gain), and with the step rows below every taps value meets every filter kind.
SHORT = [
    (1, False, "line", None, 0, True, False, (128,)),
    (1, False, "loop", "lowpole", 0, False, False, PER1),
    (1, False, "line", None, 1, False, True, PER1),
    (1, False, "loop", "bell", 1, True, False, (255,)),
    (1, False, "line", "lowpole", 2, True, True, (255,)),
    (1, False, "loop", "highshelf", 2, False, False, PER1),
    (1, False, "line", "bell", 3, False, False, PER1),
    (1, False, "loop", "lowpass", 3, True, False, (128,)),
    (2, True, "line", "highshelf", 0, False, True, PER2),
    (2, False, "loop", "bell", 0, True, False, (128, 255)),
    (2, False, "line", "lowpole", 1, True, False, (128, 255)),
    (2, True, "loop", "lowpass", 1, False, False, PER2),
    (2, True, "line", None, 2, True, True, (128, 255)),
    (2, True, "loop", "lowpole", 2, True, False, PER2),
    (2, False, "line", None, 3, False, True, PER2),
    (2, True, "loop", "highshelf", 3, False, False, (128, 255)),
]
SHORT_CAP, SHORT_T, SHORT_CUTS = 256, K.T, K.CUTS
# Two rows have no Fir node and are damped by FD.params' line gain of 0.9 alone.  The FLUSH_EDGE scale halves every 129 frames, so at 0.9 a
# trip each older echo is 1.8 times the one behind it and the output stays two decades above the threshold to the end of the noise; a third
# of that gain (0.3, 0.27) lets the newest trip dominate.  The impulse's tenth trip is still 0.3^10 = 6e-6.
LINE_GAIN_SCALE = {("short", 0): 1.0 / 3.0, ("short", 9): 1.0 / 3.0}

# ---- (b) the capacity step: len = 257 is the first length that needs 512 slots, len = 512 fills them ---------------------------------------
# 220 and 399 reach the top of the mirror zone under K.CUTS_STEP
PER_STEP = ((128, 511), (220, 399), (399, 256), (128, 128), (256, 220))
STEP = [
    (1, False, "loop", "lowpole", 2, True, False, (256,)),
    (1, False, "line", "bell", 1, True, False, (511,)),
    (2, False, "loop", "lowpole", 3, True, False, (128, 256)),
    (2, True, "line", None, 0, True, False, (128, 511)),
    (2, True, "line", "highshelf", 2, True, True, PER_STEP),
]
STEP_CAP, STEP_T, STEP_CUTS = 512, K.T_STEP, K.CUTS_STEP
# which rows claim what (test_feedback_delay_cases.py holds them to it)
STEP_FIRST_LENGTH_OF_512 = (0, 2, 4)      # a line of 256 samples
STEP_FULL = (1, 3, 4)                     # a line of 511 samples: len == cap

TABLES = {"short": (SHORT, SHORT_CAP, SHORT_T, SHORT_CUTS), "step": (STEP, STEP_CAP, STEP_T, STEP_CUTS)}


def is_per(delays):
    return np.ndim(delays) == 2


def row_id(row):
    N, rev, place, filt, taps, lg, og, delays = row
    d = "per" if is_per(delays) else "x".join(str(k) for k in delays)
    return f"{N}-{taps}-{place}-{filt}-{'rev' if rev else 'fwd'}-{'lg' if lg else 'nolg'}-{'og' if og else 'noog'}-{d}"


def row_params(table, index):
    """Bank.feedback_delay keyword arguments of a row; a per-instance row spreads every parameter over the instances (FD.params)"""
    N, rev, place, filt, taps, lg, og, delays = TABLES[table][0][index]
    per = is_per(delays)
    p = FD.params(N, place, filt, taps, lg, og, rev, V=V if per else None, delay_samples=np.asarray(delays, dtype=np.float64), seed=40 * (table == "step") + index)
    if (table, index) in LINE_GAIN_SCALE:
        p["line_gain"] = (p["line_gain"] * f32(LINE_GAIN_SCALE[(table, index)])).astype(f32)
    return p


def row_ring(p):
    """(len per instance and line, cap) as the host side computes them"""
    return K.ring_of(p["delays"], SR)


def flush_edge_scale(T):
    """1e-35 * 10^(-3 t / (2T/3)): computed in f64, rounded to f32"""
    stop = 2 * T // 3
    return (FLUSH_EDGE_TOP * 10.0 ** (-FLUSH_EDGE_DECADES * np.arange(T, dtype=np.float64) / stop)).astype(f32)


def matrix_signal(N, T, seed):
    """FD.signal(): noise that stops at 2T/3, instance 1 in the denormal range.  Instance K.IMPULSE is a unit sample at frame 0 on EVERY channel
    (without reverse() a channel that is not driven stays silent); instance FLUSH_EDGE is the noise times a scale that falls from 1e-35 to 1e-38
    while it lasts, so that every row's products cross the flush threshold (1.18e-38) somewhere, whatever its weights and gains."""
    x = FD.signal(V, N, T, seed)
    x[K.IMPULSE] = 0.0
    x[K.IMPULSE, :, 0] = 1.0
    x[FLUSH_EDGE] = x[FLUSH_EDGE] * flush_edge_scale(T)[None, :]
    return x


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(table, index, mode=MODE_PROCESS):
    """(parameters, input, the oracle's render of every instance): computed once per row and executor, shared by the layouts and the tests"""
    rows, _cap, T, cuts = TABLES[table]
    p = row_params(table, index)
    x = matrix_signal(rows[index][0], T, 900 + 31 * index + (table == "step"))
    want = np.stack([FD.oracle_render(FD.oracle_net(p, v), x[v], cuts, mode) for v in range(V)])
    return p, frozen(x), frozen(want)


# ---- (c) every ring capacity ------------------------------------------------------------------------------------------------------------------
# k_fb_frames<2, 3>, loop lowpole, line gain, reversed, delays [128, cap - 1]: plain noise, K.reverb_cuts(cap) -- the second launch ends inside
# the block whose write window wraps, the third begins there.
LADDER = tuple(range(8, 19))
LADDER_V = 2
LADDER_ROW = dict(N=2, place="loop", filt="lowpole", taps=3, line_gain=True, outer=False, reverse=True)
# k_fdn_frames_filtered: log2 cap, lines, filter, place, taps, line gain, inputs, outputs.  32 lines at 2^18 are the largest ring allocation
# either family can make, 32 * (2^18 + 64) * 4 = 33 562 624 bytes per instance: the largest scalar offset the ring steps ever form.
NETWORK_LADDER = [
    (10, 2, "lowpole", "loop", 2, True, 2, 2),
    (14, 2, "lowpole", "loop", 2, True, 2, 2),
    (18, 32, "lowpass", "line", 3, False, 2, 2),
]
LARGEST_RING_BYTES = 32 * (2 ** 18 + 64) * 4


def plain_noise(nin, T, seed):
    return (np.random.default_rng(seed).random((LADDER_V, nin, T), dtype=f32) * 2 - 1).astype(f32)


def ladder_params(log2):
    return FD.params(**LADDER_ROW, delay_samples=[K.SHORTEST, (1 << log2) - 1], seed=log2)


@functools.lru_cache(maxsize=None)
def ladder_reference(log2):
    cuts = K.reverb_cuts(1 << log2)
    p = ladder_params(log2)
    x = plain_noise(2, cuts[-1], 5000 + log2)
    want = np.stack([FD.oracle_render(FD.oracle_net(p, v), x[v], cuts) for v in range(LADDER_V)])
    return p, frozen(x), frozen(want)


def network_delays(log2, lines):
    """128, cap - 1 and the rest spread between, in samples"""
    cap = 1 << log2
    return [K.SHORTEST, cap - 1] + [int(k) for k in np.linspace(K.SHORTEST, cap - 1, lines)[1:-1].round()]


def network_params_of(row):
    log2, lines, filt, place, taps, gain, nin, nout = row
    return network_params(lines, LADDER_V, filt, taps, gain, False, 70 + log2, delay_samples=network_delays(log2, lines))


@functools.lru_cache(maxsize=None)
def network_reference(index):
    row = NETWORK_LADDER[index]
    log2, lines, filt, place, taps, gain, nin, nout = row
    cuts = K.reverb_cuts(1 << log2)
    p = network_params_of(row)
    x = plain_noise(nin, cuts[-1], 6000 + log2)
    want = np.stack([FD.oracle_render(oracle_network(lines, p, v, place, nin, nout), x[v], cuts) for v in range(LADDER_V)])
    return p, frozen(x), frozen(want)
