"""Every instantiation of the lane = frame Hadamard kernels, on the edges of the ring, bit for bit against the oracle.

The three kernels (fd_fdn.hip, fd_fdnx.hip) are sequences of the shared steps of fd_fdn_frames.hpp, compiled 57 times: every
instantiation has its own register allocation.  The tables of fdn_frames_cases.py (checked without a device by test_fdn_frames_cases.py)
render each of them against the oracle's generic Feedback / Feedback2 tree, which shares no code with the kernels:

(a) k_fdn_frames_generic<lines, taps>, all 15, and (b) k_fdn_frames_filtered<lines, taps>, all 20, on the SHORT RING: line 0 delays by
    128 samples -- the shortest legal delay: frame 63 of block B + 1 reads, at the head of block B, the slot frame 63 of block B - 1 has
    just written -- line 1 by 255 (len == cap == 256: frame 0 reads slot wp + 1, the oldest sample in the ring), the others in between.
    1 933 frames in launches of 64, 77, 1, 333, 768 and 690: the 256-slot write window wraps seven times, the ragged launches walk the
    mirror zone slot by slot, launches begin in mid-block.  From four lines on, two lines (143, 207 samples) read through the last mirror
    slot any read reaches.  Five instances (a workgroup with one live wave), one fed from the denormal range, one by a unit impulse, one
    by noise around the flush threshold (where alone Join differs between the executors: 1 / n is a power of two); both executors;
    voice-minor on the taps = 3 rows; reset and the first 700 frames again.
    The generic banks run at 44.1 kHz, the filtered ones at 48 kHz: fdsp_fdn_create builds its bank at DEFAULT_SR and applies the
    128-sample rule there, so a generic network with a 128-sample line cannot be built for another rate.  The delays are whole samples at
    the bank's rate either way, and every case asserts the len and cap the kernel gets.
(c) the capacity step: <2, 2> and <32, 3> of both kernels with lines at 128, 256 (len = 257: cap 512) and 511 (len == cap) samples.
(d) the refusals at the boundary: 127 samples refused at creation and at set_sample_rate, 128 accepted.
(e) k_fdn_render_frames<CAP_LOG2, NSEC>: reverb_stereo (NSEC = 1) and reverb4_stereo (NSEC = 2) at every ring capacity 2^9 .. 2^18,
    cap + 205 frames cut inside the block whose write window wraps.  20 of the ladder's 22 entries.  The other two, <8, 1> and <8, 2>,
    cannot be reached: a 256-slot ring needs every delay D in 128 .. 255, and both delay tables span more than that ratio at any room
    size and rate.  reverb_stereo: D_i = round(DELAYS[i] * room / 10 * sr), longest 0.082923 over shortest 0.036084 = 2.298, so
    min D >= 128 gives max D >= 293 (len 294 > 256).  reverb4_stereo: longest 0.06995449 over shortest 0.031507637 = 2.220, so
    max D >= 283.  (The ladder entry stays; DESIGN.md records it.)

No tolerance appears in this file."""
import functools

import numpy as np
import pytest

import fdn_frames_cases as K
import oracle as O
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from test_gpu_fdn import oracle_net, run
from test_gpu_fdn_network import oracle_network, params, signal
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
MODES = [MODE_PROCESS, MODE_TICK]
# A tail that "still sounds" is one of normal numbers with all 24 bits of mantissa in play: anything above 1e-9 is 29 decades over the
# flush threshold (1.2e-38), and a unit impulse that has gone round a damped network ten times is still well above that.
SOUNDS = 1e-9


def oracle_render(net, x, cuts, mode):
    return np.concatenate([net.render_blocks(x[:, a:e]) if mode == MODE_PROCESS else net.render_ticks(x[:, a:e]) for a, e in zip(cuts[:-1], cuts[1:])], axis=1)


def matrix_signal(nin, T, seed):
    """signal() with its impulse instance, and the instance whose samples lie around the flush threshold"""
    x = signal(K.V, nin, T, seed, impulse=K.IMPULSE)
    x[K.FLUSH_EDGE] *= np.float32(K.FLUSH_EDGE_SCALE)
    return x


def frozen(a):
    a.setflags(write=False)
    return a


def layouts_of(taps):
    return [LAYOUT_PLANAR, LAYOUT_VOICE_MINOR] if taps == 3 else [LAYOUT_PLANAR]


def check_edges(lens, cap, want_cap, shortest_and_full):
    """the case is about these numbers: a line at exactly 128 samples, a line that fills the ring, the capacity"""
    assert cap == want_cap and int(lens.min()) == K.SHORTEST + 1 and int(lens.max()) <= cap
    if shortest_and_full:
        assert int(lens.max()) == cap


def check_render(bank, x, got, want, layout, mode, what):
    V = x.shape[0]
    assert bank.get_option("last_kernel") == 6
    for v in range(V):
        assert_bit_equal(got[v], want[v], f"{what} instance {v}")
    assert np.isfinite(got).all()
    T = x.shape[2]
    assert np.abs(got[K.IMPULSE][:, 2 * T // 3:]).max() > SOUNDS          # the impulse still recirculates: no tail of zeros
    assert not np.any((got[K.DENORMAL] != 0) & (np.abs(got[K.DENORMAL]) < np.float32(1.17549435e-38)))   # these translation units flush
    bank.reset()
    assert_bit_equal(run(bank, x[:, :, :K.RESET_FRAMES], layout, mode, [0, K.RESET_FRAMES]), got[:, :, :K.RESET_FRAMES], f"{what} after reset")


# ---- the generic kernel ------------------------------------------------------------------------------------------------------------------
def generic_delays(samples):
    return [float(d) for d in K.seconds(samples, K.SR_GENERIC)]


@functools.lru_cache(maxsize=None)
def generic_reference(n, w, nin, nout, samples, T, cuts, mode):
    """(input, the oracle's render of every instance): computed once per case and executor, shared by the layouts"""
    x = matrix_signal(nin, T, 300 + 7 * n + len(w))
    delays = generic_delays(samples)
    want = np.stack([oracle_render(oracle_net(n, delays, w, nin, nout, sr=K.SR_GENERIC), x[v], cuts, mode) for v in range(K.V)])
    return frozen(x), frozen(want)


def generic_case(gpu, n, w, nin, nout, samples, want_cap, T, cuts, layout, mode, full):
    delays = generic_delays(samples)
    lens, cap = K.ring_of(delays, K.SR_GENERIC)
    assert [int(v) - 1 for v in lens] == list(samples)
    check_edges(lens, cap, want_cap, full)
    b = gpu.Bank.fdn(K.V, n, delays, len(w), w, nin, nout)      # created at DEFAULT_SR == SR_GENERIC, and it stays there
    assert b.sample_rate == K.SR_GENERIC and b.inputs() == nin and b.outputs() == nout
    x, want = generic_reference(n, w, nin, nout, tuple(samples), T, cuts, mode)
    got = run(b, x, layout, mode, list(cuts))
    check_render(b, x, got, want, layout, mode, f"generic <{n}, {len(w)}> {nin}->{nout} cap {cap}")


GENERIC_ROWS = [(r, layout) for r in K.GENERIC_CASES for layout in layouts_of(r[1])]
GENERIC_IDS = [f"{r[0]}-{r[1]}-{r[3]}to{r[4]}-{'planar' if l == LAYOUT_PLANAR else 'voiceminor'}" for r, l in GENERIC_ROWS]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row,layout", GENERIC_ROWS, ids=GENERIC_IDS)
def test_generic_kernel_on_the_short_ring(gpu, row, layout, mode):
    n, taps, w, nin, nout = row
    generic_case(gpu, n, w, nin, nout, K.short_ring(n), 256, K.T, K.CUTS, layout, mode, True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row", K.STEP_GENERIC, ids=[f"{r[0]}-{r[1]}-{r[5]}" for r in K.STEP_GENERIC])
def test_generic_kernel_at_the_capacity_step(gpu, row, mode):
    n, taps, w, nin, nout, second = row
    samples = K.step_ring(n, second)
    generic_case(gpu, n, w, nin, nout, samples, 512, K.T_STEP, K.CUTS_STEP, LAYOUT_PLANAR, mode, max(samples) == 511)


# ---- the filtered kernel -----------------------------------------------------------------------------------------------------------------
def filtered_params(n, taps, filt, gain, per, samples):
    k = K.per_instance_samples(samples) if per else np.asarray(samples)
    return params(n, K.V, filt, taps, gain, per, 500 + 3 * n + taps, delay_samples=k), k


@functools.lru_cache(maxsize=None)
def filtered_reference(n, taps, filt, place, gain, per, nin, nout, samples, T, cuts, mode):
    x = matrix_signal(nin, T, 700 + 11 * n + taps)
    p, _ = filtered_params(n, taps, filt, gain, per, samples)
    want = np.stack([oracle_render(oracle_network(n, p, v, place, nin, nout), x[v], cuts, mode) for v in range(K.V)])
    return frozen(x), frozen(want)


def filtered_case(gpu, n, taps, filt, place, gain, per, nin, nout, samples, want_cap, T, cuts, layout, mode, full):
    p, k = filtered_params(n, taps, filt, gain, per, samples)
    lens, cap = K.ring_of(p["delays"], K.SR)
    assert np.array_equal(lens - 1, k)
    check_edges(lens, cap, want_cap, full)
    if per:   # both edges in one launch: an instance with every line at 128 samples, another with the line that fills the shared capacity
        assert np.all(lens[K.ALL_SHORTEST] == K.SHORTEST + 1) and int(lens[0].max()) == cap
    b = gpu.Bank.fdn_network(K.V, n, place=place, inputs=nin, outputs=nout, sample_rate=K.SR, **p)
    assert b.kind == "fdn_network" and b.inputs() == nin and b.outputs() == nout
    x, want = filtered_reference(n, taps, filt, place, gain, per, nin, nout, tuple(samples), T, cuts, mode)
    got = run(b, x, layout, mode, list(cuts))
    check_render(b, x, got, want, layout, mode, f"filtered <{n}, {taps}> {filt} {place} gain {gain} per-instance {per} {nin}->{nout} cap {cap}")


FILTERED_ROWS = [(r, layout) for r in K.FILTERED_CASES for layout in layouts_of(r[1])]
FILTERED_IDS = [f"{r[0]}-{r[1]}-{r[2]}-{r[3]}-{'gain' if r[4] else 'nogain'}-{'per' if r[5] else 'shared'}-{'planar' if l == LAYOUT_PLANAR else 'voiceminor'}"
                for r, l in FILTERED_ROWS]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row,layout", FILTERED_ROWS, ids=FILTERED_IDS)
def test_filtered_kernel_on_the_short_ring(gpu, row, layout, mode):
    n, taps, filt, place, gain, per, nin, nout = row
    filtered_case(gpu, n, taps, filt, place, gain, per, nin, nout, K.short_ring(n), 256, K.T, K.CUTS, layout, mode, True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row", K.STEP_FILTERED, ids=[f"{r[0]}-{r[1]}-{r[8]}" for r in K.STEP_FILTERED])
def test_filtered_kernel_at_the_capacity_step(gpu, row, mode):
    n, taps, filt, place, gain, per, nin, nout, second = row
    samples = K.step_ring(n, second)
    filtered_case(gpu, n, taps, filt, place, gain, per, nin, nout, samples, 512, K.T_STEP, K.CUTS_STEP, LAYOUT_PLANAR, mode, max(samples) == 511)


# ---- the refusals at the boundary --------------------------------------------------------------------------------------------------------
def test_a_line_of_127_samples_is_refused_and_128_is_the_boundary(gpu):
    n, w = 4, (0.55, 0.4)
    short = K.short_ring(n)
    short[2] = K.SHORTEST - 1                                                 # len = 128
    assert int(K.ring_of(generic_delays(short), K.SR_GENERIC)[0].min()) == 128
    with pytest.raises(gpu.FdspError, match="128 samples"):
        gpu.Bank.fdn(K.V, n, generic_delays(short), len(w), w)
    p = params(n, K.V, "lowpole", 2, True, False, 1, delay_samples=short)
    assert int(K.ring_of(p["delays"], K.SR)[0].min()) == 128
    with pytest.raises(gpu.FdspError, match="128 samples"):
        gpu.Bank.fdn_network(K.V, n, place="loop", sample_rate=K.SR, **p)
    # (the same banks with that line at 128 samples are rows of the short-ring tests above; here they are only built)
    short[2] = K.SHORTEST
    assert gpu.Bank.fdn(K.V, n, generic_delays(short), len(w), w).inputs() == 1
    assert gpu.Bank.fdn_network(K.V, n, place="loop", sample_rate=K.SR, **params(n, K.V, "lowpole", 2, True, False, 1, delay_samples=short)).inputs() == 1


@pytest.mark.parametrize("family", ["generic", "filtered"])
def test_a_rate_that_takes_128_samples_to_127_is_refused_and_the_bank_stays(gpu, family):
    """127.4 / 128 of the rate: the 128-sample line would hold 127 samples.  The bank refuses and goes on at the old rate, sample for sample
    like a twin that was never asked -- in mid-stream, so the rings, the FIR carry and the feedback value must all have stayed."""
    n, w, T = 4, (0.55, 0.4), 64 * 9 + 13
    samples = K.short_ring(n)
    if family == "generic":
        sr = K.SR_GENERIC
        mk = lambda: gpu.Bank.fdn(K.V, n, generic_delays(samples), len(w), w)
        delays = generic_delays(samples)
    else:
        sr = K.SR
        p = params(n, K.V, "lowpole", 2, True, False, 1, delay_samples=samples)
        mk = lambda: gpu.Bank.fdn_network(K.V, n, place="loop", sample_rate=sr, **p)
        delays = p["delays"]
    lower = sr * 127.4 / 128.0
    assert int(K.ring_of(delays, lower)[0].min()) == 128 and int(K.ring_of(delays, sr)[0].min()) == 129
    a, twin = mk(), mk()
    x = signal(K.V, 1, T, 91, impulse=K.IMPULSE)
    cut = 64 * 3 + 7
    a1 = run(a, x[:, :, :cut], LAYOUT_PLANAR, MODE_PROCESS, [0, cut])
    t1 = run(twin, x[:, :, :cut], LAYOUT_PLANAR, MODE_PROCESS, [0, cut])
    with pytest.raises(gpu.FdspError, match="128 samples"):
        a.set_sample_rate(lower)
    a2 = run(a, x[:, :, cut:], LAYOUT_PLANAR, MODE_PROCESS, [0, T - cut])
    t2 = run(twin, x[:, :, cut:], LAYOUT_PLANAR, MODE_PROCESS, [0, T - cut])
    assert np.abs(t2[K.IMPULSE]).max() > SOUNDS
    assert_bit_equal(np.concatenate([a1, a2], axis=2), np.concatenate([t1, t2], axis=2), f"{family}: after the refused rate")


# ---- the reverbs' kernel -----------------------------------------------------------------------------------------------------------------
REVERB_ROWS = [(r[:4], m) for r in K.REVERB_CASES for m in ([MODE_PROCESS, MODE_TICK] if r[4] else [MODE_PROCESS])]
REVERB_IDS = [f"{'reverb_stereo' if r[0] == 1 else 'reverb4_stereo'}-cap2^{r[1]}-{'process' if m == MODE_PROCESS else 'tick'}" for r, m in REVERB_ROWS]


@pytest.mark.parametrize("row,mode", REVERB_ROWS, ids=REVERB_IDS)
def test_reverb_kernel_at_every_ring_capacity(gpu, row, mode):
    nsec, log2, room, sr = row
    cap = 1 << log2
    lens = K.reverb_lens(nsec, room, sr)
    assert cap // 2 < int(lens.max()) <= cap and int(lens.min()) > 128          # the longest line picks this capacity; the 128-sample rule
    assert int(K.reverb_lens(nsec, room, O.DEFAULT_SR).min()) > 128            # (the bank is created at DEFAULT_SR and then moved)
    cuts = K.reverb_cuts(cap)
    V, T = K.REVERB_V, cuts[-1]
    x = (np.random.default_rng(1000 * nsec + log2).random((V, 2, T), dtype=np.float32) * 2 - 1).astype(np.float32)
    time = K.reverb_time(nsec, room)
    if nsec == 1:
        b = gpu.Bank.reverb_stereo(V, room, time, K.REVERB_DAMPING)
        net = lambda: O.reverb_stereo(room, time, K.REVERB_DAMPING)
    else:
        b = gpu.Bank.reverb4_stereo(V, room, time)
        net = lambda: O.reverb4_stereo(room, time)
    b.set_sample_rate(sr)
    got = run(b, x, LAYOUT_PLANAR, mode, list(cuts))
    assert b.get_option("last_kernel") == 6
    assert np.isfinite(got).all() and np.abs(got[:, :, cap:]).max() > SOUNDS     # what the longest line delayed by a whole ring sounds
    for v in range(V):
        o = net()
        o.set_sample_rate(sr)
        assert_bit_equal(got[v], oracle_render(o, x[v], cuts, mode), f"NSEC {nsec} cap 2^{log2} room {room} at {sr} Hz instance {v}")
