"""Every instantiation of the feedback delay kernel k_fb_frames<NL, K> (fd_fbdelay.hip), on the edges of the ring and at every ring capacity,
bit for bit against the oracle's generic Feedback / Feedback2 tree built per instance.  The tables are feedback_delay_cases.py (checked
without a device by test_feedback_delay_cases.py, which also holds the oracle alone to every side condition asked of the device here):

(a) all eight instantiations twice on the SHORT RING (256 slots): a line of 128 samples -- the shortest legal delay -- and one of 255
    (len == cap); 1 933 frames in launches of 64, 77, 1, 333, 768 and 690, so the write window wraps seven times and the ragged launches walk
    the mirror zone slot by slot.  The per-instance rows put into ONE launch the line that fills the shared capacity (instance 0), the two
    delays whose reads reach the highest mirror slot any read reaches (143 and 207 samples, instances 1 and 2) and an instance with every line
    at 128.  Five instances: plain noise, noise in the denormal range, a unit impulse on every channel, (per instance) all lines shortest,
    and noise that sinks from 1e-35 to 1e-38 -- every product `w * d`, `g * f` of every row crosses the flush threshold somewhere, which is
    where a contracted fma or an operation compiled without flush-to-zero would differ from the oracle.
(b) the capacity step: 256 samples (len = 257, the first length that takes 512 slots) and 511 (len == cap), mirror-top delays 220 and 399.
(c) every ring capacity 2^8 .. 2^18 with k_fb_frames<2, 3>, cap + 205 frames cut inside the block whose write window wraps; and
    k_fdn_frames_filtered, which takes its capacity at run time the same way, at 2^10, 2^14 and -- 32 lines, the largest ring allocation
    either family can make -- 2^18.
(d) a change of rate that would take the 128-sample line to 127 is refused and leaves the bank as it was, in mid-tail.
(e) every bus shape of test_gpu_reverb_bus.BUSES set by hand, against the oracle's whole graph; clone and reset with the bus.
(f) block launches captured into a HIP graph and replayed.

No tolerance appears in this file."""
import numpy as np
import pytest

import fdn_frames_cases as K
import feedback_delay_cases as FC
import oracle as O
import test_gpu_feedback_delay as FD
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from test_gpu_parity import assert_bit_equal
from test_gpu_reverb_bus import BUSES

pytestmark = pytest.mark.gpu
# A tail that "still sounds" is one of normal numbers with all 24 bits of mantissa in play: anything above 1e-9 is 29 decades over the flush
# threshold.  (test_feedback_delay_cases.py asks 1e-7 of the oracle's samples, to which the device's are then equal.)
SOUNDS = 1e-9
LAYOUT_NAMES = {LAYOUT_PLANAR: "planar", LAYOUT_VOICE_MINOR: "voiceminor"}
SHORT_MONO_TICK, SHORT_STEREO_TICK = 6, 13      # rows of (a) that also run with FDSP_MODE_TICK: <1, 3> and <2, 2>, both per instance
BUS_MONO, BUS_STEREO = 4, 13                    # rows of (a) under the bus: <1, 2> line lowpole, both gains | <2, 2> loop, reversed, per instance
CAPTURE_ROW = 12                                # <2, 2> line, both gains, reversed, one table row for the bank (any number of instances)


def check_row(gpu, table, index, layout, mode):
    rows, cap_claimed, T, cuts = FC.TABLES[table]
    N, rev, place, filt, taps, lg, og, delays = rows[index]
    p, x, want = FC.reference(table, index, mode)
    lens, cap = FC.row_ring(p)
    assert cap == cap_claimed and np.array_equal(lens - 1, np.asarray(delays)) and K.SHORTEST + 1 <= int(lens.min()) and int(lens.max()) <= cap
    if N == 2 or FC.is_per(delays):
        assert int(lens.min()) == K.SHORTEST + 1
    if FC.is_per(delays):
        assert np.all(lens[K.ALL_SHORTEST] == K.SHORTEST + 1) and int(lens[0].max()) == cap
    what = f"{table} {FC.row_id(rows[index])} {LAYOUT_NAMES[layout]} mode {mode}"
    b = FD.make(gpu, p, FC.V)
    got = FD.run(b, x, layout, mode, list(cuts))
    assert b.get_option("last_kernel") == 6
    for v in range(FC.V):
        assert_bit_equal(got[v], want[v], f"{what} instance {v}")
    assert np.isfinite(got).all()
    assert np.abs(got[K.IMPULSE][:, 2 * T // 3:]).max() > SOUNDS                      # the impulse still recirculates: no tail of zeros
    assert not np.any((got != 0) & (np.abs(got) < FC.SMALLEST_NORMAL))                # this translation unit flushes: no subnormal in any instance
    b.reset()
    assert_bit_equal(FD.run(b, x[:, :, :K.RESET_FRAMES], layout, mode, [0, K.RESET_FRAMES]), got[:, :, :K.RESET_FRAMES], f"{what} after reset")
    return got


MATRIX_ROWS = [(t, i, l) for t in ("short", "step") for i, r in enumerate(FC.TABLES[t][0]) for l in ([LAYOUT_PLANAR, LAYOUT_VOICE_MINOR] if r[4] == 3 else [LAYOUT_PLANAR])]
MATRIX_IDS = [f"{t}-{FC.row_id(FC.TABLES[t][0][i])}-{LAYOUT_NAMES[l]}" for t, i, l in MATRIX_ROWS]


@pytest.mark.parametrize("table,index,layout", MATRIX_ROWS, ids=MATRIX_IDS)
def test_every_instantiation_on_the_short_ring_and_at_the_capacity_step(gpu, table, index, layout):
    check_row(gpu, table, index, layout, MODE_PROCESS)


@pytest.mark.parametrize("index", [SHORT_MONO_TICK, SHORT_STEREO_TICK], ids=["mono", "stereo"])
def test_tick_mode_is_the_same_arithmetic(gpu, index):
    """the family has one arithmetic for both executors: the oracle's tick render, and the same bits as its block render"""
    got = check_row(gpu, "short", index, LAYOUT_PLANAR, MODE_TICK)
    assert_bit_equal(got, FC.reference("short", index, MODE_PROCESS)[2], "FDSP_MODE_TICK vs the oracle's block render")


# ---- (c) every ring capacity ----------------------------------------------------------------------------------------------------------------
def check_ladder(bank, x, want, cap, what):
    cuts = K.reverb_cuts(cap)
    got = FD.run(bank, x, LAYOUT_PLANAR, MODE_PROCESS, list(cuts))
    assert bank.get_option("last_kernel") == 6
    for v in range(FC.LADDER_V):
        assert_bit_equal(got[v], want[v], f"{what} instance {v}")
    assert np.isfinite(got).all() and np.abs(got[:, :, cap:]).max(axis=2).min() > SOUNDS   # what the longest line delayed by a whole ring sounds, in every channel


@pytest.mark.parametrize("log2", FC.LADDER, ids=[f"cap2^{k}" for k in FC.LADDER])
def test_feedback_delay_kernel_at_every_ring_capacity(gpu, log2):
    p, x, want = FC.ladder_reference(log2)
    lens, cap = FC.row_ring(p)
    assert cap == 1 << log2 and list(lens) == [K.SHORTEST + 1, cap]
    check_ladder(FD.make(gpu, p, FC.LADDER_V), x, want, cap, f"k_fb_frames<2, 3> cap 2^{log2}")


@pytest.mark.parametrize("index", range(len(FC.NETWORK_LADDER)), ids=[f"cap2^{r[0]}-{r[1]}lines" for r in FC.NETWORK_LADDER])
def test_filtered_network_kernel_on_the_large_rings(gpu, index):
    log2, lines, filt, place, taps, gain, nin, nout = FC.NETWORK_LADDER[index]
    p, x, want = FC.network_reference(index)
    lens, cap = K.ring_of(p["delays"], FC.SR)
    assert cap == 1 << log2 and int(lens.min()) == K.SHORTEST + 1 and int(lens.max()) == cap and len(lens) == lines
    b = gpu.Bank.fdn_network(FC.LADDER_V, lines, place=place, inputs=nin, outputs=nout, sample_rate=FC.SR, **p)
    assert b.kind == "fdn_network" and b.inputs() == nin and b.outputs() == nout
    check_ladder(b, x, want, cap, f"k_fdn_frames_filtered<{lines}, {taps}> cap 2^{log2}")


# ---- (d) the refusal at the boundary -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [7, 12], ids=["mono", "stereo"])
def test_a_rate_that_takes_128_samples_to_127_is_refused_and_the_bank_stays(gpu, index):
    """127.4 / 128 of the rate: the 128-sample line would hold 127 samples.  The bank refuses and goes on at the old rate, sample for sample
    like a twin that was never asked -- in mid-tail, so the rings, the FIR carry, the filter state and the feedback value must all have stayed."""
    N = FC.SHORT[index][0]
    p = FC.row_params("short", index)
    lower = FC.SR * 127.4 / 128.0
    assert int(K.ring_of(p["delays"], lower)[0].min()) == 128 and int(K.ring_of(p["delays"], FC.SR)[0].min()) == 129
    a, twin = FD.make(gpu, p, FC.V), FD.make(gpu, p, FC.V)
    T, cut = 64 * 9 + 13, 64 * 3 + 7
    x = FC.matrix_signal(N, T, 91)
    a1 = FD.run(a, x[:, :, :cut], LAYOUT_PLANAR, MODE_PROCESS, [0, cut])
    t1 = FD.run(twin, x[:, :, :cut], LAYOUT_PLANAR, MODE_PROCESS, [0, cut])
    with pytest.raises(gpu.FdspError, match="128 samples"):
        a.set_sample_rate(lower)
    a2 = FD.run(a, x[:, :, cut:], LAYOUT_PLANAR, MODE_PROCESS, [0, T - cut])
    t2 = FD.run(twin, x[:, :, cut:], LAYOUT_PLANAR, MODE_PROCESS, [0, T - cut])
    assert np.abs(t2[K.IMPULSE]).max() > SOUNDS
    assert_bit_equal(np.concatenate([a1, a2], axis=2), np.concatenate([t1, t2], axis=2), "after the refused rate")
    assert_bit_equal(t2[0], FD.oracle_render(FD.oracle_net(p, 0), x[0], [0, cut, T])[:, cut:], "the twin is the oracle's")


# ---- (e) the bus, set by hand ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bus", list(BUSES))
@pytest.mark.parametrize("index", [BUS_MONO, BUS_STEREO], ids=["mono", "stereo_reversed"])
def test_set_bus_by_hand_equals_the_oracles_whole_graph(gpu, index, bus):
    """fdsp_bank_set_bus with each shape the reference's documentation gives a reverb, folded into the kernel's epilogue: pass() / multipass(2),
    `&` and `*` around the tree in the oracle.  Both layouts, the ragged launches of the short ring, and clone and reset with the bus."""
    N = FC.SHORT[index][0]
    T, cuts = FC.SHORT_T, list(FC.SHORT_CUTS)
    p, x, _plain = FC.reference("short", index)
    shape, (mode, wet, dry) = BUSES[bus]

    def whole(v):
        n = shape(O, FD.build(O, p, v), O.pass_() if N == 1 else O.multipass(2))
        n.set_sample_rate(FC.SR)
        return n

    want = np.stack([FD.oracle_render(whole(v), x[v], cuts) for v in range(FC.V)])
    b = FD.make(gpu, p, FC.V)
    b.set_bus(mode, float(wet), float(dry))
    assert b.get_bus() == (mode, float(wet), float(dry))
    got = FD.run(b, x, LAYOUT_PLANAR, MODE_PROCESS, cuts)
    assert b.get_option("last_kernel") == 6
    for v in range(FC.V):
        assert_bit_equal(got[v], want[v], f"{bus} around {FC.row_id(FC.SHORT[index])} planar instance {v}")
    assert np.abs(got[K.IMPULSE][:, 2 * T // 3:]).max() > SOUNDS and np.any(got != _plain)
    b.reset()                               # reset keeps the bus; the clone carries it and continues alike, in the other layout
    at = cuts[4]
    first = FD.run(b, x[:, :, :at], LAYOUT_VOICE_MINOR, MODE_PROCESS, cuts[:5])
    twin = b.clone()
    assert twin.get_bus() == b.get_bus()
    rest = FD.run(b, x[:, :, at:], LAYOUT_VOICE_MINOR, MODE_PROCESS, [0, cuts[5] - at, T - at])
    assert_bit_equal(np.concatenate([first, rest], axis=2), want, f"{bus}: after reset, voice-minor")
    assert_bit_equal(FD.run(twin, x[:, :, at:], LAYOUT_PLANAR, MODE_PROCESS, [0, T - at]), want[:, :, at:], f"{bus}: the clone, planar, one launch")


# ---- (f) stream capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout_name", ["voice_minor_staged", "planar"])
def test_block_launches_captured_into_a_hip_graph(gpu, layout_name):
    """five 64-frame launches of k_fb_frames<2, 2> recorded once and replayed twice equal one uncaptured render of 640 frames -- planar, and with
    voice-minor buffers through the bank's planar staging copy (64 instances or more; sized by a launch before the capture)"""
    import torch

    V, NB = 80, 5
    p = FC.row_params("short", CAPTURE_ROW)
    assert FC.SHORT[CAPTURE_ROW][:2] == (2, True) and FC.SHORT[CAPTURE_ROW][4] == 2 and not FC.is_per(FC.SHORT[CAPTURE_ROW][7])
    planar = layout_name == "planar"
    b, r = FD.make(gpu, p, V), FD.make(gpu, p, V)
    ints = lambda t: t.contiguous().view(torch.int32)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand((V, 2, 64 * NB * 2) if planar else (2, 64 * NB * 2, V), device="cuda", generator=g) * 2 - 1
    kw = dict(layout=LAYOUT_PLANAR, frame_stride=64) if planar else dict(layout=LAYOUT_VOICE_MINOR)
    want = r.process(64 * NB * 2, x, **(dict(layout=LAYOUT_PLANAR, frame_stride=64 * NB * 2) if planar else kw))
    ins = [torch.empty((V, 2, 64) if planar else (2, 64, V), device="cuda") for _ in range(NB)]
    outs = [torch.empty_like(t) for t in ins]
    s = torch.cuda.Stream()
    chunks = []
    with torch.cuda.stream(s):
        ins[0].zero_()
        b.process(64, ins[0], out=outs[0], **kw)        # loads the kernel and sizes the staging buffer before the capture ...
        b.reset()                                        # ... and leaves no trace: silence through zeroed rings, then reset
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            for k in range(NB):
                b.process(64, ins[k], out=outs[k], **kw)
        for rep in range(2):
            for k in range(NB):
                sl = slice((rep * NB + k) * 64, (rep * NB + k + 1) * 64)
                ins[k].copy_(x[:, :, sl] if planar else x[:, sl, :])
            gr.replay()
            chunks.append(torch.cat(outs, dim=2 if planar else 1).clone())
        torch.cuda.synchronize()
    got = torch.cat(chunks, dim=2 if planar else 1)
    assert torch.equal(ints(got), ints(want))
    tail = want[:, :, 64 * NB:] if planar else want[:, 64 * NB:, :]
    assert float(tail.abs().max()) > 1e-3 and b.get_option("last_kernel") == 6
    # ... and the replayed samples are the oracle's (instance 0 and the last one, which sits in the ragged second tile of the staging copy)
    xh = (x if planar else x.permute(2, 0, 1)).cpu().numpy()
    gh = (got if planar else got.permute(2, 0, 1)).cpu().numpy()
    for v in (0, V - 1):
        assert_bit_equal(gh[v], FD.oracle_net(p, 0).render_blocks(np.ascontiguousarray(xh[v])), f"captured and replayed, instance {v}")
