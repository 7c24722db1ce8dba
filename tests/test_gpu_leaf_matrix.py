"""Every ahead-of-time leaf kind (register_leaf_kinds, fd_kinds_leaf.hip) in both executors and every layout, across launch boundaries, bit for bit
against the oracle.  make_kind<G> compiles k_render<G, MODE, LAYOUT, WPB> four times per kind (process / tick x voice-minor / planar) and the
pipeline kernels where the plan allows; the per-kind tests each pick one point of that matrix, at one full wave of voices, in one launch.  Here
the table is leaf_cases.py (checked without a device by test_leaf_cases.py, which also holds the oracle alone to every side condition):

(a) kind x executor x layout -- voice-minor, planar with padded 16-byte rows, planar with tight rows (frame_stride == launch length, so rows of 141,
    1 and 83 frames start unaligned) -- on 67 voices (a full wave and a wave of three lanes; voice 1 fed 1e-30): four launches of 141, 1, 64 and 83
    frames on one bank, so a node's state leaves the registers and comes back after a ragged remainder, a single frame and a whole block; a clone
    taken after the first launch; set_sample_rate(44 100) in mid-stream (the reference keeps filter state and empties delay lines); reset() and the
    first launch again.
(b) kind x executor: the same launches with "pipe_split" 0 (single-wave kernels: last_kernel == 1) and 2 (pipelines forced where the plan has one), in
    voice-minor and tight planar rows, against the default route.

No tolerance appears in this file: every comparison is assert_bit_equal."""
import numpy as np
import pytest

import leaf_cases as L
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
KINDS = list(L.TABLE)
LAYOUTS = ("voiceminor", "padded", "tight")
MODES = {"process": MODE_PROCESS, "tick": MODE_TICK}
PAD = 7.5       # what the padding of a planar output row holds before the launch, and after it
LK_SINGLE_WAVE = 1


def make_bank(gpu, row, pipe_split=None):
    if row.table:
        gpu.wavetable_build(row.table)      # the engine's own table (bit-identical to the oracle's: test_builtin_table_generator_matches_oracle_tables)
    b = gpu.Bank(row.kind, row.voices, ring_frames=row.ring_frames)
    if pipe_split is not None:
        b.set_option("pipe_split", pipe_split)
    row.configure(b, row.voices)
    assert b.inputs() == len(row.chans)
    return b


def launch(bank, x, a, b, layout, mode):
    """frames a .. b of x ([V][IN][T] or None) as one launch in `layout` -> [V][OUT][b - a].  (test_gpu_parity.run_bank fixes its own stride.)"""
    import torch

    frames, V, ni, no = b - a, bank.voices, bank.inputs(), bank.outputs()
    if layout == "voiceminor":
        inp = torch.from_numpy(np.ascontiguousarray(x[:, :, a:b].transpose(1, 2, 0))).cuda() if ni else None
        out = bank.process(frames, inp, layout=LAYOUT_VOICE_MINOR, mode=mode)
        torch.cuda.synchronize()
        return out.cpu().numpy().transpose(2, 0, 1)
    fs = frames if layout == "tight" else (frames + 63) // 64 * 64 + 64
    inp = None
    if ni:
        buf = np.zeros((V, ni, fs), dtype=np.float32)
        buf[:, :, :frames] = x[:, :, a:b]
        inp = torch.from_numpy(buf).cuda()
    out = torch.full((V, no, fs), PAD, dtype=torch.float32, device="cuda")
    bank.process(frames, inp, out=out, layout=LAYOUT_PLANAR, frame_stride=fs, mode=mode)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    # 16-byte aligned rows are stored in whole runs of four frames (fd_device.hpp: `fr + 4 <= ((size + 3) & ~3)`): up to three samples past the
    # launch, inside the row, are the kernel's; everything after that run is the caller's and stays
    assert (got[:, :, (frames + 3) // 4 * 4:] == PAD).all(), "a launch wrote past the 16-byte run that holds its last frame"
    assert layout != "tight" or got.shape[2] == frames
    return got[:, :, :frames]


def run(bank, x, spans, layout, mode):
    return np.concatenate([launch(bank, x, a, b, layout, mode) for a, b in spans], axis=2)


def assert_voices_equal(got, want, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    for v in range(got.shape[0]):
        assert_bit_equal(got[v], want[v], f"{what} voice {v}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("executor", L.EXECUTORS)
@pytest.mark.parametrize("kind", KINDS)
def test_leaf_kind_across_launches_clone_rate_change_and_reset(gpu, kind, executor, layout):
    row, mode = L.TABLE[kind], MODES[executor]
    x, want, again = L.reference(kind, executor)
    what = f"{kind} {executor} {layout}"
    end = L.CUTS[-1]
    b = make_bank(gpu, row)
    first = launch(b, x, *L.LAUNCHES[0], layout, mode)
    twin = b.clone()
    rest = run(b, x, L.LAUNCHES[1:], layout, mode)
    assert_voices_equal(np.concatenate([first, rest], axis=2), want[:, :, :end], f"{what}: launches of 141, 1, 64 and 83 frames,")
    assert_bit_equal(run(twin, x, L.LAUNCHES[1:], layout, mode), rest, f"{what}: the clone taken after the first launch")
    b.set_sample_rate(L.SR2)
    assert_voices_equal(launch(b, x, end, L.T_ALL, layout, mode), want[:, :, end:], f"{what}: after set_sample_rate({L.SR2:.0f}),")
    b.reset()
    b.set_sample_rate(L.SR)
    second = launch(b, x, *L.LAUNCHES[0], layout, mode)
    assert_voices_equal(second, again, f"{what}: after reset() and set_sample_rate({L.SR:.0f}),")
    if row.reset_restores:
        assert_bit_equal(second, first, f"{what}: the first launch again after reset()")


@pytest.mark.parametrize("executor", L.EXECUTORS)
@pytest.mark.parametrize("kind", KINDS)
def test_leaf_kind_on_every_dispatcher_route(gpu, kind, executor):
    row, mode = L.TABLE[kind], MODES[executor]
    x, want, _ = L.reference(kind, executor)
    default = run(make_bank(gpu, row), x, L.LAUNCHES, "voiceminor", mode)
    assert_voices_equal(default, want[:, :, :L.CUTS[-1]], f"{kind} {executor}: the default route, voice-minor,")
    for split in (0, 2):
        for layout in ("voiceminor", "tight"):
            b = make_bank(gpu, row, pipe_split=split)
            got = run(b, x, L.LAUNCHES, layout, mode)
            if split == 0:
                assert b.get_option("last_kernel") == LK_SINGLE_WAVE
            assert_bit_equal(got, default, f"{kind} {executor}: pipe_split {split} {layout} against the default route")
