"""The rollback of the steady block (fd_seq_steps.hpp seq_steady_block: tripped(), back to the snapshot, the items redone frame by frame)
INSIDE the scheduler kernels.  tests/test_gpu_guard_bounds.py drives it for the render kernels; here the same edge rows -- phase sweeps
around the 2047-turn threshold, filter states up to 2^127, inf, NaN, cutoffs above Nyquist -- play as events and as a score of one note
per voice.  Banks of 128 and 100 FM voices (two voice groups, one ragged), T = 200 (three blocks and an 8-frame remainder), process
mode.  Every voice plays [0, (T + 50) / SR) without fades, except the last one, which fades in over 70 frames: the launch is not fully
sustained, so it takes the scheduler kernel; wave 0 takes the steady block in every block, wave 1 goes frame by frame through the two
blocks of the fade and is steady from there on.  Bit for bit, NaN == NaN."""
import numpy as np
import pytest

from fundsp_amd import MODE_PROCESS
from fundsp_amd import workloads as W
from test_gpu_guard_bounds import SR, make_bank, params_of, reference, voice_rows
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
T = 200
FADE_FRAMES = 70
LK_EVENTS, LK_SCORE = 5, 9


def windows(V):
    """(start, end, fade_in) of the V voices"""
    fin = np.zeros(V)
    fin[V - 1] = FADE_FRAMES / SR
    return np.zeros(V), np.full(V, (T + 50) / SR), fin


def voices_of(out):
    return out.cpu().numpy()[0].T            # [outputs, frames, V] -> [V][frames]


@pytest.mark.parametrize("V", [128, 100])
def test_events_render_the_edge_rows_like_the_oracle(gpu, V):
    """Events do not reset the unit: the banks carry the preset phases and filter states, and the voice-out is the oracle's -- but for
    the fade itself, frames 0 .. 127 of the last voice (the fade's 70 frames lie in the first two blocks)."""
    start, end, fin = windows(V)
    b = make_bank(voice_rows(V))
    b.set_events(start, end, fin, 0.0)
    with np.errstate(all="ignore"):
        got = voices_of(b.process_events(T, mode=MODE_PROCESS))
    assert b.get_option("last_kernel") == LK_EVENTS
    want = reference(V, [T])
    assert_bit_equal(got[:V - 1], want[:V - 1], f"events, V = {V}: every voice but the fading one")
    assert_bit_equal(got[V - 1, 128:], want[V - 1, 128:], f"events, V = {V}: the fading voice behind its fade's blocks")


@pytest.mark.parametrize("V", [128, 100])
def test_score_of_one_note_per_voice_equals_the_events(gpu, V):
    """The same windows as one note per voice without rows.  A begun note resets the unit, so the banks are built WITHOUT presets:
    reset() then changes nothing that set_events would have kept.  The rows' parameters alone (the sweeps around the 2047-turn
    threshold, the cutoffs above Nyquist) still trip the packed guard: with the restore of the snapshot taken out of seq_steady_block
    this case fails for both V, like the events case, while none of the older scheduler tests does."""
    start, end, fin = windows(V)
    p = params_of(voice_rows(V))
    a, b = W.make_fm_svf_bank(V, SR, params=p), W.make_fm_svf_bank(V, SR, params=p)
    a.set_events(start, end, fin, 0.0)
    b.set_score(np.arange(V), start, end, fin, 0.0)
    with np.errstate(all="ignore"):
        want = voices_of(a.process_events(T, mode=MODE_PROCESS))
        got = voices_of(b.process_events(T, mode=MODE_PROCESS))
    assert a.get_option("last_kernel") == LK_EVENTS and b.get_option("last_kernel") == LK_SCORE
    assert_bit_equal(got, want, f"score of one note per voice vs events, V = {V}")
    assert b.events_time() == a.events_time()
