"""The launch protocol every render entry point of the C ABI follows (fd_capi.hip `Launch`): the per-launch event pair follows "timing", a
launch refused with FDSP_ENOTSUP leaves no event pair to read and the bank where it was, a render on the bank's stream is ordered behind one
on a caller's stream whatever the entry point, and the sequencer clock is the reference's own f64 additions however a launch is cut.

Entry points: process, process_mix (voice bank and reverb effect bank), process_events, process_events_mix, reverb_fitness.  Shapes: the
smallest that cross a voice group and a block."""
import math

import numpy as np
import pytest

from fundsp_amd import MIX_SUM, MODE_TICK
from fundsp_amd import workloads as W
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
SR = 48000.0
V, T = 64 + 21, 64 + 9
FX_V = 3


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def voice_bank():
    """fm_svf voices with one event each: fades running in both blocks of a T-frame launch, some voices silent at either end"""
    p = W.fm_svf_params(V, SR)
    b = W.make_fm_svf_bank(V, SR, params=p)
    start = (np.arange(V) % 50).astype(np.float64)
    b.set_events(start / SR, (start + 100.0) / SR, 8.0 / SR, 8.0 / SR)
    return b, p


def fx_bank(gpu):
    import torch

    b = gpu.Bank.reverb_stereo(FX_V, 10.0, 1.0, 0.5)
    b.set_sample_rate(SR)
    rng = np.random.default_rng(5)
    x = torch.from_numpy((rng.random((2, T, FX_V), dtype=np.float32) * 2 - 1).astype(np.float32)).cuda()
    return b, x


def launches(gpu):
    """(name, bank, launch) for every entry point the binding reaches; `timed`: the launch leaves an event pair when "timing" is on"""
    vb, _ = voice_bank()
    fx, x = fx_bank(gpu)
    return [
        ("process", vb, lambda: vb.process(T), True),
        ("process_mix", vb, lambda: vb.process_mix(T, mix=MIX_SUM), True),
        ("process_mix (reverb)", fx, lambda: fx.process_mix(T, x, mix=MIX_SUM), True),
        ("process_events", vb, lambda: vb.process_events(T), True),
        ("process_events_mix", vb, lambda: vb.process_events_mix(T), True),
        # several launches around an event pair of its own ("fitness_score_us"): never one to read here, whatever "timing" says
        ("reverb_fitness", fx, lambda: fx.reverb_fitness(), False),
    ]


def test_the_event_pair_follows_the_timing_option(gpu):
    import torch

    for name, b, launch, timed in launches(gpu):
        b.set_option("timing", 0)
        launch()
        with pytest.raises(gpu.FdspError):
            b.last_kernel_ms()
        b.set_option("timing", 1)
        launch()
        if timed:
            ms = b.last_kernel_ms()
            assert math.isfinite(ms) and ms >= 0.0, (name, ms)
        else:
            with pytest.raises(gpu.FdspError):
                b.last_kernel_ms()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def wide_bank(gpu):
    """A graph of four outputs with an event per voice: too wide for a fused mix-down, told the way
    test_gpu_mix.test_run_time_compiled_wide_graph_has_no_fused_mix_and_says_so tells it ("has_fused_mix" = 0), and more than the two
    outputs a fused Sequencer mix takes.  The tests below work on clones."""
    from fundsp_amd import graph as G

    b = gpu.Bank.from_graph(G.sine_hz(110.0) | G.sine_hz(220.0) | G.sine_hz(330.0) | G.noise(), V, sample_rate=SR)
    b.set_seed(np.arange(V, dtype=np.uint64) * 31 + 7)
    start = (np.arange(V) % 50).astype(np.float64)
    b.set_events(start / SR, (start + 100.0) / SR, 8.0 / SR, 8.0 / SR)
    assert b.outputs() == 4 and b.get_option("has_fused_mix") == 0
    return b


@pytest.mark.parametrize("entry", ["process_mix", "process_events_mix"])
def test_a_refused_launch_leaves_no_event_pair_and_the_bank_alone(gpu, wide_bank, entry):
    from fundsp_amd._lib import ENOTSUP

    refused = {"process_mix": lambda c: c.process_mix(T, mix=MIX_SUM), "process_events_mix": lambda c: c.process_events_mix(T)}[entry]
    hit, untouched = wide_bank.clone(), wide_bank.clone()
    hit.set_option("timing", 1)
    with pytest.raises(gpu.FdspError) as e:
        refused(hit)
    assert e.value.code == ENOTSUP, e.value
    with pytest.raises(gpu.FdspError):   # no launch happened: there is no event pair to read
        hit.last_kernel_ms()
    assert hit.events_time() == untouched.events_time()
    assert_bit_equal(host(hit.process(T)), host(untouched.process(T)), f"{entry}: a refused launch leaves the bank alone")


@pytest.mark.parametrize("family", ["plain", "mix", "events"])
def test_the_banks_stream_waits_for_a_render_on_a_caller_stream(gpu, family):
    """Render on a caller's stream, reset() with no synchronize in between, render on the bank's own stream: the reset cannot overtake the
    first render, nor the second render the reset, so the second output is a fresh bank's first."""
    import torch

    b, p = voice_bank()
    render = {"plain": lambda c: c.process(T), "mix": lambda c: c.process_mix(T, mix=MIX_SUM), "events": lambda c: c.process_events(T)}[family]
    want = host(render(b.clone()))
    s = torch.cuda.Stream()   # non-blocking: no implicit ordering with the bank's stream
    with torch.cuda.stream(s):
        render(b)
    b.reset()
    b.set_seed(p["seed"])
    b.events_rewind(0.0)
    got = host(render(b))     # the current stream is the default one here: the launch runs on the bank's own
    assert_bit_equal(got, want, f"{family}: second render, on the bank's stream")


def f64_bits(x):
    return np.float64(x).tobytes()


def reference_clock(blocks):
    """Sequencer::process / tick (sequencer.rs): time += sample_duration * size once per block, time += sample_duration once per tick"""
    sd, t = np.float64(1.0) / np.float64(SR), np.float64(0.0)
    for n in blocks:
        t = t + sd * np.float64(n)
    return t


def test_the_clock_is_the_references_additions_however_a_launch_is_cut(gpu):
    whole, _ = voice_bank()
    cut = whole.clone()
    whole.process_events(64 * 2 + 9)
    cut.process_events(64)
    cut.process_events(64 + 9)
    assert f64_bits(whole.events_time()) == f64_bits(cut.events_time())
    assert f64_bits(whole.events_time()) == f64_bits(reference_clock([64, 64, 9]))
    mixed = cut.clone()
    mixed.events_rewind(0.0)
    mixed.process_events_mix(64 * 2 + 9)
    assert f64_bits(mixed.events_time()) == f64_bits(whole.events_time())
    tick, _ = voice_bank()
    tick.process_events(9, mode=MODE_TICK)
    assert f64_bits(tick.events_time()) == f64_bits(reference_clock([1] * 9))
    assert f64_bits(tick.events_time()) != f64_bits(reference_clock([9])), "nine additions and one multiplication round differently at this rate"
    host(tick.process(1))   # (the launches above have run)
