"""The device's reverb_fitness (k_fit_terms, k_fit_combine of fundsp_amd/csrc/fd_fitness.hip) BIT FOR BIT against fitness_device_order
(tests/reverb_fitness_ref.py), the numpy restatement of the order fd_fitness.hpp states -- every term and the total, as uint32.

tests/test_gpu_reverb_fitness.py holds the same call to fitness_f64 within a yardstick of 4 * delta (1e-5 and more on a term): room in which
a loop bound off by one, the impulse sample counted or the last bin dropped all fit.  Here nothing fits: the crafted responses of
tests/reverb_fitness_cases.py (fed through a per-instance convolver bank, whose impulse response is its taps up to f32 rounding; a twin bank
shows the very samples the call scores, and the cases' conditions are asserted on those), the natural banks of test_gpu_reverb_fitness on the
oracle's responses, a search step (set_delays on two rows of five), and a call on a side stream with a render queued straight behind it.
Every comparison in this file is an equality of bits; tests/test_reverb_fitness_order_host.py shows on the CPU that each single fault of the
order changes the bits of one of the crafted cases."""
import functools

import numpy as np
import pytest

import oracle as O
import resynth_ref
import reverb_fitness_cases as K
from fundsp_amd import LAYOUT_PLANAR, MODE_PROCESS
from reverb_fitness_ref import echo_weights, fitness_device_order
from test_gpu_parity import assert_bit_equal
from test_gpu_reverb_fitness import N, banks, responses, scores, tables

pytestmark = pytest.mark.gpu
TERMS = ("echo_0", "pen_0", "echo_1", "pen_1", "total")


@functools.lru_cache(maxsize=None)
def tabs():
    return resynth_ref.tables(N, O.lib().o_math_cosf)


_WANT = {}


def restated(r):
    """uint32 [5] = echo_0, pen_0, echo_1, pen_1, total of fitness_device_order, once per distinct response"""
    if id(r) not in _WANT:
        fit, terms = fitness_device_order(r, *tabs())
        _WANT[id(r)] = (r, np.concatenate([terms, [fit]]).astype(np.float32).view(np.uint32))
    return _WANT[id(r)][1]


def device_bits(fit, terms):
    """uint32 [V, 5] of a scores() result"""
    return np.concatenate([terms, fit[:, None]], axis=1).astype(np.float32).view(np.uint32)


def mismatches(label, got, want):
    out = []
    for q in range(5):
        if got[q] != want[q]:
            g, w = got[q:q + 1].view(np.float32)[0], want[q:q + 1].view(np.float32)[0]
            out.append(f"{label} {TERMS[q]}: device {g!r} ({got[q]:#010x}) restatement {w!r} ({want[q]:#010x}), {int(got[q]) - int(want[q]):+d} ulp")
    return out


def impulse(V):
    import torch

    x = torch.zeros((V, 2, N), dtype=torch.float32, device="cuda")
    x[:, :, 0] = 1.0
    return x


def test_crafted_responses_through_a_convolver_bank(gpu):
    import torch

    taps = K.taps()
    twin, bank = gpu.Bank.convolve(5, taps, per_instance=True), gpu.Bank.convolve(5, taps, per_instance=True)
    r = twin.process(N, impulse(5), layout=LAYOUT_PLANAR, frame_stride=N, mode=MODE_PROCESS)
    torch.cuda.synchronize()
    r = r.cpu().numpy()
    for v, name in enumerate(K.NAMES):
        counts = [len(echo_weights(r[v][c])) for c in range(2)]
        print(f"{name}: samples that count {counts} of {N - 1}; largest deviation from the taps {np.abs(r[v] - taps[v]).max():.3e}")
        K.check_conditions(name, r[v])
    got = device_bits(*scores(bank))
    bad = []
    for v, name in enumerate(K.NAMES):
        want = restated(r[v])
        print(f"{name}: device {got[v].view(np.float32)} restatement {want.view(np.float32)}")
        bad += mismatches(name, got[v], want)
    assert not bad, "\n".join(bad)
    z = K.NAMES.index("zero_left")
    assert not got[z][:2].any(), "zero_left: the terms of the silent channel are +0.0 exactly"
    t = got[K.NAMES.index("tones")].view(np.float32)
    assert t[1] > 0 and t[3] > 0 and abs(t[4]) > 1000.0 * (t[0] + t[2])
    s = got[K.NAMES.index("sparse")]
    assert not s[2:4].any(), "sparse: channel 1 holds the impulse sample alone, both its terms are +0.0"


def test_natural_banks_on_the_oracles_responses(gpu):
    bad = []
    for name, b in banks(gpu).items():
        got = device_bits(*scores(b))
        for v in range(3):
            bad += mismatches(f"{name}[{v}]", got[v], restated(responses()[name][v]))
    assert not bad, "\n".join(bad)


def test_a_search_step_rescoring_two_rows_of_five(gpu):
    d = tables()
    resp = responses()["reverb4_delays"]
    before, after = [0, 1, 2, 0, 1], [0, 2, 0, 0, 1]                # rows 1 and 2 take other candidates' tables
    b = gpu.Bank.reverb4_stereo_delays(5, d[before], 100.0)
    first = device_bits(*scores(b))
    b.set_delays(d[after[1:3]], first=1)
    second = device_bits(*scores(b))
    fresh = device_bits(*scores(gpu.Bank.reverb4_stereo_delays(5, d[after], 100.0)))
    for v in (0, 3, 4):
        assert np.array_equal(second[v], first[v]), f"row {v} was not set and lost its bits"
    for v in (1, 2):
        assert not np.array_equal(second[v], first[v]), f"row {v} was set and kept its score"
        assert np.array_equal(second[v], fresh[v]), f"row {v} after set_delays vs a fresh bank with the new tables"
    bad = []
    for v in range(5):
        bad += mismatches(f"before[{v}]", first[v], restated(resp[before[v]])) + mismatches(f"after[{v}]", second[v], restated(resp[after[v]]))
    assert not bad, "\n".join(bad)


def test_a_score_on_a_side_stream_with_a_render_queued_behind_it(gpu):
    """the call on a caller's stream, then process on the bank's own stream with no host synchronisation in between: the render is ordered
    behind the call's closing reset, and both give the bits of the synchronised runs"""
    import torch

    rng = np.random.default_rng(5)
    n = 64 * 60 + 7
    x = torch.from_numpy((rng.random((3, 2, n), dtype=np.float32) * 2 - 1).astype(np.float32)).cuda()
    ref = banks(gpu)["reverb4_delays"]
    want_score = device_bits(*scores(ref))
    want = ref.process(n, x, layout=LAYOUT_PLANAR, frame_stride=n)
    torch.cuda.synchronize()
    want = want.cpu().numpy()

    b = banks(gpu)["reverb4_delays"]
    b.fitness_reserve()
    out = torch.empty((3, 2, n), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert torch.cuda.current_stream().cuda_stream != side.cuda_stream
    fit, terms = b.reverb_fitness(terms=True, stream=side.cuda_stream)
    b.process(n, x, out=out, layout=LAYOUT_PLANAR, frame_stride=n)            # the bank's own stream
    torch.cuda.synchronize()
    got_score = device_bits(fit.cpu().numpy(), terms.cpu().numpy())
    assert np.array_equal(got_score, want_score), (got_score, want_score)
    assert_bit_equal(out.cpu().numpy(), want, "the render queued behind a side-stream fitness call vs the synchronised one")
    bad = []
    for v in range(3):
        bad += mismatches(f"side stream [{v}]", got_score[v], restated(responses()["reverb4_delays"][v]))
    assert not bad, "\n".join(bad)
