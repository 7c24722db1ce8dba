"""reverb_fitness per instance on the device (fdsp_bank_reverb_fitness, Bank.reverb_fitness) against tests/reverb_fitness_ref.py on the
oracle's impulse responses.

The banks: three reverb4_stereo_delays candidates (time = 100.0 at 44.1 kHz, like examples/optimize.rs), reverb_stereo(10, 1, 0.5) and a
stereo fdn.  The response the call scores is the bank's PROCESS render of Impulse::<U2> over 32 768 frames; a twin bank fed the impulse
shows it, and it is the oracle's `impulse >> graph` bit for bit -- so the host restatements score the very same samples.

Yardstick (measured here, on the CPU, from the reference arithmetic alone): delta = the largest relative deviation of fitness_f32_serial --
the reference's own f32 order -- from fitness_f64, per term and for the total, over these responses, floored at 16 * 2^-24.  The device may
deviate from fitness_f64 by 4 * delta: another (fixed) summation order and the project's f32 FFT are f32 effects of the same size.

Measured on one MI355X (relative, per echo_0 pen_0 echo_1 pen_1 | total; test_terms_and_total_within_the_yardstick prints
them): delta 2.6e-6 1.2e-5 1.8e-6 1.1e-5 | 4.8e-5; the device's largest deviation 3.0e-8 1.4e-7 6.5e-8 1.7e-7 | 1.9e-7.

What is pinned how: the tolerance here says that the device's order computes reverb_fitness -- it is held to float64, a reference that shares
nothing with the kernel -- and leaves 1e-5 and more per term.  The arithmetic itself, all four terms and the total of these same banks and of
responses crafted for the loop bounds and the threshold, is pinned bit for bit by tests/test_gpu_reverb_fitness_bits.py against
reverb_fitness_ref.fitness_device_order, the restatement of fd_fitness.hpp's order; banks(), responses() and scores() are shared with it."""
import numpy as np
import pytest

import oracle as O
from fundsp_amd import LAYOUT_PLANAR, MODE_PROCESS, _lib
from reverb_fitness_ref import echo_weights, fitness_f32_serial, fitness_f64
from test_gpu_fdn import delays_of, oracle_net
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
N = 32768
SR = 44100.0
W2 = (0.55, 0.4)
FLOOR = 16.0 * 2.0 ** -24


def tables():
    rng = np.random.default_rng(2024)
    return (0.030 + 0.040 * rng.random((3, 32))).astype(np.float32)


def banks(gpu, V=3):
    d = tables()
    return {"reverb4_delays": gpu.Bank.reverb4_stereo_delays(V, d[np.arange(V) % 3], 100.0),
            "reverb_stereo": gpu.Bank.reverb_stereo(3, 10.0, 1.0, 0.5),
            "fdn": gpu.Bank.fdn(3, 8, delays_of(8), 2, W2, 2, 2)}


_RESP = {}


def responses():
    """the oracle's `Impulse::<U2> >> graph` over 32 768 frames per bank and instance, computed once and left unchanged"""
    if not _RESP:
        d = tables()

        def imp(node):
            node.set_sample_rate(SR)
            g = O.impulse(2) >> node
            g.set_sample_rate(SR)
            r = g.render_blocks(length=N)
            r.setflags(write=False)
            return r

        _RESP["reverb4_delays"] = [imp(O.reverb4_stereo_delays([float(x) for x in d[v]], 100.0)) for v in range(3)]
        _RESP["reverb_stereo"] = [imp(O.reverb_stereo(10.0, 1.0, 0.5))] * 3
        _RESP["fdn"] = [imp(oracle_net(8, delays_of(8), W2, 2, 2, sr=SR))] * 3
    return _RESP


_REF = {}


def host_scores():
    """(fitness_f64, fitness_f32_serial) of every distinct response"""
    if not _REF:
        for name, rs in responses().items():
            _REF[name] = [(fitness_f64(r), fitness_f32_serial(r)) for r in (rs if name == "reverb4_delays" else rs[:1])]
            if name != "reverb4_delays":
                _REF[name] = _REF[name] * 3
    return _REF


def rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / np.abs(np.asarray(b, dtype=np.float64))


def impulse_input():
    import torch

    x = torch.zeros((3, 2, N), dtype=torch.float32, device="cuda")
    x[:, :, 0] = 1.0
    return x


def scores(bank):
    import torch

    fit, terms = bank.reverb_fitness(terms=True)
    torch.cuda.synchronize()
    return fit.cpu().numpy(), terms.cpu().numpy()


def test_the_scored_response_is_the_oracles(gpu):
    import torch

    x = impulse_input()
    for name, b in banks(gpu).items():
        got = b.process(N, x, layout=LAYOUT_PLANAR, frame_stride=N, mode=MODE_PROCESS)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for v in range(3):
            assert_bit_equal(got[v], responses()[name][v], f"{name} instance {v}: impulse response")
        assert np.abs(got).max() > 0.01


def test_terms_and_total_within_the_yardstick(gpu):
    ref = host_scores()
    all_refs = [s for name in ref for s in (ref[name] if name == "reverb4_delays" else ref[name][:1])]
    for (f64, t64), _ in all_refs:
        assert np.all(np.abs(t64) > 0) and abs(f64) > 0
    d_terms = np.maximum(FLOOR, np.max([rel(t32, t64) for (_, t64), (_, t32) in all_refs], axis=0))
    d_total = max(FLOOR, max(float(rel(f32, f64)) for (f64, _), (f32, _) in all_refs))
    print(f"yardstick: delta terms {d_terms} total {d_total:.3e}")
    worst_terms, worst_total = np.zeros(4), 0.0
    for name, b in banks(gpu).items():
        fit, terms = scores(b)
        for v in range(3):
            (f64, t64), (f32, t32) = ref[name][v]
            dt, df = rel(terms[v], t64), float(rel(fit[v], f64))
            print(f"{name}[{v}]: f64 fitness {f64:.6f} terms {t64} | f32 serial {f32:.6f} | device {fit[v]:.6f} terms {terms[v]} | device rel dev terms {dt} total {df:.3e}")
            worst_terms, worst_total = np.maximum(worst_terms, dt), max(worst_total, df)
    print(f"device: worst rel dev terms {worst_terms} total {worst_total:.3e}")
    assert np.all(worst_terms <= 4.0 * d_terms), (worst_terms, d_terms)
    assert worst_total <= 4.0 * d_total, (worst_total, d_total)


def test_a_two_channel_convolver_bank(gpu):
    """A convolver's impulse response is its taps (through the partitioned FFT, so to f32 rounding): the twin bank fed the impulse shows the
    samples the call scores, and the host restatements score those -- the same yardstick as above, measured on this response."""
    import torch

    rng = np.random.default_rng(31)
    h = (rng.standard_normal((2, 20000)) * np.exp(-np.arange(20000) / 4000.0) * 0.05).astype(np.float32)
    h[:, :1500] = 0.0
    twin, b = gpu.Bank.convolve(3, h), gpu.Bank.convolve(3, h)
    r = twin.process(N, impulse_input(), layout=LAYOUT_PLANAR, frame_stride=N, mode=MODE_PROCESS)
    torch.cuda.synchronize()
    r = r.cpu().numpy()
    assert np.abs(r[0][:, :20000] - h).max() <= 1e-5 and np.array_equal(r[0], r[2])
    (f64, t64), (f32, t32) = fitness_f64(r[0]), fitness_f32_serial(r[0])
    assert np.all(t64 > 0)
    d_terms, d_total = np.maximum(FLOOR, rel(t32, t64)), max(FLOOR, float(rel(f32, f64)))
    fit, terms = scores(b)
    for v in range(3):
        dt, df = rel(terms[v], t64), float(rel(fit[v], f64))
        print(f"convolve[{v}]: f64 {f64:.6f} device {fit[v]:.6f}; rel dev terms {dt} (delta {d_terms}) total {df:.3e} (delta {d_total:.3e})")
        assert np.all(dt <= 4.0 * d_terms) and df <= 4.0 * d_total
    again = b.process(N, impulse_input(), layout=LAYOUT_PLANAR, frame_stride=N, mode=MODE_PROCESS)
    torch.cuda.synchronize()
    assert_bit_equal(again.cpu().numpy(), r, "the convolver renders after the call like a fresh one")


def test_the_echo_term_counts_the_oracles_samples(gpu):
    """The response bits are exact, so the set of samples with |r| >= 1e-9 is the oracle's: the echo term is the sum of 1 / i over exactly that
    set.  A lane adds at most 32 terms and the tree 10 levels, every 1 / i is one rounding: at most 43 roundings of positive sums, 43 * 2^-24
    relative -- and one sample more or fewer among the first 500 would show (1 / 500 of an echo term of at most 11 is 1.8e-4)."""
    fit, terms = scores(banks(gpu)["reverb4_delays"])
    for v in range(3):
        r = responses()["reverb4_delays"][v]
        for c in range(2):
            idx = echo_weights(r[c])
            assert 0 < len(idx) < N - 1
            want = float(np.sum(1.0 / idx.astype(np.float64)))
            assert want < 11.0 and abs(float(terms[v, 2 * c]) - want) <= 43 * 2.0 ** -24 * want, (v, c, len(idx), terms[v, 2 * c], want)


def test_calls_repeat_and_leave_the_bank_as_constructed(gpu):
    import torch

    rng = np.random.default_rng(3)
    n = 64 * 60 + 7
    x = torch.from_numpy((rng.random((3, 2, n), dtype=np.float32) * 2 - 1).astype(np.float32)).cuda()
    for name, b in banks(gpu).items():
        b.process(640, x[:, :, :640].contiguous(), layout=LAYOUT_PLANAR, frame_stride=640)    # (the call starts from a reset, whatever came before)
        f1, t1 = scores(b)
        f2, t2 = scores(b)
        assert np.array_equal(f1.view(np.uint32), f2.view(np.uint32)) and np.array_equal(t1.view(np.uint32), t2.view(np.uint32)), name
        fresh = banks(gpu)[name]
        got = b.process(n, x, layout=LAYOUT_PLANAR, frame_stride=n)
        want = fresh.process(n, x, layout=LAYOUT_PLANAR, frame_stride=n)
        torch.cuda.synchronize()
        assert_bit_equal(got.cpu().numpy(), want.cpu().numpy(), f"{name}: the render after a fitness call vs a fresh bank's")


def test_the_score_does_not_depend_on_the_bank_size(gpu):
    f3, t3 = scores(banks(gpu)["reverb4_delays"])
    f67, t67 = scores(banks(gpu, 67)["reverb4_delays"])
    for v in range(67):
        assert f67[v].view(np.uint32) == f3[v % 3].view(np.uint32) and np.array_equal(t67[v].view(np.uint32), t3[v % 3].view(np.uint32)), v


def test_refusals(gpu):
    import torch
    from fundsp_amd import workloads as W

    voice = W.make_fm_svf_bank(64, 48000.0, params=W.fm_svf_params(64, 48000.0))
    mono = gpu.Bank.fdn(3, 8, delays_of(8), 2, W2, 1, 1)
    for b in (voice, mono):
        with pytest.raises(gpu.FdspError) as e:
            b.reverb_fitness()
        assert e.value.code == _lib.ENOTSUP
        with pytest.raises(gpu.FdspError) as e:
            b.fitness_reserve()
        assert e.value.code == _lib.ENOTSUP
    b = banks(gpu)["reverb4_delays"]
    b.fitness_reserve()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with pytest.raises(gpu.FdspError) as e:
            with torch.cuda.graph(g, stream=s):
                b.reverb_fitness()
    assert e.value.code == _lib.EINVAL and "capture" in str(e.value)
    torch.cuda.synchronize()
    fit, _ = scores(b)                                       # the refused bank scores afterwards
    want, _ = scores(banks(gpu)["reverb4_delays"])
    assert np.array_equal(fit.view(np.uint32), want.view(np.uint32))


def test_a_reserved_bank_allocates_nothing_in_the_call(gpu):
    """the option "fitness_allocs" counts every device allocation made for the fitness calls (the scratch and the tables): a buffer freed and
    allocated again inside a call would count"""
    b = banks(gpu)["reverb4_delays"]
    assert b.get_option("fitness_scratch_kib") == 0 and b.get_option("fitness_allocs") == 0
    b.fitness_reserve()
    kib = b.get_option("fitness_scratch_kib")
    assert kib == 2 * 3 * 2 * N * 4 // 1024                  # 2 x instances x 2 x 32768 x 4 bytes
    assert b.get_option("fitness_allocs") == 2               # the scratch and the tables
    scores(b)
    scores(b)
    b.fitness_reserve()
    assert b.get_option("fitness_scratch_kib") == kib and b.get_option("fitness_allocs") == 2
    assert b.get_option("fitness_score_us") > 0              # the device time of the last call's scoring kernels
    c = b.clone()
    assert c.get_option("fitness_scratch_kib") == 0 and c.get_option("fitness_allocs") == 0   # not cloned
    lazy = banks(gpu)["reverb_stereo"]
    scores(lazy)                                             # the first uncaptured call reserves
    assert lazy.get_option("fitness_scratch_kib") == kib and lazy.get_option("fitness_allocs") == 2
