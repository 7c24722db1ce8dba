"""GPU parity of the resynthesizer banks' closure path (fdsp_resynth_fn_create, Bank.resynth_fn, resynth_fn(..) in Bank.from_graph): the
stock processors as functors against the STOCK banks (two device formulations with different kernels), and the closures of
tests/resynth_fn_cases.py bit-exact against the numpy restatement tests/resynth_fn_ref.py -- ragged launches and launches longer than a
chunk, both layouts and executors, 1 / 3 / 2048 instances with per-instance parameters, set_params, reset, clone, set_sample_rate, a captured
first launch, subnormal inputs through both builds, noise() >> resynth_fn(..), the refusals, and a foreign-bin write that is dropped."""
import functools

import numpy as np
import pytest

import oracle as O
import resynth_fn_cases as K
import resynth_fn_ref as RF
import resynth_ref as R
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from fundsp_amd import graph as GR
from test_gpu_parity import assert_bit_equal, oracle_render, run_bank

pytestmark = pytest.mark.gpu
f32 = np.float32


@functools.lru_cache(maxsize=None)
def tabs(N):
    return R.tables(N, O.lib().o_math_cosf)


def signal(V, I, T, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (V, I, T)).astype(f32)


def make(case, V, N, params=None, **kw):
    import fundsp_amd as F

    return F.Bank.resynth_fn(V, **case.spec(N), param_values=params, **kw)


def want_of(case, x, N, params=None, **kw):
    return RF.render(x, N, case.closure, case.outputs, params=params, state=case.state, tabs=tabs(N), **kw)


def bits_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{what}: {len(bad)} samples differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


def run_split(bank, x, lens, layout=LAYOUT_VOICE_MINOR, mode=MODE_PROCESS):
    parts, t0 = [], 0
    for n in lens:
        parts.append(run_bank(bank, np.ascontiguousarray(x[:, :, t0:t0 + n]), n, layout, mode))
        t0 += n
    return np.concatenate(parts, axis=2)


IO = [(1, 1), (2, 2), (1, 2), (2, 1)]
SOURCES = {(1, 1): [0], (2, 2): [1, 0], (1, 2): [0, 0], (2, 1): [1]}


@pytest.mark.parametrize("N", [4, 32, 256, 1024, 4096, 8192])
@pytest.mark.parametrize("io", IO)
@pytest.mark.parametrize("proc", ["pass", "band", "gain"])
def test_stock_functors_equal_the_stock_banks(gpu, N, io, proc):
    import fundsp_amd as F

    I, O_ = io
    V, T, NB = 3, 3 * N + 7, N // 2 + 1
    x = signal(V, I, T, seed=N + 10 * I + O_)
    rng = np.random.default_rng(N + 100)
    kw = {}
    if proc == "band":
        lo = rng.uniform(0.0, 8000.0, (V, O_)).astype(f32)
        kw = dict(band=np.stack([lo, lo + f32(6000.0)], axis=-1).astype(f32))
    if proc == "gain":
        kw = dict(gain=rng.uniform(-1.5, 1.5, (V, O_, NB)).astype(f32))
    stock = F.Bank.resynth(V, N, I, O_, processor=proc, source=SOURCES[io], **kw)
    case = K.stock(proc, N, I, O_, SOURCES[io])
    fn = make(case, V, N, K.stock_params(proc, V, O_, NB, **kw))
    want = run_bank(stock, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    got = run_bank(fn, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    assert np.any(want != 0)
    bits_equal(got, want, f"N={N} {I}->{O_} {proc}: functor bank against the stock bank")


@pytest.mark.parametrize("name", list(K.CLOSURES))
def test_closures_ragged_launches_layouts_executors(gpu, name):
    case = K.CLOSURES[name]
    N, V = 32, 3
    H = N // 4
    lens = [1, 63, 64, H - 1, H + 1, N + 5, 3 * N + 7]
    T = sum(lens)
    x = signal(V, case.inputs, T, seed=9)
    p = K.case_params(name, V, N)
    want = want_of(case, x, N, p)
    assert np.any(want != 0)
    bits_equal(run_bank(make(case, V, N, p), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), want, f"{name}: one launch")
    for layout in (LAYOUT_VOICE_MINOR, LAYOUT_PLANAR):
        for mode in (MODE_PROCESS, MODE_TICK):
            bits_equal(run_split(make(case, V, N, p), x, lens, layout, mode), want, f"{name}: ragged launches, layout {layout}, mode {mode}")
    # one instance
    bits_equal(run_bank(make(case, 1, N, None if p is None else p[:1]), x[:1], T, LAYOUT_PLANAR, MODE_PROCESS), want[:1], f"{name}: one instance")


@pytest.mark.parametrize("name", list(K.CLOSURES))
def test_closures_launch_longer_than_a_chunk(gpu, name):
    """3 instances of N = 32 take chunks of 30 848 samples: 31 500 samples in one launch are two chunks, and equal 5 ragged launches"""
    case = K.CLOSURES[name]
    N, V, T = 32, 3, 31500
    x = signal(V, case.inputs, T, seed=21)
    p = K.case_params(name, V, N, seed=1)
    want = want_of(case, x, N, p)
    bits_equal(run_bank(make(case, V, N, p), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), want, f"{name}: one long launch")
    bits_equal(run_split(make(case, V, N, p), x, [7, 20000, 1, 11000, 492], LAYOUT_PLANAR), want, f"{name}: long ragged launches")


@pytest.mark.parametrize("name", list(K.CLOSURES))
def test_closures_many_instances_per_instance_parameters(gpu, name):
    """2048 instances of N = 256 take chunks of 3968 samples: 5000 samples are two chunks"""
    case = K.CLOSURES[name]
    N, V, T = 256, 2048, 5000
    x = signal(V, case.inputs, T, seed=5)
    p = K.case_params(name, V, N, seed=2)
    got = run_bank(make(case, V, N, p), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    sel = [0, 1, 777, 2046, 2047]
    want = want_of(case, x[sel], N, None if p is None else p[sel])
    for n, v in enumerate(sel):
        assert_bit_equal(got[v], want[n], f"{name}: instance {v}")


def test_set_params_reset_and_clone(gpu):
    N, V, T1, T2 = 64, 3, 300, 400
    x = signal(V, 1, T1 + T2, seed=11)
    x1, x2 = np.ascontiguousarray(x[:, :, :T1]), np.ascontiguousarray(x[:, :, T1:])
    # set_params between launches: the frames above the launch's start take the new values
    p1, p2 = K.case_params("gate", V, N, seed=3), K.case_params("gate", V, N, seed=4)
    b = make(K.GATE, V, N, p1)
    a = run_bank(b, x1, T1, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    b.set_resynth_params(p2)
    got = run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    want = want_of(K.GATE, x, N, p1, changes=[(T1, dict(params=p2))])
    bits_equal(np.concatenate([a, got], axis=2), want, "set_params between launches")
    b.set_resynth_params(p1[1], first=1)   # one row
    b.set_resynth_params(p1[:1])
    b.set_resynth_params(p1[2:], first=2)
    b.reset()
    bits_equal(run_bank(b, x1, T1, LAYOUT_VOICE_MINOR, MODE_PROCESS), want[:, :, :T1], "reset, rows set one by one")
    # the smoother: reset clears the state with the windows; a clone in mid-stream continues bit-equal to its source
    ps = K.case_params("smooth", V, N)
    want = want_of(K.SMOOTH, x, N, ps)
    b = make(K.SMOOTH, V, N, ps)
    run_bank(b, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    b.reset()
    bits_equal(run_bank(b, x1, T1, LAYOUT_VOICE_MINOR, MODE_PROCESS), want[:, :, :T1], "smoother after reset")
    c = b.clone()
    for bank, what in ((b, "source"), (c, "clone")):
        bits_equal(run_bank(bank, x2, T2, LAYOUT_VOICE_MINOR, MODE_PROCESS), want[:, :, T1:], f"smoother, {what} in mid-stream")


def test_time_switch_follows_set_sample_rate(gpu):
    """fft.time() in f64: the switch happens at param(0) seconds, and earlier in samples after set_sample_rate(22050) in mid-stream"""
    N, V, T1, T2 = 32, 3, 200, 600
    x = signal(V, 1, T1 + T2, seed=31)
    p = np.array([[0.004], [0.009], [0.02]], f32)
    b = make(K.SWITCH, V, N, p)
    a = run_bank(b, np.ascontiguousarray(x[:, :, :T1]), T1, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    b.set_sample_rate(22050.0)
    got = run_bank(b, np.ascontiguousarray(x[:, :, T1:]), T2, LAYOUT_VOICE_MINOR, MODE_PROCESS)
    want = want_of(K.SWITCH, x, N, p, changes=[(T1, dict(sample_rate=22050.0))])
    assert not np.array_equal(want, want_of(K.SWITCH, x, N, p)), "the change of rate moves the switch"
    bits_equal(np.concatenate([a, got], axis=2), want, "time switch across set_sample_rate")


def test_captured_first_launch_replays_against_an_uncaptured_twin(gpu):
    """The module is compiled and loaded at creation: the bank's very first launch is captured; the replays move on like the twin's launches"""
    import torch

    N, V, T, reps = 32, 5, 40, 4
    x = signal(V, 1, T * reps, seed=13)
    p = K.case_params("smooth", V, N)
    b, twin = make(K.SMOOTH, V, N, p), make(K.SMOOTH, V, N, p)
    inp = torch.zeros((1, T, V), dtype=torch.float32, device="cuda")
    out = torch.zeros((1, T, V), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.process(T, inp, out)
    parts = []
    for r in range(reps):
        inp.copy_(torch.from_numpy(np.ascontiguousarray(x[:, :, T * r:T * (r + 1)].transpose(1, 2, 0))))
        g.replay()
        torch.cuda.synchronize()
        parts.append(out.cpu().numpy().transpose(2, 0, 1).copy())
    got = np.concatenate(parts, axis=2)
    bits_equal(got, run_split(twin, x, [T] * reps), "captured first launch, replayed, against the twin")
    bits_equal(got, want_of(K.SMOOTH, x, N, p), "captured first launch, replayed, against the restatement")


def test_subnormal_inputs_through_both_builds(gpu):
    N, V, T = 32, 2, 200
    for name in ("cross", "smooth", "gate"):
        case = K.CLOSURES[name]
        x = signal(V, case.inputs, T, seed=17)
        x[0] *= f32(2.0 ** -130)
        x[1, 0] *= f32(2.0 ** -100)   # (cross: products of the two inputs' bins fall into the denormal range)
        x[1, 1:] *= f32(2.0 ** -25)
        p = None if case.params == 0 else np.full((V, 1), 0.5 if name == "smooth" else 0.0, f32)
        outs = []
        for ftz in (False, True):
            got = run_bank(make(case, V, N, p, flush_denormals=ftz), x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)
            bits_equal(got, want_of(case, x, N, p, ftz=ftz), f"{name}, ftz={ftz}")
            outs.append(got)
        assert not np.array_equal(outs[0], outs[1]), f"{name}: the flushed build differs on subnormal data"


def test_chain_noise_into_resynth_fn(gpu):
    """noise() >> resynth_fn(1024, gate) through Bank.from_graph: the front's own render fed to the restatement"""
    import torch

    import fundsp_amd as F
    from fundsp_amd.bank import PIPE_ID, atto, probe_hash

    T, N = 6000, 1024
    g = GR.noise() >> GR.resynth_fn(**K.GATE.spec(N), threshold=np.array([20.0, 60.0], f32))
    ch = F.Bank.from_graph(g, 2)
    assert isinstance(ch, F.Chain) and ch.effect.kind == "resynth"
    out = ch.process(T)
    torch.cuda.synchronize()
    got = out.cpu().numpy().transpose(2, 0, 1)
    n = O.noise()
    n.set_seed(int(atto(np.uint64(probe_hash(g)), PIPE_ID)))
    x = oracle_render(n, None, T, MODE_PROCESS)
    want = want_of(K.GATE, np.stack([x, x]), N, np.array([[20.0], [60.0]], f32))
    assert not np.array_equal(want[0], want[1])
    bits_equal(got, want, "noise() >> resynth_fn(gate)")
    # the node alone, moved to another rate
    b = F.Bank.from_graph(GR.resynth_fn(**K.stock("band", 64, 1, 1, [0]).spec(64), lo=1000.0, hi=5000.0), 3, sample_rate=22050.0)
    xs = signal(3, 1, 500, seed=2)
    bits_equal(run_bank(b, xs, 500, LAYOUT_VOICE_MINOR, MODE_PROCESS), R.render(xs, 64, processor="band", band=(1000.0, 5000.0), sample_rate=22050.0, tabs=tabs(64)),
               "resynth_fn(band) alone at 22.05 kHz")


def test_refusals_and_the_dropped_foreign_write(gpu):
    import ctypes as C

    import fundsp_amd as F
    from fundsp_amd import _lib

    L = _lib.lib()
    N, V, T = 32, 3, 200
    x = signal(V, 1, T, seed=7)
    b = make(K.FOREIGN, V, N)
    bits_equal(run_bank(b, x, T, LAYOUT_VOICE_MINOR, MODE_PROCESS), R.render(x, N, tabs=tabs(N)), "writes to a foreign bin or channel are dropped: a pass-through")
    bits_equal(run_bank(make(K.FOREIGN, V, N), x, T, LAYOUT_PLANAR, MODE_TICK), want_of(K.FOREIGN, x, N), "... and equal to the restatement")
    one = np.ones((V, 2 * (N // 2 + 1)), f32)
    assert L.fdsp_resynth_set_band(b._h, _lib._fp(), 0, 0) == _lib.EINVAL      # NULL values
    assert L.fdsp_resynth_set_band(b._h, one.ctypes.data_as(_lib._fp), 0, 1) == _lib.ENOTSUP
    assert L.fdsp_resynth_set_gain(b._h, one.ctypes.data_as(_lib._fp), 0, 1) == _lib.ENOTSUP
    stock = F.Bank.resynth(V, N)
    assert L.fdsp_resynth_set_params(stock._h, one.ctypes.data_as(_lib._fp), 0, 1) == _lib.ENOTSUP
    gate = make(K.GATE, V, N, np.zeros((V, 1), f32))
    assert L.fdsp_resynth_set_params(gate._h, one.ctypes.data_as(_lib._fp), 2, 2) == _lib.EINVAL   # beyond the instances
    assert L.fdsp_resynth_set_params(gate._h, one.ctypes.data_as(_lib._fp), 3, 0) == _lib.OK
    with pytest.raises(ValueError):
        gate.set_resynth_params(np.ones((1, 2), f32))
    assert L.fdsp_bank_set_bus(b._h, _lib.BUS_WET, 0.5, 1.0) == _lib.ENOTSUP
    out = C.c_void_p()
    assert L.fdsp_bank_process_mix(b._h, 64, None, out, _lib.MIX_SUM, 0, None) == _lib.ENOTSUP
    with pytest.raises(F.FdspError) as e:
        make(K.Case("Nope", "struct Nope { int", None), V, N)
    assert e.value.code == _lib.EINVAL and "error:" in str(e.value)
