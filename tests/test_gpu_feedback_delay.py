"""GPU parity of the feedback delay banks (fdsp_feedback_delay_create, Bank.feedback_delay, Bank.feedback_tree):

    line form:  feedback( L [>> reverse()] [* g] )          loop form:  feedback2( L [>> reverse()], Y )
      L = line | line_0 | line_1,  line_i = delay(t_i) [>> fir(w_i..)] [>> F_i] [* g_i],  Y = F [* g] | (F_0 [* g_0]) | (F_1 [* g_1])

bit for bit against the oracle's generic Feedback / Feedback2 tree built per instance with that instance's parameters: the grammar matrix, the
ring and launch edges, both layouts, per-instance parameters, the denormal range, reset / clone / a change of rate, the refusals, the bus,
the fused mix-down, a chain behind a generator, and the run-time compiled rendering of the same graphs.  Delays are 128 .. 300 samples, so
several trips round the loop fit into the 1 200 frames a case renders at most."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
from fundsp_amd import BUS_DRY_WET, LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MIX_PAN, MIX_SUM, MODE_PROCESS, MODE_TICK, _lib
from fundsp_amd import graph as GR
from test_feedback_delay_plan import cpp_case
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
SR = 48000.0
SECONDS = lambda k: (np.asarray(k, dtype=np.float64) / SR).astype(np.float32).astype(np.float64)   # whole samples at SR as the f32 seconds delay(t) takes


def params(N, place, filt, taps, line_gain, outer, reverse, V=None, delay_samples=None, seed=0):
    """Bank.feedback_delay keyword arguments: one value per channel, and with V a [V, N] spread of delays / cutoffs / gains"""
    rng = np.random.default_rng(1000 + seed)
    k = np.asarray(delay_samples if delay_samples is not None else ([150, 233][:N]), dtype=np.float64)
    p = dict(place=place, reverse=bool(reverse))
    if V is not None and k.ndim == 1:
        k = k[None, :] + 7.0 * np.arange(V, dtype=np.float64)[:, None]       # 150 .. 150 + 7 (V - 1)
    p["delays"] = SECONDS(k)
    spread = (lambda a, lo, hi: (a[None, :] * np.linspace(lo, hi, V, dtype=np.float32)[:, None]).astype(np.float32)) if V is not None else (lambda a, lo, hi: a)
    if taps:
        w = ((rng.random((N, taps), dtype=np.float32) * 0.5 + 0.3) / np.float32(taps)).astype(np.float32)
        p["weights"] = (w[None] * np.linspace(1.0, 0.8, V, dtype=np.float32)[:, None, None]).astype(np.float32) if V is not None else w
    if filt is not None:
        p["filter"] = filt
        p["cutoff"] = spread(np.array([2500.0, 4100.0][:N], dtype=np.float32), 1.0, 2.0)
        if filt != "lowpole":
            p["q"] = spread(np.array([0.8, 1.1][:N], dtype=np.float32), 1.0, 1.3)
            p["gain"] = spread(np.array([0.5, 0.7][:N], dtype=np.float32), 1.0, 1.2)    # (a bell that cuts: the loop stays stable)
    if line_gain:
        p["line_gain"] = spread(np.array([0.9, 0.8][:N], dtype=np.float32), 1.0, 0.9)
    if outer:
        p["outer_gain"] = np.linspace(0.95, 0.85, V, dtype=np.float32) if V is not None else 0.9
    return p


def build(m, p, v=None):
    """the Feedback / Feedback2 tree of instance v in the oracle's notation (m = oracle), or the whole bank's graph with per-voice arrays
    (m = fundsp_amd.graph, v = None)"""
    N = np.asarray(p["delays"]).shape[-1]
    filt = p.get("filter")

    def val(name, i):
        a = np.asarray(p[name])
        if a.ndim == 2:
            return float(a[v, i]) if v is not None else np.ascontiguousarray(a[:, i].astype(np.float32))
        return float(a[i])

    def weights(i):
        w = np.asarray(p["weights"])
        if w.ndim == 3:
            return [float(x) for x in w[v, i]] if v is not None else [np.ascontiguousarray(w[:, i, j]) for j in range(w.shape[-1])]
        return [float(x) for x in w[i]]

    def F(i):
        c = val("cutoff", i)
        f = m.lowpole_hz(c) if filt == "lowpole" else m._fsvf(filt, c, val("q", i), val("gain", i))
        return f * val("line_gain", i) if "line_gain" in p else f

    def line(i):
        x = m.delay(val("delays", i))
        if "weights" in p:
            x = x >> m.fir(*weights(i))
        if p["place"] == "line":
            if filt is not None:
                x = x >> F(i)
            elif "line_gain" in p:
                x = x * val("line_gain", i)
        return x

    L = line(0) if N == 1 else (line(0) | line(1))
    if p.get("reverse"):
        L = L >> m.reverse(2)
    if p.get("outer_gain") is not None:
        og = np.asarray(p["outer_gain"], dtype=np.float32)
        L = L * (float(og) if og.ndim == 0 else float(og[v]) if v is not None else og)
    if p["place"] == "line":
        return m.feedback(L)
    return m.feedback2(L, F(0) if N == 1 else (F(0) | F(1)))


def oracle_net(p, v, sr=SR):
    n = build(O, p, v)
    n.set_sample_rate(sr)
    return n


def oracle_render(net, x, cuts, mode=MODE_PROCESS):
    return np.concatenate([net.render_blocks(x[:, a:e]) if mode == MODE_PROCESS else net.render_ticks(x[:, a:e]) for a, e in zip(cuts[:-1], cuts[1:])], axis=1)


def signal(V, N, T, seed, stop=None):
    """noise that stops at `stop` (2T/3); instance 1 (where there is one) lives in the denormal range"""
    rng = np.random.default_rng(seed)
    x = (rng.random((V, N, T), dtype=np.float32) * 2 - 1).astype(np.float32)
    stop = 2 * T // 3 if stop is None else stop
    x[:, :, stop:] = 0.0
    if V > 1:
        x[1] *= np.float32(1e-30)
        x[1, :, max(0, stop - 40):stop] = np.float32(3e-39)
    return x


def run(bank, x, layout, mode, cuts, pad=0):
    """x: [V][N][T] -> [V][N][T], launch by launch; planar rows `pad` floats longer than the launch"""
    import torch

    parts = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        n = e - a
        if layout == LAYOUT_PLANAR:
            xi = np.zeros(x.shape[:2] + (n + pad,), dtype=np.float32)
            xi[:, :, :n] = x[:, :, a:e]
            y = bank.process(n, torch.from_numpy(xi).cuda(), layout=layout, frame_stride=n + pad, mode=mode)
            torch.cuda.synchronize()
            parts.append(y.cpu().numpy()[:, :, :n])
        else:
            xi = torch.from_numpy(np.ascontiguousarray(x[:, :, a:e].transpose(1, 2, 0))).cuda()
            y = bank.process(n, xi, layout=layout, mode=mode)
            torch.cuda.synchronize()
            parts.append(y.cpu().numpy().transpose(2, 0, 1))
    return np.concatenate(parts, axis=2)


def make(gpu, p, V, sr=SR):
    b = gpu.Bank.feedback_delay(V, **p, sample_rate=sr)
    N = np.asarray(p["delays"]).shape[-1]
    assert b.kind == "feedback_delay" and b.inputs() == N and b.outputs() == N
    return b


# ---- the grammar matrix -----------------------------------------------------------------------------------------------------------------
# (place, filter, taps, line gain, outer gain): every value of every axis, with each of the three channel shapes below; the loop form needs
# its filter and has no outer gain (the grammar)
ROWS = [
    ("line", None, 0, False, False),
    ("line", None, 0, True, False),        # the echo, feedback(delay(t) * g)
    ("line", None, 3, False, True),        # the ping-pong's shape with a FIR
    ("line", None, 1, True, True),
    ("line", "lowpole", 0, True, False),
    ("line", "lowpole", 3, False, True),
    ("line", "lowpass", 1, True, True),
    ("line", "bell", 3, True, False),
    ("line", "bell", 1, False, True),
    ("loop", "lowpole", 0, True, False),
    ("loop", "lowpass", 1, True, False),
    ("loop", "bell", 0, False, False),
    ("loop", "bell", 3, True, False),
]
SHAPES = [(1, False), (2, False), (2, True)]   # channels, reverse()
MATRIX = [(N, rev) + r for N, rev in SHAPES for r in ROWS]


def test_the_matrix_covers_every_value_with_every_shape():
    for N, rev in SHAPES:
        rows = [r[2:] for r in MATRIX if r[:2] == (N, rev)]
        assert {r[0] for r in rows} == {"line", "loop"} and {r[1] for r in rows} == {None, "lowpole", "lowpass", "bell"}
        assert {r[2] for r in rows} == {0, 1, 3} and {r[3] for r in rows} == {False, True} and {r[4] for r in rows} == {False, True}
    assert len(MATRIX) == 39


@pytest.mark.parametrize("N,rev,place,filt,taps,lg,og", MATRIX, ids=["-".join(str(v) for v in r) for r in MATRIX])
def test_grammar_matrix_matches_oracle(gpu, N, rev, place, filt, taps, lg, og):
    V, T = 5, 64 * 9 + 37
    p = params(N, place, filt, taps, lg, og, rev, seed=taps + 4 * N)
    b = make(gpu, p, V)
    x = signal(V, N, T, 17 + N + taps)
    cuts = [0, 64, 101, 102, T]
    got = run(b, x, LAYOUT_PLANAR, MODE_PROCESS, cuts)
    assert b.get_option("last_kernel") == 6
    for v in (0, 1, V - 1):
        assert_bit_equal(got[v], oracle_render(oracle_net(p, v), x[v], cuts), f"{p['place']} N={N} rev={rev} {filt} fir{taps} lg={lg} og={og} instance {v}")
    assert np.abs(got[0, :, 2 * T // 3 + 130:]).max() > 1e-6                            # the tail recirculates
    assert not np.any((got[1] != 0) & (np.abs(got[1]) < np.float32(1.17549435e-38)))    # no denormal reaches the output


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
# delays of exactly 128 samples (the shortest) and 255 (len == cap == 256: the ring exactly full); 700 frames wrap the 256-slot rings twice, and
# after the launches of 64 + 37 + 1 + 300 the write position is 146: the second block of the last launch straddles the wrap
EDGE = dict(N=2, place="loop", filt="lowpole", taps=3, line_gain=True, outer=False, reverse=True, delay_samples=[128, 255])
EDGE_T = 700
EDGE_CUTS = [0, 64, 101, 102, 402, EDGE_T]


@functools.lru_cache(maxsize=None)
def edge_reference(V):
    """(parameters, input, the oracle's render of instances 0, 1, V // 2, V - 1): computed once per V, shared by the layouts"""
    p = params(V=None, **EDGE)
    x = signal(V, 2, EDGE_T, 300 + V, stop=500)
    want = {v: oracle_render(oracle_net(p, v), x[v], EDGE_CUTS) for v in sorted({0, min(1, V - 1), V // 2, V - 1})}
    for a in (x, *want.values()):
        a.setflags(write=False)
    return p, x, want


@pytest.mark.parametrize("layout,pad", [(LAYOUT_PLANAR, 0), (LAYOUT_PLANAR, 3), (LAYOUT_VOICE_MINOR, 0)], ids=["planar", "planar_odd_stride", "voice_minor"])
@pytest.mark.parametrize("V", [1, 5, 67])
def test_ring_edges_bank_sizes_and_layouts(gpu, V, layout, pad):
    """V = 1 and 5: a partial workgroup; 67: the staged voice-minor path (V >= 64) and a ragged last workgroup"""
    p, x, want = edge_reference(V)
    assert int(np.round(p["delays"] * SR).min()) == 128 and int(np.round(p["delays"] * SR).max()) + 1 == 256
    b = make(gpu, p, V)
    got = run(b, x, layout, MODE_PROCESS, EDGE_CUTS, pad)
    for v, w in want.items():
        assert_bit_equal(got[v], w, f"V={V} layout={layout} pad={pad} instance {v}")
    assert np.abs(got[0, :, 520:]).max() > 1e-6


@pytest.mark.parametrize("T", [1, 63, 64, 65, 200])
def test_launch_lengths_in_mid_tail(gpu, T):
    """a launch of T frames behind 300 frames of noise (a fresh network answers its first 128 frames with zeros, which would prove nothing)"""
    V = 5
    p = params(V=None, **EDGE)
    x = signal(V, 2, 300 + T, 40 + T, stop=300 + T)
    b = make(gpu, p, V)
    got = run(b, x, LAYOUT_PLANAR, MODE_PROCESS, [0, 300, 300 + T])
    for v in (0, V - 1):
        assert_bit_equal(got[v], oracle_render(oracle_net(p, v), x[v], [0, 300, 300 + T]), f"T={T} instance {v}")
    assert np.abs(got[0, :, 300:]).max() > 1e-3


def test_split_launches_and_tick_mode_change_no_bit(gpu):
    V, T = 5, 402
    p = params(V=None, **EDGE)
    x = signal(V, 2, T, 77, stop=350)
    whole = run(make(gpu, p, V), x, LAYOUT_PLANAR, MODE_PROCESS, [0, T])
    assert np.abs(whole[0]).max() > 1e-3
    assert_bit_equal(run(make(gpu, p, V), x, LAYOUT_PLANAR, MODE_PROCESS, [0, 64, 101, 102, T]), whole, "64 + 37 + 1 + 300 vs one launch of 402")
    assert_bit_equal(run(make(gpu, p, V), x, LAYOUT_PLANAR, MODE_TICK, [0, T]), whole, "FDSP_MODE_TICK vs FDSP_MODE_PROCESS")
    assert_bit_equal(run(make(gpu, p, V), x, LAYOUT_VOICE_MINOR, MODE_TICK, [0, 64, 101, 102, T]), whole, "tick, voice-minor, split")
    assert_bit_equal(whole[0], oracle_net(p, 0).render_ticks(x[0]), "the oracle's tick executor")


# ---- per-instance parameters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,place,filt,taps,lg,og,rev", [(2, "line", "bell", 3, True, True, True), (1, "loop", "lowpole", 2, True, False, False),
                                                           (1, "line", None, 0, True, True, False)])
def test_each_instance_equals_a_bank_of_its_own_row(gpu, N, place, filt, taps, lg, og, rev):
    V, T = 5, 64 * 8 + 11
    p = params(N, place, filt, taps, lg, og, rev, V=V, seed=3)
    x = signal(V, N, T, 91)
    got = run(make(gpu, p, V), x, LAYOUT_PLANAR, MODE_PROCESS, [0, 100, T])
    for v in range(V):
        row = {k: (a[v] if isinstance(a, np.ndarray) and a.ndim and a.shape[0] == V and k != "filter" else a) for k, a in p.items()}
        if og:
            row["outer_gain"] = float(p["outer_gain"][v])
        one = run(make(gpu, row, 1), x[v:v + 1], LAYOUT_PLANAR, MODE_PROCESS, [0, 100, T])
        assert_bit_equal(got[v], one[0], f"instance {v} vs a one-instance bank of its row")
    for v in (0, V - 1):
        assert_bit_equal(got[v], oracle_render(oracle_net(p, v), x[v], [0, 100, T]), f"instance {v} vs the oracle")
    assert not np.array_equal(got[0], got[V - 1])


# ---- denormals --------------------------------------------------------------------------------------------------------------------------
def test_an_impulse_decays_to_exact_zero_and_a_subnormal_input_is_zero(gpu):
    """1e-37 through `* 0.5` once per trip: 5e-38, 2.5e-38, 1.25e-38, then 6.25e-39 -- below the smallest normal f32, flushed: Feedback::new
    calls prevent_denormals.  Instance 1 is fed subnormals only: xin = in + value flushes them on the way into the delay line."""
    V, T = 3, 128 * 7
    p = dict(place="line", reverse=False, delays=SECONDS([128]), line_gain=np.array([0.5], dtype=np.float32))
    x = np.zeros((V, 1, T), dtype=np.float32)
    x[0, 0, 0] = np.float32(1e-37)
    x[1, 0, :200] = np.float32(3e-39)
    x[2, 0, 0] = 1.0
    got = run(make(gpu, p, V), x, LAYOUT_PLANAR, MODE_PROCESS, [0, 300, T])
    for v in range(V):
        assert_bit_equal(got[v], oracle_render(oracle_net(p, v), x[v], [0, 300, T]), f"instance {v}")
    # a trip round the loop is 129 frames: the delay's 128 and the frame the feedback value waits for its input
    assert got[0, 0, 128] == np.float32(1e-37) * np.float32(0.5) and got[0, 0, 128 + 2 * 129] == np.float32(1e-37) * np.float32(0.125)
    assert not got[0, 0, 128 + 2 * 129 + 1:].any()  # exact zero from the fourth trip on: 6.25e-39 is flushed
    assert not got[1].any()                         # a subnormal input is treated as zero
    assert got[2, 0, 128 + 5 * 129] == np.float32(0.5 ** 6)


# ---- lifecycle --------------------------------------------------------------------------------------------------------------------------
LIFE = dict(N=2, place="loop", filt="lowpass", taps=3, line_gain=True, outer=False, reverse=True)


def life_params():
    p = params(**LIFE)
    p["delays"] = np.array([0.004, 0.006], dtype=np.float32).astype(np.float64)   # 176 / 265 samples at 44.1 kHz, 192 / 288 at 48 kHz
    return p


def test_reset_in_mid_tail(gpu):
    V, T = 5, 900
    p = life_params()
    x = signal(V, 2, T, 5, stop=500)
    b = make(gpu, p, V)
    first = run(b, x, LAYOUT_PLANAR, MODE_PROCESS, [0, 600])
    b.reset()
    again = run(b, x, LAYOUT_PLANAR, MODE_PROCESS, [0, 77, T])
    assert_bit_equal(again[:, :, :600], first, "after reset: the same first launches again")
    for v in (0, V - 1):
        n = oracle_net(p, v)
        n.render_blocks(x[v][:, :600])
        n.reset()
        assert_bit_equal(again[v], oracle_render(n, x[v], [0, 77, T]), f"the oracle after reset, instance {v}")


def test_clone_in_mid_tail(gpu):
    V, T = 5, 900
    p = life_params()
    x = signal(V, 2, T, 6, stop=500)
    b = make(gpu, p, V)
    a1 = run(b, x, LAYOUT_PLANAR, MODE_PROCESS, [0, 600])
    c = b.clone()
    a2 = run(b, x[:, :, 600:], LAYOUT_PLANAR, MODE_PROCESS, [0, 77, T - 600])
    c2 = run(c, x[:, :, 600:], LAYOUT_VOICE_MINOR, MODE_PROCESS, [0, T - 600])
    assert_bit_equal(c2, a2, "the clone continues like the original")
    assert np.abs(a2[0]).max() > 1e-4
    for v in (0, V - 1):
        assert_bit_equal(np.concatenate([a1, a2], axis=2)[v], oracle_render(oracle_net(p, v), x[v], [0, 600, 677, T]), f"instance {v}")


def test_change_of_rate_in_mid_tail(gpu):
    """44 100 -> 48 000 Hz: the rings are resized and emptied, the coefficients follow, the Fir history, the filter states and `value` stay"""
    V, T = 5, 1100
    p = life_params()
    x = signal(V, 2, T, 7, stop=800)
    b = make(gpu, p, V, sr=44100.0)
    a1 = run(b, x[:, :, :500], LAYOUT_PLANAR, MODE_PROCESS, [0, 500])
    b.set_sample_rate(48000.0)
    a2 = run(b, x[:, :, 500:], LAYOUT_PLANAR, MODE_PROCESS, [0, 70, T - 500])
    assert np.abs(a2[:, :, 0]).max() > 0.0   # (the emptied lines read zeros: what sounds at once is the Fir history that stayed)
    nets = {}
    for v in (0, V - 1):
        n = nets[v] = oracle_net(p, v, sr=44100.0)
        w1 = n.render_blocks(x[v][:, :500])
        n.set_sample_rate(48000.0)
        w2 = oracle_render(n, x[v][:, 500:], [0, 70, T - 500])
        assert_bit_equal(a1[v], w1, f"44.1 kHz instance {v}")
        assert_bit_equal(a2[v], w2, f"48 kHz instance {v}")
    # a rate at which a delay falls under two blocks is refused and changes nothing
    with pytest.raises(gpu.FdspError, match="128 samples"):
        b.set_sample_rate(22050.0)
    x3 = signal(V, 2, 200, 8)
    a3 = run(b, x3, LAYOUT_PLANAR, MODE_PROCESS, [0, 200])
    for v in (0, V - 1):
        assert_bit_equal(a3[v], nets[v].render_blocks(x3[v]), f"after the refused change, instance {v}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_einval_and_create_no_bank(gpu):
    L = gpu.lib()

    def raw(delays, channels, sr=SR, **kw):
        d = (C.c_double * len(delays))(*delays)
        net = _lib.FeedbackDelay(channels=channels, delays=d, **kw)
        h = C.c_void_p(1)
        rc = L.fdsp_feedback_delay_create(2, C.byref(net), sr, C.byref(h))
        return rc, h.value, L.fdsp_last_error()

    rc, h, err = raw([127.0 / SR], 1)
    assert rc == _lib.EINVAL and not h and b"at least 128 samples" in err
    rc, h, err = raw([128.0 / SR], 1)
    assert rc == 0 and h
    L.fdsp_bank_destroy(C.c_void_p(h))
    rc, h, err = raw([(2 ** 18) / SR], 1)                  # len = 2^18 + 1
    assert rc == _lib.EINVAL and not h and b"2^18 slots" in err
    rc, h, err = raw([0.005] * 3, 3)
    assert rc == _lib.EINVAL and not h and b"channels" in err
    rc, h, err = raw([0.005], 1, place=_lib.FDN_IN_LOOP)
    assert rc == _lib.EINVAL and not h and b"loop form" in err
    with pytest.raises(gpu.FdspError, match="128 samples") as e:
        gpu.Bank.feedback_delay(2, [0.005, 127.0 / SR], sample_rate=SR)
    assert e.value.code == _lib.EINVAL
    with pytest.raises(gpu.FdspError, match="channels"):
        gpu.Bank.feedback_delay(2, [0.005] * 3, sample_rate=SR)
    with pytest.raises(gpu.FdspError, match="loop form"):
        gpu.Bank.feedback_delay(2, 0.005, place="loop", sample_rate=SR)
    with pytest.raises(ValueError, match="feedback_tree"):
        gpu.Bank.feedback_tree(GR.fdn(GR.stacki(2, lambda i: GR.delay(0.005))), 2)


# ---- bus, mix, chain --------------------------------------------------------------------------------------------------------------------
def test_bus_equals_the_oracles_pass_and_wet_feedback(gpu):
    """`pass() & 0.2 * feedback(..)`, examples/network.rs's shape, folded into the kernel's epilogue (fdsp_bank_set_bus)"""
    V, T = 5, 700
    p = params(1, "line", "lowpole", 2, True, False, False)
    b = make(gpu, p, V)
    b.set_bus(BUS_DRY_WET, 0.2, 1.0)
    x = signal(V, 1, T, 12)
    got = run(b, x, LAYOUT_PLANAR, MODE_PROCESS, [0, 100, T])
    for v in (0, 1, V - 1):
        n = O.pass_() & 0.2 * build(O, p, v)
        n.set_sample_rate(SR)
        assert_bit_equal(got[v], oracle_render(n, x[v], [0, 100, T]), f"bus instance {v}")


def dev(x, layout):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0)) if layout == LAYOUT_VOICE_MINOR else np.ascontiguousarray(x)).cuda()


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("layout", [LAYOUT_VOICE_MINOR, LAYOUT_PLANAR])
def test_fused_mix_sum_equals_process_plus_sum_voices(gpu, layout):
    V, T = 67, 64 * 3 + 9
    p = params(2, "line", None, 0, False, True, True)
    b = make(gpu, p, V)
    warm = signal(V, 2, 400, 3, stop=400)
    b.process(400, dev(warm, LAYOUT_VOICE_MINOR))
    ref = b.clone()
    b.set_option("fx_mix_chunk_frames", 64)
    assert b.get_option("has_fused_mix") == 1
    x = signal(V, 2, T, 4, stop=T)
    mix = host(b.process_mix(T, dev(x, layout), mix=MIX_SUM, layout=layout))
    out = ref.process(T, dev(x, LAYOUT_VOICE_MINOR))
    assert mix.shape == (2, T) and np.abs(mix).max(axis=1).min() > 0
    assert_bit_equal(mix, host(gpu.sum_voices(out)), "MIX_SUM, chunks of 64 frames, vs process + sum_voices")
    x2 = dev(signal(V, 2, 70, 5, stop=70), LAYOUT_VOICE_MINOR)
    assert_bit_equal(host(b.process(70, x2)), host(ref.process(70, x2)), "the next render after a mix launch")


def test_fused_mix_pan_on_the_mono_bank(gpu):
    import torch

    V, T = 67, 64 * 2 + 5
    p = params(1, "line", None, 0, True, False, False)
    b = make(gpu, p, V)
    pan = np.linspace(-1.2, 1.2, V).astype(np.float32)
    b.set_pan(pan)
    b.process(300, dev(signal(V, 1, 300, 13, stop=300), LAYOUT_VOICE_MINOR))
    ref = b.clone()
    x = signal(V, 1, T, 14, stop=T)
    mix = host(b.process_mix(T, dev(x, LAYOUT_VOICE_MINOR), mix=MIX_PAN))
    out = ref.process(T, dev(x, LAYOUT_VOICE_MINOR))
    assert mix.shape == (2, T) and np.abs(mix[0] - mix[1]).max() > 0
    assert_bit_equal(mix, host(gpu.mix_stereo(out[0], torch.from_numpy(pan).cuda())), "MIX_PAN vs process + mix_stereo")
    two = make(gpu, params(2, "line", None, 0, True, False, False), 3)
    with pytest.raises(gpu.FdspError):
        two.process_mix(64, dev(signal(3, 2, 64, 1), LAYOUT_VOICE_MINOR), mix=MIX_PAN)


def test_chain_behind_a_generator_equals_the_oracles_whole_graph(gpu):
    """noise() >> feedback(delay(t) * g), composed by the caller: the front compiled with flushed denormals as the one graph would be, seeded from
    the construction hash of the whole graph and then per voice"""
    from fundsp_amd.bank import probe_hash

    V, T = 5, 800
    t, g = float(SECONDS(171)), 0.7
    body = lambda m: m.feedback(m.delay(t) * g)
    whole = GR.noise() >> body(GR)
    front = gpu.Bank.from_graph(GR.noise(), V, sample_rate=SR, flush_denormals=True)
    eff = gpu.Bank.feedback_tree(body(GR), V, sample_rate=SR)
    assert eff.kind == "feedback_delay"
    ch = gpu.Chain(front, eff, construction_hash=probe_hash(whole))
    got = host(ch.process(T, layout=LAYOUT_PLANAR))[:, :, :T]
    n = O.noise() >> body(O)
    n.set_sample_rate(SR)
    want = n.render_blocks(None, length=T)
    for v in (0, V - 1):
        assert_bit_equal(got[v], want, f"as constructed, instance {v}")
    seeds = np.arange(V, dtype=np.uint64) * 5 + 1
    ch.reset()
    ch.set_seed(seeds)
    got = host(ch.process(T, layout=LAYOUT_PLANAR))[:, :, :T]
    for v in (0, 3, V - 1):
        n = O.noise() >> body(O)
        n.set_sample_rate(SR)
        n.set_seed(int(seeds[v]))
        assert_bit_equal(got[v], n.render_blocks(None, length=T), f"set_seed, instance {v}")
    assert not np.array_equal(got[0], got[1])


# ---- the compiled route -----------------------------------------------------------------------------------------------------------------
G3, G6 = GR._db_amp(-3.0), GR._db_amp(-6.0)
T0, T1 = float(SECONDS(160)), float(SECONDS(213))
COMPILED = {   # six graphs: each costs a run-time compile
    "readme_echo": lambda m: m.feedback(m.delay(T0) * G3),
    "readme_ping_pong": lambda m: m.feedback((m.delay(T0) | m.delay(T0)) >> m.reverse(2) * G6),
    "line_filter_mono": lambda m: m.feedback(m.delay(T0) >> m.fir(0.3, 0.4) >> m.lowpole_hz(3000.0) * 0.8),
    "loop_filter_mono": lambda m: m.feedback2(m.delay(T0), m.lowpass_hz(2500.0, 0.9) * 0.8),
    "line_filter_stereo": lambda m: m.feedback((m.delay(T0) >> m.bell_hz(2000.0, 0.8, 0.5) * 0.9 | m.delay(T1) >> m.bell_hz(3000.0, 1.1, 0.6) * 0.8) >> m.reverse(2)),
    "loop_filter_stereo": lambda m: m.feedback2((m.delay(T0) >> m.fir(0.2, 0.3, 0.2) | m.delay(T1) >> m.fir(0.1, 0.3, 0.3)) >> m.reverse(2),
                                                m.lowpole_hz(2500.0) * 0.9 | m.lowpole_hz(4000.0) * 0.8),
}


@pytest.mark.parametrize("name", sorted(COMPILED))
def test_feedback_tree_equals_the_compiled_route(gpu, name):
    V, T = 3, 64 * 10 + 7
    g = COMPILED[name](GR)
    fast = gpu.Bank.feedback_tree(g, V, sample_rate=SR)
    slow = gpu.Bank.from_graph(g, V, sample_rate=SR)
    assert fast.kind == "feedback_delay" and slow.kind.startswith("jit_")   # (from_graph does not route these graphs)
    x = signal(V, g.nin, T, 50 + len(name))
    a = run(fast, x, LAYOUT_VOICE_MINOR, MODE_PROCESS, [0, 64 * 3, T])
    b = run(slow, x, LAYOUT_VOICE_MINOR, MODE_PROCESS, [0, 64 * 3, T])
    assert fast.get_option("last_kernel") == 6 and slow.get_option("last_kernel") != 6
    assert np.abs(a[0, :, 2 * T // 3 + 170:]).max() > 1e-6
    assert_bit_equal(a, b, f"{name}: lane-per-frame kernel vs run-time compiled lane-per-voice graph")
    n = COMPILED[name](O)
    n.set_sample_rate(SR)
    assert_bit_equal(a[0], oracle_render(n, x[0], [0, 64 * 3, T]), f"{name}: the oracle")


# ---- the C++ host side ------------------------------------------------------------------------------------------------------------------
def test_cpp_bank_feedback_delay_renders_the_ping_pong():
    cpp_case("--gpu")
