"""GPU parity of the filtered / per-instance Hadamard feedback delay networks (fdsp_fdn_network_create, Bank.fdn_network):

    line form:  split | multisplit >> fdn(stacki(|i| delay(t_i) [>> fir(w_i..)] [>> F_i] [* g_i])) >> join | multijoin
    loop form:  split | multisplit >> fdn2(stacki(|i| delay(t_i) [>> fir(w_i..)]), stacki(|i| F_i [* g_i])) >> join | multijoin

bit-exact against the oracle's generic Feedback / Feedback2 graph built per instance with that instance's parameters (both executors, both
layouts, ragged launches, reset, a change of rate, clone, a denormal tail), against the run-time compiled lane-per-voice rendering of the
same graph, and through Bank.from_graph's bus and chain routes."""
import numpy as np
import pytest

import oracle as O
from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR, MODE_PROCESS, MODE_TICK
from fundsp_amd import graph as GR
from test_gpu_fdn import delays_of, run
from test_gpu_parity import assert_bit_equal

pytestmark = pytest.mark.gpu
SR = 48000.0


def params(n, V, filt, taps, gain, per_voice, seed, delay_range=None, delay_samples=None):
    """Bank.fdn_network keyword arguments: per-line values, and with per_voice a [V, n] spread of room sizes / cutoffs / gains;
    delay_range: (lo, hi) seconds in place of the doc example's 0.01 .. 0.03; delay_samples: the delays themselves, [n] or (per_voice)
    [V, n] whole samples at SR, taken as they are"""
    rng = np.random.default_rng(seed)
    base = np.array(delays_of(n, *delay_range) if delay_range else delays_of(n), dtype=np.float32)
    p = {}
    if delay_samples is not None:
        k = np.asarray(delay_samples, dtype=np.float64)
        assert k.shape == ((V, n) if per_voice else (n,)) and np.all(k == np.round(k))
        p["delays"] = (k / SR).astype(np.float32).astype(np.float64)   # (the f32 seconds delay(t: f32) takes)
    elif per_voice:
        room = np.linspace(1.0, 1.6, V, dtype=np.float32)[:, None]
        p["delays"] = (base[None, :] * room).astype(np.float32).astype(np.float64)
    else:
        p["delays"] = base.astype(np.float64)
    if taps:
        w = (rng.random((n, taps), dtype=np.float32) * 0.5 + 0.2).astype(np.float32)
        p["weights"] = w / np.float32(taps)
    if filt is not None:
        p["filter"] = filt
        c = np.float32(1500.0) + np.arange(n, dtype=np.float32) * np.float32(97.0)
        p["cutoff"] = (c[None, :] * np.linspace(1.0, 2.0, V, dtype=np.float32)[:, None]).astype(np.float32) if per_voice else c
        if filt != "lowpole":
            p["q"] = np.full(n, 0.8, np.float32)
            p["gain"] = np.full(n, 0.5, np.float32) if filt == "highshelf" else np.full(n, 1.0, np.float32)
    if gain:
        g = np.float32(0.97) - np.arange(n, dtype=np.float32) * np.float32(0.004)
        p["line_gain"] = (g[None, :] * np.linspace(1.0, 0.9, V, dtype=np.float32)[:, None]).astype(np.float32) if per_voice else g
    return p


def at(a, v, i):
    a = np.asarray(a)
    return a[v, i] if a.ndim == 2 else a[i]


def oracle_network(n, p, v, place, nin, nout, sr=SR):
    """the generic Feedback / Feedback2 graph of instance v"""
    filt, taps = p.get("filter"), (0 if "weights" not in p else p["weights"].shape[-1])

    def fir_of(i):
        w = p["weights"]
        return O.fir(*(w[v, i] if w.ndim == 3 else w[i]))

    def f_of(i):
        c = float(at(p["cutoff"], v, i))
        f = O.lowpole_hz(c) if filt == "lowpole" else O._fsvf(filt, c, float(at(p["q"], v, i)), float(at(p["gain"], v, i)))
        return f * float(at(p["line_gain"], v, i)) if "line_gain" in p else f

    def x_of(i):
        x = O.delay(float(at(p["delays"], v, i)))
        if taps:
            x = x >> fir_of(i)
        if place == "line":
            if filt is not None:
                x = x >> f_of(i)
            elif "line_gain" in p:
                x = x * float(at(p["line_gain"], v, i))
        return x

    head = O.split(n) if nin == 1 else O.multisplit(2, n // 2)
    tail = O.join(n) if nout == 1 else O.multijoin(2, n // 2)
    core = O.fdn(O.stacki(n, x_of)) if place == "line" else O.fdn2(O.stacki(n, x_of), O.stacki(n, f_of))
    net = head >> core >> tail
    net.set_sample_rate(sr)
    return net


def device_graph(n, p, place, nin, nout, V):
    """the same network in graph notation (per-voice arrays where the parameters are [V, n])"""
    filt, taps = p.get("filter"), (0 if "weights" not in p else p["weights"].shape[-1])

    def col(a, i):
        a = np.asarray(a)
        return np.ascontiguousarray(a[:, i].astype(np.float32)) if a.ndim == 2 else float(a[i])

    def f_of(i):
        c = col(p["cutoff"], i)
        f = GR.lowpole_hz(c) if filt == "lowpole" else GR._fsvf(filt, c, col(p["q"], i), col(p["gain"], i))
        return f * col(p["line_gain"], i) if "line_gain" in p else f

    def x_of(i):
        x = GR.delay(col(p["delays"], i))
        if taps:
            x = x >> GR.fir(*[float(w) for w in p["weights"][i]])
        if place == "line" and filt is not None:
            x = x >> f_of(i)
        return x

    head = GR.split(n) if nin == 1 else GR.multisplit(2, n // 2)
    tail = GR.join(n) if nout == 1 else GR.multijoin(2, n // 2)
    core = GR.fdn(GR.stacki(n, x_of)) if place == "line" else GR.fdn2(GR.stacki(n, x_of), GR.stacki(n, f_of))
    return head >> core >> tail


def signal(V, nin, T, seed, impulse=None):
    """noise that stops at 2T/3; instance 1 in the denormal range; `impulse`: an instance driven by one unit sample instead"""
    rng = np.random.default_rng(seed)
    x = (rng.random((V, nin, T), dtype=np.float32) * 2 - 1).astype(np.float32)
    x[:, :, 2 * T // 3:] = 0.0
    x[1] *= np.float32(1e-30)                            # an instance that lives in the denormal range: Feedback2::new flushes
    x[1, :, 2 * T // 3 - 40:2 * T // 3] = np.float32(3e-39)
    if impulse is not None:
        x[impulse] = 0.0
        x[impulse, 0, 0] = 1.0
    return x


# The smallest ring that can still go wrong: delays of 0.003 .. 0.005 s are 144 .. 240 samples at 48 kHz (above the 128-sample rule), so the
# rings have 256 slots, the write window of the 1 933 frames below wraps seven times, and the ragged launches of 77, 1 and 333 frames cross
# the mirror zone (the first 64 slots, copied behind the ring) slot by slot.
SHORT_RING_DELAYS = (0.003, 0.005)

CASES = [  # lines, filter, place, taps, gain, inputs, outputs, per-voice parameters, instances, delay range (None: the doc example's)
    (32, "lowpole", "loop", 3, True, 2, 2, True, 66, None),
    (16, "lowpass", "line", 0, True, 1, 1, False, 6, None),
    (2, "highshelf", "loop", 3, False, 1, 2, False, 6, None),
    (16, "highshelf", "line", 3, False, 2, 1, True, 66, None),
    (32, "lowpass", "line", 2, True, 1, 1, True, 5, None),
    # the filtered kernel without a filter (its instantiation of the steps the generic kernel shares with it), a workgroup with one live wave
    (16, None, "line", 3, False, 1, 1, False, 5, None),
    (4, None, "line", 2, True, 2, 2, True, 5, None),
    (2, "lowpole", "loop", 3, True, 1, 2, False, 5, SHORT_RING_DELAYS),
]
# (the ids pytest would give the first nine columns: a row's id does not change when a column is added behind them)
CASE_IDS = ["-".join(str(v) for v in r[:9]) for r in CASES]


@pytest.mark.parametrize("mode", [MODE_PROCESS, MODE_TICK])
@pytest.mark.parametrize("layout", [LAYOUT_PLANAR, LAYOUT_VOICE_MINOR])
@pytest.mark.parametrize("n,filt,place,taps,gain,nin,nout,per_voice,V,delay_range", CASES, ids=CASE_IDS)
def test_network_matches_oracle(gpu, n, filt, place, taps, gain, nin, nout, per_voice, V, delay_range, layout, mode):
    T = 64 * 30 + 13
    p = params(n, V, filt, taps, gain, per_voice, n + taps, delay_range)
    if delay_range == SHORT_RING_DELAYS:   # (the case is about a 256-slot ring)
        assert 128 <= int(np.round(p["delays"] * SR).min()) and int(np.round(p["delays"] * SR).max()) + 1 <= 256
    b = gpu.Bank.fdn_network(V, n, place=place, inputs=nin, outputs=nout, sample_rate=SR, **p)
    assert b.kind == "fdn_network" and b.inputs() == nin and b.outputs() == nout
    x = signal(V, nin, T, 11 * n + taps)
    cuts = [0, 64, 141, 142, 475, 64 * 12 + 475, T]          # ragged launches: 64, 77, 1, 333, 768, ..
    got = run(b, x, layout, mode, cuts)
    assert b.get_option("last_kernel") == 6
    for v in sorted({0, 1, V // 2, V - 1}):
        net = oracle_network(n, p, v, place, nin, nout)
        want = [net.render_blocks(x[v][:, a:e]) if mode == MODE_PROCESS else net.render_ticks(x[v][:, a:e]) for a, e in zip(cuts[:-1], cuts[1:])]
        assert_bit_equal(got[v], np.concatenate(want, axis=1), f"{place} fdn<{n}> {filt} fir{taps} {nin}->{nout} instance {v}")
    assert np.abs(got[0, :, 2 * T // 3 + 200:]).max() > 1e-6          # the tail recirculates
    assert not np.any((got[1] != 0) & (np.abs(got[1]) < np.float32(1.17549435e-38)))   # no denormal reaches the output
    b.reset()   # reset mid-stream: the same first launches again
    assert_bit_equal(run(b, x[:, :, :700], layout, mode, [0, 64, 700]), got[:, :, :700], "after reset")


@pytest.mark.parametrize("mode", [MODE_PROCESS, MODE_TICK])
@pytest.mark.parametrize("n", [2, 16])
def test_unfiltered_network_equals_the_generic_fdn_kernel(gpu, n, mode):
    """k_fdn_frames_generic and k_fdn_frames_filtered are two instantiations of the same block steps (fd_fdn_frames.hpp): the same network
    through fdsp_fdn_create and, with its weights repeated per line and no filter, through fdsp_fdn_network_create gives identical samples
    over full, ragged and one-frame launches.  No oracle: this holds the two kernels against each other."""
    V, T, w = 5, 64 * 9 + 13, (0.2, 0.4, 0.2)
    delays = delays_of(n, *SHORT_RING_DELAYS)   # 144 .. 240 samples: the network recirculates (and its 256-slot rings wrap) within the 589 frames
    a = gpu.Bank.fdn(V, n, delays, 3, w)
    a.set_sample_rate(SR)
    b = gpu.Bank.fdn_network(V, n, delays, weights=np.tile(np.array(w, dtype=np.float32), (n, 1)), filter=None, sample_rate=SR)
    assert a.kind == "fdn" and b.kind == "fdn_network"
    x = signal(V, 1, T, 41 + n)
    cuts = [0, 64, 141, 142, T]
    ya = run(a, x, LAYOUT_PLANAR, mode, cuts)
    yb = run(b, x, LAYOUT_PLANAR, mode, cuts)
    assert a.get_option("last_kernel") == 6 and b.get_option("last_kernel") == 6
    assert np.abs(ya[0]).max() > 1e-3
    assert_bit_equal(yb, ya, f"fdn<{n}> fir3: filtered kernel without a filter vs generic kernel")


@pytest.mark.parametrize("place,filt", [("loop", "lowpole"), ("line", "highshelf")])
def test_clone_and_sample_rate_move_keep_filter_and_feedback_state(gpu, place, filt):
    """fdsp_bank_clone continues where the bank stands; 48 -> 96 kHz in the middle of a tail empties the lines but keeps the Fir carry,
    the filter states and the feedback value (Feedback2::set_sample_rate, feedback.rs:254-257) -- as the oracle graph does"""
    n, V, T = 16, 7, 64 * 24 + 5
    p = params(n, V, filt, 3, True, True, 3)
    b = gpu.Bank.fdn_network(V, n, place=place, sample_rate=SR, **p)
    x = signal(V, 1, T, 5)
    x[:, :, 1000:] = 0.0
    a1 = run(b, x[:, :, :1000], LAYOUT_PLANAR, MODE_PROCESS, [0, 1000])
    c = b.clone()
    a2 = run(b, x[:, :, 1000:], LAYOUT_PLANAR, MODE_PROCESS, [0, 77, T - 1000])
    c2 = run(c, x[:, :, 1000:], LAYOUT_PLANAR, MODE_PROCESS, [0, T - 1000])
    assert_bit_equal(c2, a2, "the clone continues like the original")
    b.set_sample_rate(96000.0)
    a3 = run(b, x, LAYOUT_VOICE_MINOR, MODE_PROCESS, [0, 333, T])
    assert np.abs(a3[:, :, :64]).max() > 0.0                      # the feedback value and the filter states survived the move
    for v in (0, 3, V - 1):
        net = oracle_network(n, p, v, place, 1, 1)
        want = np.concatenate([net.render_blocks(x[v][:, :1000]), net.render_blocks(x[v][:, 1000:])], axis=1)
        assert_bit_equal(np.concatenate([a1, a2], axis=2)[v], want, f"48 kHz instance {v}")
        net.set_sample_rate(96000.0)
        assert_bit_equal(a3[v], net.render_blocks(x[v]), f"96 kHz instance {v}")


@pytest.mark.parametrize("place", ["line", "loop"])
def test_from_graph_takes_the_network_kernel_and_equals_the_run_time_compiled_graph(gpu, place):
    """Bank.from_graph recognises the shape (graph.fdn_network_plan); fdn_kernel=False compiles the same graph and renders it one lane per voice.
    Every instance, per-voice parameters: identical samples."""
    n, V, T = 8, 9, 64 * 20 + 7
    filt = "lowpole" if place == "loop" else "lowpass"
    p = params(n, V, filt, 3, True, True, 17)
    g = device_graph(n, p, place, 2, 2, V)
    assert GR.fdn_plan(g) is None and GR.fdn_network_plan(g, V) is not None
    fast = gpu.Bank.from_graph(g, V, sample_rate=SR)
    slow = gpu.Bank.from_graph(g, V, sample_rate=SR, fdn_kernel=False)
    assert fast.kind == "fdn_network" and slow.kind.startswith("jit_")
    x = signal(V, 2, T, 23)
    a = run(fast, x, LAYOUT_VOICE_MINOR, MODE_PROCESS, [0, 64 * 7, T])
    b = run(slow, x, LAYOUT_VOICE_MINOR, MODE_PROCESS, [0, 64 * 7, T])
    assert fast.get_option("last_kernel") == 6 and slow.get_option("last_kernel") != 6
    assert_bit_equal(a, b, f"{place} form: lane-per-frame kernel vs run-time compiled lane-per-voice graph")
    if place == "line":
        # a delay under two blocks at the creation rate: FDSP_EINVAL from the C ABI, and from_graph falls back to the compiled graph
        # (the same graph type as above: no further compile)
        short = dict(p)
        short["delays"] = np.array(p["delays"], copy=True)
        short["delays"][:, 2] = 100.0 / SR
        with pytest.raises(gpu.FdspError, match="128 samples"):
            gpu.Bank.fdn_network(V, n, place=place, inputs=2, outputs=2, sample_rate=SR, **short)
        fb = gpu.Bank.from_graph(device_graph(n, short, place, 2, 2, V), V, sample_rate=SR)
        assert fb.kind == slow.kind


def test_bus_and_chain_routes(gpu):
    """`0.5 * net & 0.8 * multipass()` folds into the network bank's epilogue (fdsp_bank_set_bus); `front >> net` becomes a Chain of the front's
    compiled bank and the network bank -- both against the oracle"""
    import fundsp_amd

    n, V, T = 4, 5, 64 * 16 + 3
    p = params(n, V, "lowpole", 2, True, False, 29)
    net = device_graph(n, p, "loop", 2, 2, V)
    bus = 0.5 * net & 0.8 * GR.multipass(2)
    b = gpu.Bank.from_graph(bus, V, sample_rate=SR)
    assert b.kind == "fdn_network" and b.get_bus() == (2, 0.5, float(np.float32(0.8)))
    x = signal(V, 2, T, 31)
    got = run(b, x, LAYOUT_PLANAR, MODE_PROCESS, [0, 100, T])
    for v in (0, V - 1):
        o = 0.5 * oracle_network(n, p, v, "loop", 2, 2) & 0.8 * O.multipass(2)
        o.set_sample_rate(SR)
        assert_bit_equal(got[v], np.concatenate([o.render_blocks(x[v][:, :100]), o.render_blocks(x[v][:, 100:])], axis=1), f"bus instance {v}")
    line = device_graph(n, p, "line", 1, 1, V)
    ch = gpu.Bank.from_graph(GR.lowpole_hz(3000.0) >> line, V, sample_rate=SR)
    assert isinstance(ch, fundsp_amd.Chain) and ch.effect.kind == "fdn_network"
    x1 = signal(V, 1, T, 37)
    got = run(ch, x1, LAYOUT_PLANAR, MODE_PROCESS, [0, T])
    for v in (0, 2):
        o = O.lowpole_hz(3000.0) >> oracle_network(n, p, v, "line", 1, 1)
        o.set_sample_rate(SR)
        assert_bit_equal(got[v], o.render_blocks(x1[v]), f"chain instance {v}")


def test_invalid_networks(gpu):
    import ctypes as C

    from fundsp_amd import _lib

    with pytest.raises(gpu.FdspError, match="lines"):
        gpu.Bank.fdn_network(2, 12, [0.01] * 12, filter="lowpole", cutoff=1000.0)
    with pytest.raises(gpu.FdspError, match="loop form"):
        gpu.Bank.fdn_network(2, 4, [0.01] * 4, place="loop")
    with pytest.raises(gpu.FdspError, match="128 samples"):
        gpu.Bank.fdn_network(2, 4, [0.002] * 4, filter="lowpole", cutoff=1000.0, sample_rate=SR)       # 96 samples
    d = (C.c_double * 4)(*([0.01] * 4))
    net = _lib.FdnNetwork(lines=4, inputs=1, outputs=1, taps=0, filter=_lib.FDN_FILTER_SVF, svf_mode=8, place=0, per_instance=0, delays=d)
    h = C.c_void_p()
    assert gpu.lib().fdsp_fdn_network_create(2, C.byref(net), SR, C.byref(h)) < 0 and not h.value
    assert b"cutoff" in gpu.lib().fdsp_last_error()
    cut = (C.c_float * 4)(*([1000.0] * 4))
    net.cutoff = C.cast(cut, C.POINTER(C.c_float))
    net.q = C.cast(cut, C.POINTER(C.c_float))
    assert gpu.lib().fdsp_fdn_network_create(2, C.byref(net), SR, C.byref(h)) < 0 and b"gain" in gpu.lib().fdsp_last_error()
