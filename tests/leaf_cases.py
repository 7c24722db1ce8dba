"""The case table of tests/test_gpu_leaf_matrix.py: one row per leaf kind that register_leaf_kinds (fundsp_amd/csrc/fd_kinds_leaf.hip) registers.
Kept apart from the GPU test so that tests/test_leaf_cases.py can check, without a device, that the table has a row for every registered name and
that the oracle alone meets every side condition asked of the inputs (finite, still moving in the last launches, rings that fit at both rates).

A row holds the kind's name, `ring_frames`, `configure(bank, V)` (per-voice parameters, seeds and ring upload, ending at SR and reset),
`oracle(v)` (the oracle node of voice v in the same state) and `inputs(V, T, rng)` ([V][IN][T], None for generators).  Parameter ranges and oracle
constructors are those of the kind's own test (test_gpu_parity / nodes2 / nodes3 / delays / config4); nothing here is a new range.

The run every row is put through: launches CUTS[i] .. CUTS[i + 1] at SR (141 = two blocks, one 8-frame item, a 5-frame remainder; 1; 64; 83 frames: in
process mode every launch starts a new block), then set_sample_rate(SR2) and T_RATE frames more, then reset(), set_sample_rate(SR) and the first
launch again.  `reference(kind, executor)` is that run on the oracle, computed once."""
import functools
import zlib

import numpy as np

import oracle as O

f32 = np.float32
V = 67                      # one full wave plus a wave with three live lanes
V_BANK = 72                 # biquad_bank: voices come in groups of eight
CUTS = (0, 141, 142, 206, 289)
LAUNCHES = tuple(zip(CUTS[:-1], CUTS[1:]))
T_RATE = 77
T_ALL = CUTS[-1] + T_RATE
SR, SR2 = 48000.0, 44100.0
EXECUTORS = ("process", "tick")
TINY, NEGATIVE, SWEEP = 1, 3, 4     # voice 1: every audio channel scaled by 1e-30f; voice 3: negative frequency; voice 4: a frequency sweep
SHAPE_CASES = [("clip", 2.0, 0.0), ("clip_to", -0.3, 0.6), ("tanh", 1.5, 0.0), ("atan", 0.8, 0.0), ("softsign", 3.0, 0.0),
               ("crush", 8.0, 0.0), ("soft_crush", 6.0, 0.0), ("adaptive_tanh", 1.0, 0.05)]     # test_gpu_nodes2.SHAPE_CASES
SVF_NAMES = list(O.SVF_MODES)
BQ_MODES = ["resonator", "lowpass", "highpass", "bell"]


def rng_of(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def uni(key, lo, hi, n=V):
    return (lo + (hi - lo) * rng_of(*key).random(n)).astype(f32)


def logu(key, lo, hi, n=V):
    return (lo * (hi / lo) ** rng_of(*key).random(n)).astype(f32)


# ---- input channels: (V, T, rng) -> [V][T] -------------------------------------------------------------------------------------------------
def audio(scale=1.0):
    def f(V, T, rng):
        x = ((rng.random((V, T), dtype=f32) * f32(2) - f32(1)) * f32(scale)).astype(f32)
        x[TINY] *= f32(1e-30)       # the leaf units keep IEEE denormals, as the reference does outside Feedback
        return x
    return f


def stepped_audio(hold):
    """a stepped control signal in +-1 (test_follow_and_afollow)"""
    def f(V, T, rng):
        return np.repeat(audio()(V, (T + hold - 1) // hold, rng), hold, axis=1)[:, :T].copy()
    return f


def held(lo, hi, hold):
    """uniform in lo .. hi, held for `hold` frames (hold None: one value per voice)"""
    def f(V, T, rng):
        h = hold or T
        return np.repeat(lo + (hi - lo) * rng.random((V, (T + h - 1) // h)), h, axis=1)[:, :T].astype(f32)
    return f


def freq(lo, hi, hold, negative=False):
    """log-uniform in lo .. hi held for `hold` frames (None: one value per voice); voice SWEEP sweeps lo .. hi, voice NEGATIVE is negated"""
    def f(V, T, rng):
        h = hold or T
        x = np.repeat(lo * (hi / lo) ** rng.random((V, (T + h - 1) // h)), h, axis=1)[:, :T].astype(f32)
        x[SWEEP] = np.linspace(lo, hi, T)
        if negative:
            x[NEGATIVE] = -x[NEGATIVE]
        return x
    return f


def stretches(chan, spans=((50, 90), (135, 150))):
    """stretches of a constant value, one across the first launch boundaries: coefficients must not be re-derived (test_rez_with_inputs)"""
    def f(V, T, rng):
        x = chan(V, T, rng)
        for a, b in spans:
            x[:, a:b] = x[:, a - 1:a]
        return x
    return f


def wandering(lo, span):
    """(lo + span * u^2) * (1 + 0.2 * u') per frame (test_dsf); voices 5 and 6 sit on the pow(r, 1) and pow(r, 2) special cases"""
    def f(V, T, rng):
        x = ((lo + span * rng.random((V, 1)) ** 2) * (1.0 + 0.2 * rng.random((V, T)))).astype(f32)
        x[5] = 23000.0 * (1.0 + 0.01 * rng.random(T))      # (not a constant: 11 025 Hz is a period of exactly four frames at SR2)
        x[6] = 11025.0 * (1.0 + 0.01 * rng.random(T))
        return x
    return f


def dsf_roughness(V, T, rng):
    rough = (0.05 + 0.9 * rng.random(V)).astype(f32)
    return np.clip(rough[:, None] + 0.3 * (rng.random((V, T)) - 0.5), -0.2, 1.2).astype(f32)


def tap_delay(V, T, rng):
    """constant per voice (some beyond max_delay), voice 2 below min_delay, voice SWEEP modulated like a chorus (test_taps)"""
    x = np.repeat((0.0002 + 0.0036 * rng.random((V, 1))).astype(f32), T, axis=1)
    x[2] = 0.0
    x[SWEEP] = 0.0015 + 0.001 * np.sin(np.arange(T) / 9.0)
    return x


def pluck_input(V, T, rng):
    """silence with a burst of "extra string excitation" across the first two launch boundaries (test_pluck)"""
    x = np.zeros((V, T), dtype=f32)
    x[:, 130:150] = (rng.random((V, 20)) - 0.5).astype(f32)
    x[TINY] *= f32(1e-30)
    return x


def adsr_gate(V, T, rng):
    """gates whose edges fall inside launches (odd voices) and exactly on the launch boundaries 141, 142, 206 and 289 (all four classes); every voice is
    still in a moving segment of its envelope through the last launch and the launch after the rate change"""
    g = np.zeros((V, T), dtype=f32)
    for v in range(V):
        k = v % 4
        if k == 0:
            g[v, 1:141] = 1.0
            g[v, 206:289] = 1.0
        elif k == 1:
            g[v, 3 + v % 40:142] = 1.0
            g[v, 230:] = 0.5            # re-trigger during the release
        elif k == 2:
            g[v, 1:150 + v % 50] = 1.0
            g[v, 206:] = 1.0
        else:
            g[v, 20:142] = 1.0
            g[v, 142:206] = 0.5
            g[v, 289:] = 1.0
    return g


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
SEEDS = np.arange(V_BANK, dtype=np.uint64) * np.uint64(977) + np.uint64(5)


class Row:
    """`slots`: {slot name: scalar | [V]}; `make(v)`: the bare oracle node of voice v (of voices group * v .. for biquad_bank); `chans`: one channel
    maker per input; `seeded`: set_seed(SEEDS[v]) on both sides; `ring0`: [V][ring_frames] uploaded to ring 0; `table`: the wavetable the kind reads
    (built by the engine before the bank is made); `longest(sr)`: ring positions the longest delay of any voice takes at `sr`.
    `executors_agree`: the oracle's process and tick renders of the whole run are bit-identical (False: the row tells the two kernels apart).
    `reset_restores`: reset() then set_sample_rate(SR) brings the first launch back (False for adsr_live alone: EnvelopeIn::reset rewinds the time
    and leaves the closure's attack / release instants, envelope.rs:293-298, so the oracle's second first launch is another)."""

    def __init__(self, kind, slots, make, chans=(), seeded=False, ring_frames=0, longest=None, ring0=None, table=None, voices=V, group=1,
                 executors_agree=True, reset_restores=True):
        self.kind, self.slots, self.make, self.chans, self.seeded = kind, slots, make, tuple(chans), seeded
        self.ring_frames, self.longest, self.ring0, self.table = ring_frames, longest, ring0, table
        self.voices, self.group, self.executors_agree, self.reset_restores = voices, group, executors_agree, reset_restores

    def configure(self, bank, V):
        assert V == self.voices
        for name, value in self.slots.items():
            bank.set_param(name, value if np.isscalar(value) else np.asarray(value[:V], dtype=f32))
        if self.ring0 is not None:
            bank.set_ring(0, self.ring0)
        bank.set_sample_rate(SR)        # derives the coefficients (and the mls polynomial) from the parameters
        if self.seeded:
            bank.set_seed(SEEDS[:V])
        bank.reset()                    # Adaptive shapes start from reset()'s level, not new()'s: the run ends with a reset and must begin like it

    def oracle(self, v):
        n = self.make(v)
        n.set_sample_rate(SR)
        if self.seeded:
            n.set_seed(int(SEEDS[v]))
        n.reset()
        return n

    def inputs(self, V, T, rng):
        if not self.chans:
            return None
        x = np.stack([c(V, T, rng) for c in self.chans], axis=1).astype(f32)
        assert x.shape == (V, len(self.chans), T)
        return x


TABLE = {}


def row(kind, *a, **kw):
    assert kind not in TABLE
    TABLE[kind] = Row(kind, *a, **kw)


def _shape_slots(prefix, cases):
    return {f"{prefix}:shape": np.array([O.SHAPES[c[0]] for c in cases], dtype=f32),
            f"{prefix}:shape_p0": np.array([c[1] for c in cases], dtype=f32),
            f"{prefix}:shape_p1": np.array([c[2] for c in cases], dtype=f32),
            # Adaptive<Tanh>(timescale = p1): the node derives its smoothing itself -- Shaper at every set_sample_rate (shape.rs:197-200, 232-234), the
            # nonlinear biquads once, at Adaptive::new's DEFAULT_SR (their set_sample_rate never reaches the shape, biquad.rs:535-538)
            f"{prefix}:shape_timescale": np.array([c[2] if c[0] == "adaptive_tanh" else 0.0 for c in cases], dtype=f32)}


def _build():
    A = audio()
    row("pass", {}, lambda v: O.pass_(), [A])
    row("tick", {}, lambda v: O.tick(), [A])
    row("sine", {}, lambda v: O.sine(), [freq(20.0, 20000.0, 1, negative=True)], seeded=True, executors_agree=False)
    row("noise", {}, lambda v: O.noise(), seeded=True)

    # -- state variable filters and biquads (test_gpu_parity)
    k = "fixed_svf"
    fc, q, g = logu((k, "fc"), 20.0, 20000.0).clip(20, 0.45 * SR), uni((k, "q"), 0.3, 5.3), uni((k, "gain"), 0.25, 3.25)
    modes = np.arange(V) % 9
    row(k, {":mode": modes.astype(f32), ":cutoff": fc, ":q": q, ":gain": g},
        lambda v: O._fsvf(SVF_NAMES[modes[v]], float(fc[v]), float(q[v]), float(g[v])), [A])
    m3, m4 = np.arange(V) % 6, 6 + np.arange(V) % 3
    row("svf3", {":mode": m3.astype(f32)}, lambda v: O.svf(SVF_NAMES[m3[v]]), [A, freq(100.0, 8000.0, 16), held(0.5, 4.0, 16)])
    row("svf4", {":mode": m4.astype(f32)}, lambda v: O.svf(SVF_NAMES[m4[v]]), [A, freq(100.0, 8000.0, 16), held(0.5, 4.0, 16), held(0.5, 2.0, 16)])
    bfc, bq = logu(("biquad", "fc"), 20.0, 20000.0, V_BANK).clip(None, 0.49 * SR), logu(("biquad", "q"), 0.5, 10.0, V_BANK)
    coefs = np.stack([O.biquad_coefs("lowpass", SR, float(f), float(qq)) for f, qq in zip(bfc, bq)])
    bslots = {f":{n}": coefs[:, i].copy() for i, n in enumerate(("a1", "a2", "b0", "b1", "b2"))}
    row("biquad", bslots, lambda v: O.biquad(*coefs[v]), [A])

    def bank_of_eight(g):           # one BiquadBank<f32x8> per eight voices, voice = instance * 8 + lane (biquad_bank.rs:73-96)
        n = O.biquad_bank()
        for lane in range(8):
            O.set_biquad_bank(n, lane, coefs[g * 8 + lane])
        return n
    row("biquad_bank", bslots, bank_of_eight, [A], voices=V_BANK, group=8)
    k = "butterpass_hz"
    bf = logu((k, "fc"), 50.0, 10000.0)
    row(k, {":cutoff": bf}, lambda v: O.butterpass_hz(float(bf[v])), [A])
    row("butterpass", {}, lambda v: O.butterpass(), [A, freq(100.0, 8000.0, 16)])
    k = "resonator_hz"
    rf, rq = logu((k, "fc"), 50.0, 10000.0), uni((k, "q"), 1.0, 21.0)
    row(k, {":center": rf, ":q": rq}, lambda v: O.Node(O.lib().o_resonator(1, float(rf[v]), float(rq[v]))), [A])
    row("resonator", {}, lambda v: O.Node(O.lib().o_resonator(3, 440.0, 1.0)), [A, freq(100.0, 8000.0, 16), held(0.5, 4.0, 16)])
    k = "moog_hz"
    mf, mq = logu((k, "fc"), 50.0, 10000.0), uni((k, "q"), 0.1, 0.9)
    row(k, {":cutoff": mf, ":q": mq}, lambda v: O.moog_hz(float(mf[v]), float(mq[v])), [A])
    row("moog", {}, lambda v: O.moog(), [A, freq(100.0, 8000.0, 1), held(0.05, 0.7, 1)])
    for n in (2, 3):
        w = uni((f"fir{n}", "w"), -0.5, 0.5, V * n).reshape(V, n) + (f32(0.25), f32(0.5), f32(0.25))[:n]   # around test_fir_and_tick's weights
        row(f"fir{n}", {f":w[{i}]": w[:, i].copy() for i in range(n)}, lambda v, w=w: O.fir(*w[v]), [A])

    # -- the config-4 path (test_gpu_config4)
    for k in ("saw", "square", "triangle"):
        row(k, {}, lambda v, k=k: O.wavesynth(k), [freq(20.0, 18000.0, None, negative=True)], seeded=True, table=k, executors_agree=False)
    k = "adsr_live"
    a, d, s, r = uni((k, "a"), 0.001, 0.011), uni((k, "d"), 0.002, 0.022), uni((k, "s"), 0.2, 0.9), uni((k, "r"), 0.002, 0.022)
    row(k, {":attack": a, ":decay": d, ":sustain": s, ":release": r},
        lambda v: O.adsr_live(float(a[v]), float(d[v]), float(s[v]), float(r[v])), [adsr_gate], seeded=True, executors_agree=False, reset_restores=False)
    pans = np.linspace(-1.3, 1.3, V).astype(f32)     # beyond +-1: clamp11
    row("pan", {":pan": pans}, lambda v: O.pan(float(pans[v])), [A])

    # -- one-pole filters, pink, morph (test_gpu_nodes2)
    for k, mk in (("lowpole_hz", O.lowpole_hz), ("highpole_hz", O.highpole_hz), ("dcblock_hz", O.dcblock_hz), ("allpole_delay", O.allpole_delay)):
        p = uni((k, "p"), 0.05, 2.05) if k == "allpole_delay" else logu((k, "p"), 20.0, 10000.0)
        row(k, {":delay" if k == "allpole_delay" else ":cutoff": p}, lambda v, p=p, mk=mk: mk(float(p[v])), [A])
    row("lowpole", {}, lambda v: O.lowpole(), [A, freq(100.0, 5100.0, 32)])
    row("highpole", {}, lambda v: O.highpole(), [A, freq(100.0, 5100.0, 32)])
    row("allpole", {}, lambda v: O.allpole(), [A, held(0.2, 3.2, 32)])
    row("pinkpass", {}, lambda v: O.pinkpass(), [A])
    row("morph", {}, lambda v: O.morph(), [A, freq(100.0, 5100.0, 32), held(0.5, 4.5, 32), held(-1.0, 1.0, 32)])

    # -- test_gpu_nodes3
    k = "rez_hz"
    zf, zq, band = uni((k, "fc"), 100.0, 6100.0), uni((k, "q"), 0.05, 0.95), (np.arange(V) % 2).astype(f32)
    row(k, {":bandpass": band, ":cutoff": zf, ":q": zq},
        lambda v: (O.bandrez_hz if band[v] else O.lowrez_hz)(float(zf[v]), float(zq[v])), [A])
    row("rez", {":bandpass": band}, lambda v: O.bandrez() if band[v] else O.lowrez(),
        [A, stretches(freq(200.0, 3200.0, 1)), stretches(held(0.1, 0.9, 1))])
    rt, rel = uni(("follow", "rt"), 0.0005, 0.0505), uni(("follow", "rel"), 0.0005, 0.0505)
    row("follow", {":response_time": rt}, lambda v: O.follow(float(rt[v])), [stepped_audio(32)])
    row("afollow", {":attack_time": rt, ":release_time": rel}, lambda v: O.afollow(float(rt[v]), float(rel[v])), [stepped_audio(32)])
    bits = np.array([5, 10, 29, 31])[np.arange(V) % 4]
    row("mls", {":bits": bits.astype(f32)}, lambda v: O.mls_bits(int(bits[v])), seeded=True)
    k = "pluck"
    pf = (60.0 + 2000.0 * rng_of(k, "f").random(V) ** 2).astype(f32)
    gps, damp = uni((k, "gps"), 0.1, 0.95), uni((k, "damp"), 0.0, 1.0)
    exc = rng_of(k, "exc").uniform(-1, 1, (V, 1024)).astype(f32)        # >= sample_rate / 60 Hz - 1 samples
    row(k, {":frequency": pf, ":gain_per_second": gps, ":high_frequency_damping": damp},
        lambda v: O.pluck(float(pf[v]), float(gps[v]), float(damp[v]), exc[v]), [pluck_input], ring_frames=1024, ring0=exc,
        longest=lambda sr: int(np.floor(sr / float(pf.min()) - 1.2)))
    TAU = f32(6.2831855)
    ea, ek, hz = uni(("lfo_exp", "a"), 0.2, 1.2), uni(("lfo_exp", "k"), 0.5, 40.5), uni(("lfo_sine_hz", "hz"), 0.2, 15.2)
    row("lfo_exp", {"0:a": ea, "0:k": ek}, lambda v: O.lfo(lambda t: ea[v] * O.m_expf(-t * ek[v])), seeded=True, executors_agree=False)

    def lfo_sine(v):
        def sine(t):
            u = O.m_sinf(t * hz[v] * TAU) * f32(0.5) + f32(0.5)
            return f32(0.25) * (f32(1.0) - u) + f32(2.0) * u
        return O.lfo(sine)
    row("lfo_sine_hz", {"0:hz": hz, "0:lo": 0.25, "0:hi": 2.0}, lfo_sine, seeded=True, executors_agree=False)
    row("lfo2_exp", {}, lambda v: O.lfo2(lambda t, s: O.m_expf(-t * s)), [held(1.0, 31.0, 50)], seeded=True, executors_agree=False)
    spacing = (1 + np.arange(V) % 2).astype(f32)
    rough = uni(("dsf_r", "rough"), 0.05, 0.95)
    rough[:3] = [0.0, 1.0, 0.5]                                         # clamped to 0.0001 / 0.9999 by set_roughness
    row("dsf_r", {":harmonic_spacing": spacing, ":roughness": rough},
        lambda v: (O.dsf_saw_r if spacing[v] == 1.0 else O.dsf_square_r)(float(rough[v])), [wandering(30.0, 8000.0)], seeded=True)
    row("dsf", {":harmonic_spacing": spacing}, lambda v: O.dsf_saw() if spacing[v] == 1.0 else O.dsf_square(),
        [wandering(30.0, 8000.0), dsf_roughness], seeded=True)

    # -- delay lines (test_gpu_delays)
    times = np.concatenate([[0.0, 1.0 / SR, 3.0 / SR], np.linspace(0.0002, 0.004, V - 3)]).astype(f32)
    row("delay", {":time": times}, lambda v: O.delay(float(times[v])), [A], ring_frames=512,
        longest=lambda sr: int(round(float(times.max()) * sr)) + 1)
    max_d = 0.003
    row("tap", {":min_delay": 0.0005, ":max_delay": max_d}, lambda v: O.tap(0.0005, max_d), [A, tap_delay], ring_frames=1024,
        longest=lambda sr: 1 << int(np.ceil(np.log2(np.ceil(f32(max_d) * f32(sr)) + 11))))
    row("tap_linear", {":min_delay": 0.0, ":max_delay": max_d}, lambda v: O.tap_linear(0.0, max_d), [A, tap_delay], ring_frames=1024,
        longest=lambda sr: 1 << int(np.ceil(np.log2(np.ceil(f32(max_d) * f32(sr)) + 2))))
    eta = np.linspace(-0.8, 0.8, V + 1)[:V].astype(f32)       # (an even count: no voice at exactly 0, where the node is its inner node)
    row("allnest_delay", {":coefficient": eta, "0:time": 0.003}, lambda v: O.allnest_c(float(eta[v]), O.delay(0.003)), [A], ring_frames=256,
        longest=lambda sr: int(round(float(f32(0.003)) * sr)) + 1)
    row("allnest_tick", {":coefficient": eta}, lambda v: O.allnest_c(float(eta[v]), O.tick()), [A])
    row("allnest_pass", {":coefficient": eta}, lambda v: O.allnest_c(float(eta[v]), O.pass_()), [A])

    # -- waveshapers, phase oscillators, chaos, nonlinear biquads (test_gpu_nodes2)
    cases = [SHAPE_CASES[v % len(SHAPE_CASES)] for v in range(V)]
    row("shape", _shape_slots("", cases), lambda v: O.shape(*cases[v]), [audio(2.0)], executors_agree=False)
    for k in ("ramp", "poly_saw", "poly_square", "poly_pulse"):
        row(k, {}, lambda v, k=k: O.Node(O.lib().o_phase_osc(O.OSCS[k])),
            [freq(2500.0 if k in ("poly_square", "poly_pulse") else 20.0, 10000.0, None, negative=True)] + ([held(0.1, 0.9, None)] if k == "poly_pulse" else []), seeded=True)
    row("rossler", {}, lambda v: O.rossler(), [freq(110.0, 1000.0, None)], seeded=True)
    row("lorenz", {}, lambda v: O.lorenz(), [freq(110.0, 1000.0, None)], seeded=True)
    mode_i, shape_i = np.arange(V) % 4, (np.arange(V) // 4 + 3) % len(SHAPE_CASES)
    nl = [SHAPE_CASES[s] for s in shape_i]
    for k, dirty in (("fbiquad_hz", False), ("dbiquad_hz", True)):
        c, nq, ng = logu((k, "center"), 200.0, 4000.0), uni((k, "q"), 0.7, 10.7), uni((k, "gain"), 0.5, 2.5)
        slots = {":mode": np.array([O.BQ_KINDS[BQ_MODES[m]] for m in mode_i], dtype=f32), ":center": c, ":q": nq, ":gain": ng}
        for which in ([0, 1] if dirty else [0]):
            slots.update(_shape_slots(str(which), nl))
        row(k, slots, lambda v, dirty=dirty, c=c, nq=nq, ng=ng: O.nlbiquad(dirty, 1, BQ_MODES[mode_i[v]], *nl[v], float(c[v]), float(nq[v]), float(ng[v])),
            [A])
    for k, dirty, ni in (("fbiquad3", False, 3), ("fbiquad4", False, 4), ("dbiquad3", True, 3), ("dbiquad4", True, 4)):
        mode = "bell" if ni == 4 else "lowpass"
        slots = {":mode": float(O.BQ_KINDS[mode])}
        for which in ([0, 1] if dirty else [0]):
            slots.update({f"{which}:shape": float(O.SHAPES["softsign"]), f"{which}:shape_p0": 0.5, f"{which}:shape_p1": 0.0})
        row(k, slots, lambda v, dirty=dirty, ni=ni, mode=mode: O.nlbiquad(dirty, ni, mode, "softsign", 0.5, 0.0),
            [A, freq(300.0, 3300.0, 32), held(0.7, 5.7, 32)] + ([held(0.5, 2.5, 32)] if ni == 4 else []))


_build()


# ---- the run on the oracle -------------------------------------------------------------------------------------------------------------------
def oracle_launch(node, x, frames, executor):
    """[inputs][frames] (None for a generator) -> [outputs][frames]; in process mode the launch starts a new block"""
    if executor == "process":
        return node.render_blocks(x, length=frames, block=64)
    return node.render_ticks(x, length=frames)


def row_inputs(kind):
    r = TABLE[kind]
    return r.inputs(r.voices, T_ALL, rng_of(kind, "inputs"))


@functools.lru_cache(maxsize=None)
def reference(kind, executor):
    """(x [V][IN][T_ALL] or None, want [V][OUT][T_ALL], again [V][OUT][CUTS[1]]): the four launches at SR and T_RATE frames at SR2 in `want`; the first
    launch rendered again after reset() and set_sample_rate(SR) in `again`.  Read-only: shared by every test of the (kind, executor)."""
    r = TABLE[kind]
    x = row_inputs(kind)
    want, again = [], []
    for g in range(r.voices // r.group):
        n = r.oracle(g)
        xs = None if x is None else np.ascontiguousarray(x[g] if r.group == 1 else x[g * r.group:(g + 1) * r.group, 0])
        cut = lambda a, b: None if xs is None else np.ascontiguousarray(xs[:, a:b])
        parts = [oracle_launch(n, cut(a, b), b - a, executor) for a, b in LAUNCHES]
        n.set_sample_rate(SR2)
        parts.append(oracle_launch(n, cut(CUTS[-1], T_ALL), T_RATE, executor))
        n.reset()
        n.set_sample_rate(SR)
        first = oracle_launch(n, cut(0, CUTS[1]), CUTS[1], executor)
        w = np.concatenate(parts, axis=1)
        if r.group == 1:
            want.append(w)
            again.append(first)
        else:               # the group's node has one channel per voice
            want.extend(w[:, None, :])
            again.extend(first[:, None, :])
    want, again = np.stack(want).astype(f32), np.stack(again).astype(f32)
    for a in (x, want, again):
        if a is not None:
            a.setflags(write=False)
    return x, want, again
