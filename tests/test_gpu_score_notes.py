"""Scores rendered with one lane per NOTE (set_option("score_exec", SCORE_NOTES), fd_device.hpp render_score_notes_body).

The note path must compute what the voice path computes -- samples, voice state, clock -- bit for bit: against the oracle's Sequencer with
one fresh unit per note, against the default path, across split launches with the executor switched in between, with the notes of one
voice spread over several waves (the write-back goes through a staging image), for the write-back's owner (a zero-length note behind the
last rendered one, a voice in which nothing renders), mixed in chunks, on a kind with an input, on run-time compiled graphs and on every
ahead-of-time kind that reports "has_score_notes"."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from fundsp_amd import MODE_PROCESS, MODE_TICK, SCORE_NOTES, SCORE_VOICES
from fundsp_amd import workloads as W
from score_cases import SPLIT, SR, T, V, Score, build_score, pool_output
from test_gpu_config4 import tables  # noqa: F401  (fixture: the oracle's wavetables installed on the device)
from test_gpu_parity import assert_bit_equal
from test_gpu_score import fm_bank, fm_case, fm_note_params, fm_oracle, fm_rows, voices_of

pytestmark = pytest.mark.gpu
MODES = [MODE_PROCESS, MODE_TICK]
LK_SCORE, LK_SCORE_NOTES = 9, 10


def notes_bank(make=fm_bank):
    b = make()
    b.set_option("score_exec", SCORE_NOTES)
    return b


def host(x):
    return x.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
def test_note_path_against_the_oracle(gpu, mode):
    """501: 70 voices, 597 frames, a few hundred notes -- several waves of notes with a partial last one"""
    sc, _, _ = fm_case()
    assert sc.n > 256 and sc.n % 64 != 0
    want, clock = fm_oracle(mode)
    b = fm_bank()
    assert b.get_option("score_exec") == SCORE_VOICES and b.get_option("has_score_notes") == 1
    b.set_option("score_exec", SCORE_NOTES)
    assert b.get_option("score_exec") == SCORE_NOTES
    got = voices_of(b.process_events(T, mode=mode))
    assert b.get_option("last_kernel") == LK_SCORE_NOTES
    for v in range(V):
        assert_bit_equal(got[v], want[v], f"note path, voice {v}")
    assert b.events_time() == clock


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mixed", [False, True])
def test_note_path_against_the_default_path(gpu, mode, mixed):
    a, b = fm_bank(), notes_bank()
    run = (lambda x: x.process_events_mix(T, mode=mode)) if mixed else (lambda x: x.process_events(T, mode=mode))
    want, got = host(run(a)), host(run(b))
    assert a.get_option("last_kernel") == LK_SCORE and b.get_option("last_kernel") == LK_SCORE_NOTES
    assert_bit_equal(got, want, "score_exec 1 vs 0")
    assert_bit_equal(b.get_state(), a.get_state(), "voice state, score_exec 1 vs 0")
    assert b.events_time() == a.events_time()
    assert np.abs(got).max() > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [(1, 1, 1), (0, 1, 0), (1, 0, 1)])
def test_split_launches_and_a_switch_of_executor_in_between(gpu, mode, order):
    """SPLIT == one launch == the oracle; with the option switched between the launches a note carried in was begun by the other executor"""
    import torch

    want, clock = fm_oracle(mode)
    b = fm_bank()
    parts = []
    for n, ex in zip(SPLIT, order):
        b.set_option("score_exec", ex)
        parts.append(b.process_events(n, mode=mode))
        assert b.get_option("last_kernel") == (LK_SCORE_NOTES if ex else LK_SCORE)
    got = voices_of(torch.cat(parts, dim=1))
    for v in range(V):
        assert_bit_equal(got[v], want[v], f"split launches {order} vs the oracle, voice {v}")
    assert b.events_time() == clock
    ref = fm_bank()
    for n in SPLIT:
        ref.process_events(n, mode=mode)
    assert_bit_equal(b.get_state(), ref.get_state(), f"voice state after split launches {order}")


def many_notes_case():
    """3 voices; voice 0 has about 200 notes of 3 - 12 frames with gaps of 0 - 3 frames and random fades over 64 * 40 + 13 frames"""
    rng = np.random.default_rng(551)
    Tm = 64 * 40 + 13
    voice, start, dur = [], [], []
    t = 2.0
    while t < Tm - 14:
        d = float(rng.integers(3, 13))
        voice.append(0), start.append(t), dur.append(d)
        t += d + float(rng.integers(0, 4))
    for v, (s, d) in ((1, (100.3, 900.0)), (2, (1500.0, 64.0))):
        voice.append(v), start.append(s), dur.append(d)
    start, dur = np.array(start), np.array(dur)
    s, e = start / SR, (start + dur) / SR
    for i in range(1, s.size):                                       # legato where the gap is 0: the same bits
        if voice[i] == voice[i - 1] and start[i] == start[i - 1] + dur[i - 1]:
            s[i] = e[i - 1]
            e[i] = s[i] + dur[i] / SR
    d = e - s
    fin = np.where(rng.random(s.size) < 0.5, d * rng.random(s.size), 0.0)
    fout = np.where(rng.random(s.size) < 0.5, d * rng.random(s.size), 0.0)
    sc = Score(voice, s, e, np.minimum(fin, d), np.minimum(fout, d), rng.integers(0, 2, s.size), {})
    assert 190 <= int(np.sum(sc.voice == 0)) <= 400
    return sc, Tm


def test_a_voice_whose_notes_fill_several_waves(gpu):
    """Two launches cut inside one of voice 0's early notes: in the second launch the carried-in note (lane 6 or so) and the last rendered
    note (a lane some waves later) are different notes -- the owner must not overwrite the slots the carried-in note still has to load"""
    import torch

    sc, Tm = many_notes_case()
    k_cut = 6
    T1 = int(round(sc.start[k_cut] * SR)) + 2                        # inside note 6 of voice 0 (every note has >= 3 frames)
    assert sc.start[k_cut] * SR < T1 - 1 and sc.end[k_cut] * SR > T1 + 0.6 and T1 < 64 * 2
    p, pn = W.fm_svf_params(3, SR), fm_note_params(sc.n, 552)

    def bank(ex):
        b = W.make_fm_svf_bank(3, SR, params=p)
        b.set_score(sc.voice, sc.start, sc.end, sc.fin, sc.fout, sc.fade, params=fm_rows(pn))
        b.set_option("score_exec", ex)
        return b

    seq = O.Sequencer(0, 1, SR)
    for k in range(sc.n):
        f, m = float(pn["f"][k]), float(pn["m"][k])
        n = O.sine_hz(f) * f * m + f >> O.sine() >> O.lowpass_hz(float(pn["fc"][k]), float(pn["q"][k]))
        n.set_seed(int(p["seed"][sc.voice[k]]))
        seq.push(sc.start[k], sc.end[k], int(sc.fade[k]), sc.fin[k], sc.fout[k], n)
    # (the first launch is not a multiple of 64 frames: the oracle renders the same two launches, block clocks and all)
    _, per1 = seq.render(T1, process=True)
    _, per2 = seq.render(Tm - T1, process=True)
    want = pool_output(sc, np.concatenate([per1, per2], axis=2), 3)
    a, b = bank(SCORE_VOICES), bank(SCORE_NOTES)
    outs = []
    for n in (T1, Tm - T1):
        oa, ob = a.process_events(n), b.process_events(n)
        assert b.get_option("last_kernel") == LK_SCORE_NOTES
        assert_bit_equal(host(ob), host(oa), f"launch of {n} frames, score_exec 1 vs 0")
        assert_bit_equal(b.get_state(), a.get_state(), f"voice state after the launch of {n} frames")
        outs.append(ob)
    got = voices_of(torch.cat(outs, dim=1))
    for v in range(3):
        assert_bit_equal(got[v], want[v], f"voice {v} vs the oracle")
    assert b.events_time() == seq.time()


@pytest.mark.parametrize("mode", MODES)
def test_the_write_back_owner(gpu, mode):
    """Voice 0 ends the launch with a zero-length note behind a rendered one; voice 1 has no rendered note (one note after the launch, one
    of zero length inside it); voice 2's last note ends exactly at the launch's last frame; voice 3 has no notes at all"""
    Tw = 64 * 3 + 7
    voice = [0, 0, 0, 1, 1, 2, 2]
    start = np.array([5.0, 100.0, 120.0, 50.0, Tw + 30.0, 10.0, Tw - 40.0]) / SR
    end = np.array([60.0, 120.0, 120.0, 50.0, Tw + 90.0, 30.0, float(Tw)]) / SR
    start[2] = end[2] = end[1]
    sc = Score(voice, start, end, np.zeros(7), np.zeros(7), np.ones(7, dtype=np.int32), {})
    p, pn = W.fm_svf_params(4, SR), fm_note_params(sc.n, 561)

    def bank(ex):
        b = W.make_fm_svf_bank(4, SR, params=p)
        b.set_score(sc.voice, sc.start, sc.end, sc.fin, sc.fout, sc.fade, params=fm_rows(pn))
        b.set_option("score_exec", ex)
        return b

    a, b = bank(SCORE_VOICES), bank(SCORE_NOTES)
    before = b.get_state()
    oa, ob = host(a.process_events(Tw, mode=mode)), host(b.process_events(Tw, mode=mode))
    assert_bit_equal(ob, oa, "samples, score_exec 1 vs 0")
    sa, sb = a.get_state(), b.get_state()
    assert_bit_equal(sb, sa, "voice state, score_exec 1 vs 0")
    assert_bit_equal(sb[:, 1], before[:, 1], "a voice in which nothing rendered stays untouched")
    assert_bit_equal(sb[:, 3], before[:, 3], "a voice without notes stays untouched")
    assert not np.array_equal(sb[:, 0].view(np.uint32), before[:, 0].view(np.uint32))
    slot = [n for n, _ in b.slots()].index(W.FM_SLOTS["cutoff"])
    assert sb[slot, 0] == pn["fc"][1], "the zero-length note's row must not reach the slots: the rendered note before it owns them"
    assert np.all(ob[0, Tw - 1, 2] != 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", [64, 128])
def test_mix_in_chunks(gpu, mode, chunk):
    per_bank, fused_bank, whole, chunked = fm_bank(), fm_bank(), notes_bank(), notes_bank()
    chunked.set_option("score_chunk_frames", chunk)
    assert chunked.get_option("score_chunk_frames") == chunk
    got = host(chunked.process_events_mix(T, mode=mode))
    assert chunked.get_option("last_kernel") == LK_SCORE_NOTES and chunked.get_option("score_scratch_frames") == chunk
    assert_bit_equal(got, host(gpu.sum_voices(per_bank.process_events(T, mode=mode))), "chunked note mix vs sum_voices(process_events)")
    assert_bit_equal(got, host(fused_bank.process_events_mix(T, mode=mode)), "chunked note mix vs the default path's fused mix")
    assert_bit_equal(got, host(whole.process_events_mix(T, mode=mode)), "chunked vs unchunked note mix")
    assert whole.get_option("score_scratch_frames") >= T
    assert_bit_equal(chunked.get_state(), fused_bank.get_state(), "voice state after the chunked mix")
    assert chunked.events_time() == fused_bank.events_time()
    with pytest.raises(gpu.FdspError):
        chunked.set_option("score_chunk_frames", 100)                # not a multiple of 64


def test_kind_with_an_input_in_two_launches_under_the_option(gpu):
    """svf_shape_svf over a per-voice noise stream, as tests/test_gpu_score.py plays it"""
    import torch

    Vg, T1 = 64 + 6, 64 * 4
    sc = build_score(521, voices=Vg)
    rng = np.random.default_rng(522)
    rows = {"0.0:cutoff": (200.0 * np.exp2(5.0 * rng.random(sc.n))).astype(np.float32), "0.0:q": (0.5 + 3.0 * rng.random(sc.n)).astype(np.float32),
            "1:cutoff": (50.0 * np.exp2(4.0 * rng.random(sc.n))).astype(np.float32), "1:q": (0.5 + rng.random(sc.n)).astype(np.float32)}

    def bank(ex):
        b = gpu.Bank("svf_shape_svf", Vg)
        for name, value in (("0.0:mode", O.SVF_MODES["lowpass"]), ("1:mode", O.SVF_MODES["highpass"]), ("0.1:shape", O.SHAPES["tanh"]), ("0.1:shape_p0", 1.0)):
            b.set_param(name, np.full(Vg, float(value), dtype=np.float32))
        b.set_sample_rate(SR)
        b.set_score(sc.voice, sc.start, sc.end, sc.fin, sc.fout, sc.fade, params=rows)
        b.set_option("score_exec", ex)
        return b

    x = (rng.random((Vg, 1, T), dtype=np.float32) * 2 - 1).astype(np.float32)
    d = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 2, 0))).cuda()
    a, b = bank(SCORE_VOICES), bank(SCORE_NOTES)
    assert b.get_option("has_score_notes") == 1
    for lo, hi in ((0, T1), (T1, T)):
        oa, ob = a.process_events(hi - lo, d[:, lo:hi].contiguous()), b.process_events(hi - lo, d[:, lo:hi].contiguous())
        assert b.get_option("last_kernel") == LK_SCORE_NOTES
        assert_bit_equal(host(ob), host(oa), f"frames {lo} .. {hi}, score_exec 1 vs 0")
        assert_bit_equal(b.get_state(), a.get_state(), f"voice state after frames {lo} .. {hi}")
    assert np.abs(host(ob)).max() > 0.01
    # mixed and chunked: a chunk's lanes read their inputs at an offset into rows that are longer than the chunk.  (svf_shape_svf has no
    # fused Sequencer mix, with either executor; a run-time compiled filter has.)
    from fundsp_amd import graph as GR

    g = GR.lowpass_hz(1200.0, 1.5)
    cutoff = [n for n, _, _ in g.slot_values() if n.endswith("cutoff")]

    def jit_bank(ex):
        m = gpu.Bank.from_graph(g, Vg, sample_rate=SR)
        m.set_score(sc.voice, sc.start, sc.end, sc.fin, sc.fout, sc.fade, params={cutoff[0]: rows["0.0:cutoff"]})
        m.set_option("score_exec", ex)
        return m

    m0, m1 = jit_bank(SCORE_VOICES), jit_bank(SCORE_NOTES)
    m1.set_option("score_chunk_frames", 128)
    want, got = host(m0.process_events_mix(T, d)), host(m1.process_events_mix(T, d))
    assert m1.get_option("last_kernel") == LK_SCORE_NOTES
    assert_bit_equal(got, want, "chunked mix of a graph with an input")
    assert_bit_equal(m1.get_state(), m0.get_state(), "voice state after the chunked mix of a graph with an input")
    assert np.abs(got).max() > 0.01


@pytest.mark.parametrize("mode", MODES)
def test_run_time_compiled_graphs(gpu, tables, mode):
    from fundsp_amd import graph as GR

    Vj = 70
    sc = build_score(511, voices=Vj)
    rng = np.random.default_rng(512)
    fc = (300.0 * np.exp2(5.0 * rng.random(sc.n))).astype(np.float32)
    seeds = np.arange(Vj, dtype=np.uint64) * 7 + 3

    def bank(g, ex, **kw):
        cutoff = [n for n, _, _ in g.slot_values() if n.endswith(":cutoff")]
        assert len(cutoff) == 1
        b = gpu.Bank.from_graph(g, Vj, sample_rate=SR, **kw)
        b.set_seed(seeds)
        b.set_score(sc.voice, sc.start, sc.end, sc.fin, sc.fout, sc.fade, params={cutoff[0]: fc})
        b.set_option("score_exec", ex)
        return b

    # a hashed graph without rings takes the note path and equals the oracle
    b = bank(GR.noise() >> GR.lowpass_hz(1000.0, 1.0), SCORE_NOTES)
    assert b.get_option("has_score_notes") == 1
    got = voices_of(b.process_events(T, mode=mode))
    assert b.get_option("last_kernel") == LK_SCORE_NOTES
    seq = O.Sequencer(0, 1, SR)
    for k in range(sc.n):
        n = O.noise() >> O.lowpass_hz(float(fc[k]), 1.0)
        n.set_seed(int(seeds[sc.voice[k]]))
        seq.push(sc.start[k], sc.end[k], int(sc.fade[k]), sc.fin[k], sc.fout[k], n)
    _, per = seq.render(T, process=(mode == MODE_PROCESS))
    want = pool_output(sc, per, Vj)
    for v in range(Vj):
        assert_bit_equal(got[v], want[v], f"compiled graph without rings, score voice {v}")
    assert b.events_time() == seq.time()
    # the graph with a ring keeps the voice path and its bits
    ring = GR.noise() >> GR.lowpass_hz(1000.0, 1.0) >> (GR.pass_() & GR.delay(0.002))
    r0, r1 = bank(ring, SCORE_VOICES, ring_frames=128), bank(ring, SCORE_NOTES, ring_frames=128)
    assert r1.get_option("has_score_notes") == 0 and r1.get_option("score_exec") == SCORE_NOTES
    o0, o1 = host(r0.process_events(T, mode=mode)), host(r1.process_events(T, mode=mode))
    assert r1.get_option("last_kernel") == LK_SCORE
    assert_bit_equal(o1, o0, "a graph with a ring under score_exec 1")
    # ... and so does the kind whose adsr_live keeps its gate memory across reset()
    assert W.make_saw_moog_bank(4, SR).get_option("has_score_notes") == 0


def test_every_ahead_of_time_kind_that_qualifies(gpu, tables):
    """4 voices, three notes per voice with rows on the kind's first f32 parameter slot, random inputs, two launches: score_exec 1 equals
    0, samples and state.  A node wrongly declared fresh (state that survives row / update / reset) shows here."""
    import torch

    L = gpu.lib()
    Vk, launches = 4, (64 * 3 + 5, 64 * 2)
    Tk = sum(launches)
    rng = np.random.default_rng(571)
    voice = np.repeat(np.arange(Vk), 3)
    start = (np.tile(np.array([3.0, 90.3, 64 * 3 - 10.0]), Vk) + np.repeat(np.arange(Vk) * 7.0, 3)) / SR
    end = start + np.tile(np.array([70.0, 61.0, 120.0]), Vk) / SR
    fin, fout = np.tile(np.array([0.0, 10.0, 30.0]), Vk) / SR, np.tile(np.array([20.0, 0.0, 50.0]), Vk) / SR
    fade = (np.arange(voice.size) % 2).astype(np.int32)
    took, kept = [], []
    for kind in range(L.fdsp_kind_count()):
        name = L.fdsp_kind_name(kind).decode()
        try:
            probe = gpu.Bank(name, Vk)
        except gpu.FdspError:
            continue                                                 # (kinds that are no plain voice banks)
        if probe.get_option("has_score_notes") != 1:
            kept.append(name)
            continue
        slots = probe.slots()
        fparams = [n for n, k in slots if k == 0 and not n.endswith((".lo", ".hi"))]
        state0 = probe.get_state()
        ni = probe.inputs()
        x = torch.from_numpy((rng.random((max(ni, 1), Tk, Vk), dtype=np.float32) * 2 - 1)).cuda() if ni else None
        params = {}
        if fparams:                                                  # rows near the slot's default: (0.5 .. 1.5) x it, or x 1 where it is 0
            base = float(state0[[n for n, _ in slots].index(fparams[0]), 0])
            params = {fparams[0]: ((base if base != 0.0 else 1.0) * (0.5 + rng.random(voice.size))).astype(np.float32)}
        banks = []
        for ex in (SCORE_VOICES, SCORE_NOTES):
            b = gpu.Bank(name, Vk)
            b.set_sample_rate(SR)
            b.set_seed(np.arange(Vk, dtype=np.uint64) * 11 + 5)
            try:
                b.set_score(voice, start, end, fin, fout, fade, params=params)
            except gpu.FdspError:
                b.set_score(voice, start, end, fin, fout, fade)      # (the first parameter is no f32 slot a score may write)
            b.set_option("score_exec", ex)
            banks.append(b)
        a, b = banks
        t0 = 0
        for n in launches:
            xin = x[:, t0:t0 + n].contiguous() if ni else None
            oa, ob = host(a.process_events(n, xin)), host(b.process_events(n, xin))
            assert a.get_option("last_kernel") == LK_SCORE and b.get_option("last_kernel") == LK_SCORE_NOTES, name
            assert_bit_equal(ob, oa, f"{name}: launch of {n} frames, score_exec 1 vs 0")
            assert_bit_equal(b.get_state(), a.get_state(), f"{name}: voice state after the launch of {n} frames")
            t0 += n
        took.append(name)
    assert "fm_svf" in took and "svf_shape_svf" in took and "saw_moog_adsr_pan" in kept, (took, kept)
    assert len(took) >= 10, took


def test_capture_rule_of_the_mixed_note_path(gpu):
    """A mixed launch under the option inside a stream capture without a prior mix_reserve is refused with the reserve text and leaves the
    bank as it was; after mix_reserve the same launch, uncaptured, allocates nothing"""
    import torch

    want = host(fm_bank().process_events_mix(T))
    b, twin = notes_bank(), notes_bank()
    out = torch.empty((1, T), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with pytest.raises(gpu.FdspError) as e:
            with torch.cuda.graph(g, stream=s):
                b.process_events_mix(T, out=out, stream=s.cuda_stream)
    assert e.value.code == gpu._lib.EINVAL and "fdsp_bank_mix_reserve" in str(e.value)
    torch.cuda.synchronize()
    assert b.events_time() == 0.0 and b.get_option("score_scratch_frames") == 0
    assert_bit_equal(b.get_state(), twin.get_state(), "the refused bank is as it was")
    b.mix_reserve(T)
    frames = b.get_option("score_scratch_frames")
    assert frames >= T
    assert_bit_equal(host(b.process_events_mix(T)), want, "the refused bank mixes correctly afterwards")
    assert b.get_option("score_scratch_frames") == frames, "a reserved bank allocates nothing in the launch"
    # ... and a reserved bank captures
    c = notes_bank()
    c.mix_reserve(T)
    notes_bank().process_events_mix(T)                              # the kernels are loaded outside the capture
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=s):
            c.process_events_mix(T, out=out, stream=s.cuda_stream)
        g2.replay()
    torch.cuda.synchronize()
    assert_bit_equal(host(out), want, "a captured mixed note launch after mix_reserve")


def test_clones_copy_the_option_and_effect_banks_refuse_it(gpu):
    want, clock = fm_oracle(MODE_PROCESS)
    c = notes_bank().clone()
    assert c.get_option("score_exec") == SCORE_NOTES
    got = voices_of(c.process_events(T))
    assert c.get_option("last_kernel") == LK_SCORE_NOTES
    for v in range(V):
        assert_bit_equal(got[v], want[v], f"clone under score_exec 1, voice {v}")
    b = notes_bank()
    b.set_score([], [], [])                                          # dropping the score leaves the option alone
    assert b.get_option("score_exec") == SCORE_NOTES
    L = gpu.lib()
    h = C.c_void_p()
    gpu._lib.check(L.fdsp_reverb_stereo_create(2, 10.0, 1.0, 0.5, C.byref(h)))
    try:
        assert L.fdsp_bank_set_option(h, b"score_exec", 1) == gpu._lib.EINVAL
        assert L.fdsp_bank_get_option(h, b"has_score_notes") == 0
    finally:
        L.fdsp_bank_destroy(h)
