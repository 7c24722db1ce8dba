"""The packed sine and SVF guards decided per block / per item from the producer's output bound (fd_nodes.hpp: SineB, FixedSvfB,
HoistOf) on the device: banks of 128 and 100 FM voices (two voice groups, one ragged) whose voices carry the edge rows of the host
check -- phase sweeps around the 2047-turn threshold, initial phases 3000 / -0.0, negative f and m, filter states around 2^96 up to
2^127, inf, NaN, ic2eq = -0.0, cutoffs above Nyquist with q = 1e-30 / 1e30 -- rendered through every kernel family the headline graph
can take (single wave, stage pipeline at pipe_split 1 and 2, three-way time split, fused mix-down, a run-time compiled graph), T = 200
(three blocks and an 8-frame remainder) and T = 192 (whole blocks: small banks take the time split).  Every comparison is bit for bit
(NaN == NaN) against the CPU oracle: the oracle's oscillators, and the reference SVF tick (svf.rs:995-1006) on their output -- in numpy,
because the oracle's filter cannot be given a preset state; where the filter starts from rest the two are checked against each other."""
import numpy as np
import pytest

import oracle as O
from fundsp_amd import LAYOUT_VOICE_MINOR, MIX_PAN, MODE_PROCESS
from fundsp_amd import workloads as W
from guard_bound_rows import edge_rows
from svf_par_ref import tick
from test_gpu_parity import assert_bit_equal, run_bank

pytestmark = pytest.mark.gpu
SR = 48000.0
F = np.float32
ROWS = edge_rows()
_REF = {}


def voice_rows(V):
    return [ROWS[v % len(ROWS)] for v in range(V)]


def reference_rows(lengths):
    """[row][sum(lengths)]: consecutive launches of `lengths` frames, each cut into 64-frame blocks from its own first frame."""
    key = tuple(lengths)
    if key in _REF:
        return _REF[key]
    n, total = len(ROWS), sum(lengths)
    x = np.zeros((n, total), dtype=F)
    full = np.zeros((n, total), dtype=F)
    for k, (f, m, fc, q, pm, pc, ic1, ic2, preset) in enumerate(ROWS):
        def osc():
            return (O.constant(float(f)) >> O.sine().phase(float(pm))) * float(f) * float(m) + float(f) >> O.sine().phase(float(pc))
        a, b = osc(), osc() >> O.lowpass_hz(float(fc), float(q))
        a.set_sample_rate(SR)
        b.set_sample_rate(SR)
        x[k] = np.concatenate([a.render_blocks(None, length=L, block=64)[0] for L in lengths])
        full[k] = np.concatenate([b.render_blocks(None, length=L, block=64)[0] for L in lengths])
    co = np.stack([O.svf_coefs("lowpass", SR, float(r[2]), float(r[3])) for r in ROWS]).astype(F)   # a1 a2 a3 m0 m1 m2
    a1, a2, a3, m0, m1, m2 = (co[:, j].copy() for j in range(6))
    ic1 = np.array([r[6] for r in ROWS], dtype=F)
    ic2 = np.array([r[7] for r in ROWS], dtype=F)
    y = np.zeros_like(x)
    two = F(2.0)
    with np.errstate(all="ignore"):
        for t in range(total):  # SvfCore::tick, the reference's operations in the reference's order, all rows at once
            y[:, t], ic1, ic2 = tick((a1, a2, a3, m0, m1, m2), ic1, ic2, x[:, t], two)
    rest = np.array([not r[8] for r in ROWS])
    assert_bit_equal(y[rest], full[rest], "the numpy SVF tick equals the oracle's filter where it starts from rest")
    _REF[key] = y
    return y


def reference(V, lengths):
    return reference_rows(lengths)[np.arange(V) % len(ROWS)]


def preset(b, rows):
    """Phases and filter state through set_state (slot order of the bank: the first phase is the modulator's)."""
    names = [n for n, _ in b.slots()]
    ph = [i for i, n in enumerate(names) if n.endswith(":phase")]
    i1 = [i for i, n in enumerate(names) if n.endswith(":ic1eq")]
    i2 = [i for i, n in enumerate(names) if n.endswith(":ic2eq")]
    assert len(ph) == 2 and len(i1) == 1 and len(i2) == 1, names
    st = b.get_state()
    st[ph[0]] = np.array([r[4] for r in rows], dtype=F)
    st[ph[1]] = np.array([r[5] for r in rows], dtype=F)
    st[i1[0]] = np.array([r[6] for r in rows], dtype=F)
    st[i2[0]] = np.array([r[7] for r in rows], dtype=F)
    b.set_state(st)
    return b


def params_of(rows):
    col = lambda j: np.array([r[j] for r in rows], dtype=F)
    return dict(f=col(0), m=col(1), fc=col(2), q=col(3), seed=np.arange(len(rows), dtype=np.uint64))


def make_bank(rows, **opts):
    b = W.make_fm_svf_bank(len(rows), SR, params=params_of(rows))
    for k, v in opts.items():
        b.set_option(k, v)
    return preset(b, rows)


FAMILIES = [("single wave", dict(pipe_split=0), 1),
            ("pipeline, pipe_split 1", dict(time_split=0, pipe_split=1), None),
            ("pipeline, pipe_split 2", dict(time_split=0, pipe_split=2), 2),
            ("time split", dict(time_split=1), None)]   # (T = 192: the three-way time split; T = 200: falls back to the pipeline)


@pytest.mark.parametrize("V", [128, 100])
@pytest.mark.parametrize("T", [200, 192])
def test_every_family_renders_the_edge_rows_like_the_oracle(gpu, V, T):
    rows = voice_rows(V)
    want = reference(V, [T])
    for name, opts, family in FAMILIES:
        b = make_bank(rows, **opts)
        with np.errstate(all="ignore"):
            got = run_bank(b, None, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)[:, 0, :]
        k = b.get_option("last_kernel")
        if family is not None:
            assert k == family, (name, k)
        if name == "time split":
            assert k == (4 if T % 64 == 0 else 2), (name, T, k)
        assert_bit_equal(got, want, f"{name} (family {k}), V = {V}, T = {T}")


@pytest.mark.parametrize("V", [128, 100])
def test_two_launches_continue_the_state(gpu, V):
    """100 + 100 frames (64 + 32 + a 4-frame remainder each) into one voice-out history, against the oracle rendered with the SAME two
    launches.  Not against one launch of 200 frames: process semantics cut every launch into 64-frame blocks from its own first frame, so
    100 + 100 is blocks of 64 | 32 + 4 remainder | 64 | 32 + 4 where 200 is 64 | 64 | 64 | 8, and remainder frames take the tick arithmetic
    (sinf, wrapped phase) -- the samples differ by design.  The last line asserts exactly that, so that a reference which ignored the
    partition would be noticed."""
    rows = voice_rows(V)
    want = reference(V, [100, 100])
    for opts in (dict(time_split=0), dict(pipe_split=0)):
        b = make_bank(rows, **opts)
        with np.errstate(all="ignore"):
            got = np.concatenate([run_bank(b, None, 100, LAYOUT_VOICE_MINOR, MODE_PROCESS)[:, 0, :] for _ in range(2)], axis=1)
        assert_bit_equal(got, want, f"100 + 100 frames, {opts}")
    assert not np.array_equal(want.view(np.uint32), reference(V, [200]).view(np.uint32))  # (another block partition: other samples)


@pytest.mark.parametrize("V", [128, 100])
@pytest.mark.parametrize("T", [200, 192])
def test_fused_mix_down_equals_the_unfused_pair(gpu, V, T):
    """process_mix(MIX_PAN) against voice-out + mix_stereo, on the rows whose samples stay finite (a NaN voice would make the whole
    mix NaN and the comparison empty)."""
    import torch

    ref = reference_rows([T])
    with np.errstate(all="ignore"):
        ok = [k for k in range(len(ROWS)) if np.isfinite(ref[k]).all() and np.abs(ref[k]).max() < 1.0e6]
    assert len(ok) > 40
    rows = [ROWS[ok[v % len(ok)]] for v in range(V)]
    pan = np.linspace(-1, 1, V).astype(F)
    for opts in (dict(), dict(time_split=0)):
        vo = run_bank(make_bank(rows, **opts), None, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)[:, 0, :]
        assert_bit_equal(vo, ref[[ok[v % len(ok)] for v in range(V)]], f"voice-out of the mix rows, {opts}")
        bm = make_bank(rows, **opts)
        bm.set_pan(pan)
        mix = bm.process_mix(T, mix=MIX_PAN)
        torch.cuda.synchronize()
        assert bm.get_option("last_kernel") == (4 if (T % 64 == 0 and not opts) else 2)
        unfused = gpu.mix_stereo(torch.from_numpy(np.ascontiguousarray(vo.T)).cuda(), torch.from_numpy(pan).cuda()).cpu().numpy()
        assert np.isfinite(unfused).all() and np.abs(unfused).max() > 0.1
        assert_bit_equal(mix.cpu().numpy(), unfused, f"fused mix-down vs mix_stereo(voice-out), V = {V}, T = {T}, {opts}")


def test_run_time_compiled_graph_of_the_same_shape(gpu):
    from fundsp_amd import graph as GR

    V = 100
    rows = voice_rows(V)
    p = params_of(rows)
    g = GR.sine_hz(p["f"]) * p["f"] * p["m"] + p["f"] >> GR.sine() >> GR.lowpass_hz(p["fc"], p["q"])
    for T, opts in ((200, dict(time_split=0)), (192, dict(time_split=1)), (200, dict(pipe_split=0))):
        b = gpu.Bank.from_graph(g, V, sample_rate=SR)
        b.set_seed(p["seed"])
        for k, v in opts.items():
            b.set_option(k, v)
        preset(b, rows)
        with np.errstate(all="ignore"):
            got = run_bank(b, None, T, LAYOUT_VOICE_MINOR, MODE_PROCESS)[:, 0, :]
        assert_bit_equal(got, reference(V, [T]), f"run-time compiled FM voice, T = {T}, {opts} (family {b.get_option('last_kernel')})")
