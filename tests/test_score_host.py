"""Scores, host side (no GPU): fundsp_amd.score.assign_voices, the argument checks of fdsp_bank_set_score that need no device, the
symbol in library and header, the shared clock arithmetic walked on the CPU next to the oracle's Sequencer
(tests/host/check_score_blocks.hip), and the premise of the whole feature -- reset() == a fresh unit -- checked on the oracle for the
three graphs tests/test_gpu_score.py plays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
from fundsp_amd.score import assign_voices
from score_cases import SR, V, build_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def overlap_rule_holds(voice, start, end):
    for v in np.unique(voice):
        i = np.flatnonzero(voice == v)
        i = i[np.argsort(start[i], kind="stable")]
        if not np.all(end[i][:-1] <= start[i][1:]):
            return False
    return True


def test_assign_voices_legato_reuses_a_voice():
    v = assign_voices([0.0, 1.0, 2.0, 0.5], [1.0, 2.0, 3.0, 0.7], 2)
    assert v.tolist() == [0, 0, 0, 1] and v.dtype == np.int32


def test_assign_voices_breaks_ties_by_index_and_takes_the_lowest_free_voice():
    assert assign_voices([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 3).tolist() == [0, 1, 2]
    # voice 0 frees up at 1.0, voice 1 at 0.5: the note at 1.0 takes the lowest-numbered free voice, not the one free the longest
    assert assign_voices([0.0, 0.0, 1.0], [1.0, 0.5, 2.0], 2).tolist() == [0, 1, 0]
    # input in any order: notes are taken by start
    assert assign_voices([1.0, 0.0], [2.0, 1.5], 2).tolist() == [1, 0]


def test_assign_voices_names_the_note_that_does_not_fit():
    with pytest.raises(ValueError, match=r"note 2 .* all 2 voices"):
        assign_voices([0.0, 0.1, 0.2, 5.0], [1.0, 1.0, 1.0, 6.0], 2)
    with pytest.raises(ValueError, match=r"note 0 "):
        assign_voices([0.0], [1.0], 0)
    with pytest.raises(ValueError, match=r"note 1 ends before it starts"):
        assign_voices([0.0, 1.0], [1.0, 0.5], 4)


def test_assign_voices_empty():
    v = assign_voices([], [], 4)
    assert v.shape == (0,) and v.dtype == np.int32


def test_assign_voices_always_satisfies_the_overlap_rule():
    rng = np.random.default_rng(7)
    for _ in range(20):
        n = int(rng.integers(1, 300))
        start = np.round(rng.random(n) * 10.0, int(rng.integers(1, 4)))          # many ties and exact legato boundaries
        end = start + np.round(rng.random(n) * 0.5, 2)
        poly = n
        v = assign_voices(start, end, poly)
        assert overlap_rule_holds(v, start, end)
        need = int(v.max()) + 1
        assert assign_voices(start, end, need).tolist() == v.tolist()             # the lowest voices first: no more than it needs
        if need > 1:
            with pytest.raises(ValueError):
                assign_voices(start, end, need - 1)
    sc = build_score(501)                                                          # ... and the test score re-allotted from scratch
    assert overlap_rule_holds(assign_voices(sc.start, sc.end, V), sc.start, sc.end)


@pytest.fixture(scope="module")
def F():
    import fundsp_amd

    fundsp_amd.lib()
    return fundsp_amd


def test_set_score_argument_checks_without_a_device(F):
    L = F.lib()
    voice, ev = (C.c_int * 1)(0), (C.c_double * 4)(0.0, 0.01, 0.0, 0.0)
    assert L.fdsp_bank_set_score(None, 1, voice, ev, None, 0, None, None) == F._lib.EINVAL
    assert b"bank is NULL" in L.fdsp_last_error()
    assert L.fdsp_bank_set_score(None, 0, None, None, None, 0, None, None) == F._lib.EINVAL


def test_library_and_header_agree_on_the_symbol(F):
    header = open(os.path.join(ROOT, "include", "fundsp_hip.h")).read()
    m = re.search(r"int fdsp_bank_set_score\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m and len(m.group(1).split(",")) == 8
    assert hasattr(C.CDLL(F._lib.SO_PATH), "fdsp_bank_set_score")
    res, args = F._lib.SYMBOLS["fdsp_bank_set_score"]
    assert res is C.c_int and len(args) == 8
    shim = open(os.path.join(ROOT, "rust_shim", "src", "lib.rs")).read()
    assert "pub fn fdsp_bank_set_score" in shim and "pub fn set_score" in shim
    assert "void set_score(" in open(os.path.join(ROOT, "include", "fundsp_hip.hpp")).read()


def test_score_kernels_of_run_time_compiled_graphs_build(F):
    """fdsp_graph_check compiles the third module of a run-time compiled graph -- its score kernels -- with hiprtc (no device needed):
    the graph of tests/test_gpu_score.py (a hashed node and a delay ring), and one with three outputs (no fused mix: an empty body)"""
    L = F.lib()
    fm = "Pipe<Pipe<Unop<Pipe<Constant<1>,Sine>,UAddScalar>,Sine>,FixedSvf>"
    for expr in ("Pipe<Pipe<Noise,FixedSvf>,Bus<Pass,Delay>>", f"Stack<Stack<{fm},{fm}>,{fm}>"):
        assert L.fdsp_graph_check(expr.encode()) == 0, (expr, L.fdsp_last_error())


def test_block_windows_and_note_advance_against_the_oracle_sequencer(tmp_path):
    """tests/host/check_score_blocks.hip: fd_seq.hpp's block windows, fade phases and the note-advance rule, walked on the CPU over random
    scores block by block and tick by tick, in one launch and in split launches, against oracle/o_sequencer.c"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    O.build()
    exe = tmp_path / "check_score_blocks"
    cmd = [hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unused-result",
           "-I", os.path.join(ROOT, "fundsp_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"), "-o", str(exe),
           os.path.join(ROOT, "tests", "host", "check_score_blocks.hip"), "-L" + os.path.join(ROOT, "oracle"), "-lfundsp_oracle",
           "-Wl,-rpath," + os.path.join(ROOT, "oracle")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all equal" in r.stdout, r.stdout + r.stderr


# ---- reset() == a fresh unit, on the oracle ------------------------------------------------------------------------------
def _fm(): return O.sine_hz(220.0) * 220.0 * 3.0 + 220.0 >> O.sine() >> O.lowpass_hz(1500.0, 2.0)
def _noise_ring(): return O.noise() >> O.lowpass_hz(900.0, 1.0) >> (O.pass_() & O.delay(0.002))
def _svf_shape_svf(): return O.lowpass_hz(1200.0, 1.5) >> O.shape("tanh", 1.0, 0.0) >> O.highpass_hz(300.0, 0.8)
def _saw_moog():
    return (((O.dc(110.0) >> O.saw()) | O.dc(800.0) | O.dc(0.3)) >> O.moog()) * O.adsr_live(0.005, 0.01, 0.6, 0.01) >> O.pan(0.2)


def _twice_and_fresh(make, nin, process, T=64 * 3 + 21):
    """(first render, render after reset(), a fresh node's render) of the same input"""
    x = None
    if nin:
        x = (np.random.default_rng(5).random((nin, T), dtype=np.float32) * 2 - 1).astype(np.float32)
        x[0, :7] = 0.0                                                             # (a gate: low, then a low -> high edge)
        x[0, 7:150] = np.abs(x[0, 7:150]) + 0.1

    def render(n):
        return n.render_blocks(x, length=T, block=64) if process else n.render_ticks(x, length=T)

    def new():
        n = make()
        n.set_sample_rate(SR)
        n.set_seed(77)
        return n

    used = new()
    first = render(used)
    used.reset()
    return first, render(used), render(new())


@pytest.mark.parametrize("name,make,nin", [("fm_svf", _fm, 0), ("noise_lowpass_bus_delay", _noise_ring, 0), ("svf_shape_svf", _svf_shape_svf, 1)])
@pytest.mark.parametrize("process", [True, False])
def test_reset_equals_a_fresh_unit_on_the_oracle(name, make, nin, process):
    """Render, reset(), render again: the second render must equal a fresh node's, bit for bit -- delay ring, noise sequence, oscillator
    phases and filter state included.  These are the graphs whose notes tests/test_gpu_score.py compares with fresh oracle units; a graph
    that fails this is the wrong graph for that suite."""
    first, again, want = _twice_and_fresh(make, nin, process)
    assert np.array_equal(first.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(again.view(np.uint32), want.view(np.uint32)), f"{name}: reset() does not give back a fresh unit"
    assert np.abs(want).max() > 0.0


def test_adsr_live_keeps_its_gate_memory_across_reset():
    """... and saw_moog_adsr_pan IS such a graph: adsr_live's closure state (attacked, attack_start, release_start: shared variables in the
    reference, adsr.rs:26-56) survives reset() (envelope.rs:293-298 resets the envelope's clock only), so a unit that has played a note
    does not restart like a fresh one.  Its second and later notes on a voice are what the reference's reset() gives, not what a fresh
    unit gives; tests/test_gpu_score.py therefore plays ONE note per voice on that kind and the many-note score on svf_shape_svf."""
    first, again, want = _twice_and_fresh(_saw_moog, 1, True)
    assert np.array_equal(first.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(again.view(np.uint32), want.view(np.uint32))
