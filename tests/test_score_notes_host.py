"""Scores with one lane per note, host side (no GPU): the two executors restated on the CPU over a real node type and compared sample by
sample and slot by slot (tests/host/check_score_notes.hip), the options and constants in library, header and package, and the third
module of run-time compiled graphs with the note kernels' entry points."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def F():
    import fundsp_amd

    fundsp_amd.lib()
    return fundsp_amd


def test_note_walk_equals_voice_walk_on_the_cpu(tmp_path):
    """tests/host/check_score_notes.hip: random scores (legato pairs, several notes in a block, zero-length notes -- one directly behind
    the last rendered note of a voice --, notes carried across a split, off-grid times) rendered the way render_score_body walks a voice and
    the way render_score_notes_body walks a note, the shared predicate of fd_seq.hpp deciding the write-back: one launch and split
    launches, process and tick, every sample and every voice's final slot image bit-equal.  It also pins the clock trap: the multiplied
    block clock differs from the accumulated one."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "check_score_notes"
    cmd = [hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unused-result",
           "-I", os.path.join(ROOT, "fundsp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "check_score_notes.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all equal" in r.stdout, r.stdout + r.stderr
    m = re.search(r"(\d+) of 1500 differ", r.stdout)
    assert m and int(m.group(1)) > 0, r.stdout


def test_options_without_a_device(F):
    """What the library answers before it touches a device: the process-wide chunk option checks its range; the per-bank options need a bank"""
    L = F.lib()
    try:
        assert L.fdsp_set_option(b"score_chunk_frames", 128) == 0
        assert L.fdsp_set_option(b"score_chunk_frames", 100) == F._lib.EINVAL
        assert b"multiple of 64" in L.fdsp_last_error()
        assert L.fdsp_set_option(b"score_chunk_frames", -64) == F._lib.EINVAL
    finally:
        assert L.fdsp_set_option(b"score_chunk_frames", 0) == 0
    assert L.fdsp_bank_set_option(None, b"score_exec", 1) == F._lib.EINVAL
    assert L.fdsp_bank_get_option(None, b"has_score_notes") == F._lib.EINVAL
    assert L.fdsp_set_option(b"score_exec", 1) == F._lib.EINVAL       # a property of a bank, not of the process


def test_header_library_and_package_agree_on_the_constants(F):
    header = open(os.path.join(ROOT, "include", "fundsp_hip.h")).read()
    defs = dict(re.findall(r"#define (FDSP_SCORE_\w+) (\d+)", header))
    assert defs == {"FDSP_SCORE_VOICES": "0", "FDSP_SCORE_NOTES": "1"}
    assert (F.SCORE_VOICES, F.SCORE_NOTES) == (0, 1)
    for name in ('"score_exec"', '"has_score_notes"', '"score_chunk_frames"', '"score_scratch_frames"'):
        assert name in header, name
    assert re.search(r"10 a score rendered with one lane per note", header)
    opts = open(os.path.join(ROOT, "fundsp_amd", "csrc", "fd_opts.hpp")).read()
    assert re.search(r"LK_SCORE = 9, LK_SCORE_NOTES = 10\b", opts)
    so = open(F._lib.SO_PATH, "rb").read()
    for name in (b"score_exec", b"has_score_notes", b"score_chunk_frames"):
        assert name in so, name
    assert "score_exec" in F.Bank.set_score.__doc__


def test_score_module_of_run_time_compiled_graphs_builds_with_the_note_kernels(F):
    """fdsp_graph_check compiles the third module with hiprtc (no device needed); it now carries jit_score_notes_<mode> next to
    jit_score_<mode> and jit_score_mix_<mode>: a hashed graph without rings (a real body), the graph with a delay ring (an empty body),
    a gated graph with adsr_live, and three outputs"""
    L = F.lib()
    assert b"jit_score_notes_" in open(F._lib.SO_PATH, "rb").read()
    fm = "Pipe<Pipe<Unop<Pipe<Constant<1>,Sine>,UAddScalar>,Sine>,FixedSvf>"
    for expr in ("Pipe<Noise,FixedSvf>", "Pipe<Pipe<Noise,FixedSvf>,Bus<Pass,Delay>>", "Binop<OpMul,Pipe<Noise,FixedSvf>,AdsrLive>", f"Stack<Stack<{fm},{fm}>,{fm}>"):
        assert L.fdsp_graph_check(expr.encode()) == 0, (expr, L.fdsp_last_error())
