"""The launch policy of the voice kernels (fundsp_amd/csrc/fd_plan.hpp: kernel family, voice groups per workgroup, grid) against its
decision table, on the host: every family renders the same bits, so only this table can see a wrong choice.  The program includes
fd_plan.hpp alone (no HIP) and is built with the host compiler, once plainly and once under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


def build_and_run(tmp_path, name, extra=()):
    exe = tmp_path / name
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "fundsp_amd", "csrc"), "-o", str(exe),
           os.path.join(ROOT, "tests", "host", "check_render_plan.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad 0" in r.stdout
    return r.stdout


def test_render_plan_matches_its_decision_table(tmp_path):
    out = build_and_run(tmp_path, "check_render_plan")
    assert int(out.split()[0]) >= 90   # the table was not emptied


def test_render_plan_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "check_render_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
