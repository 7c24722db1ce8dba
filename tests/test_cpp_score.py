"""Bank::set_score of the C++ host side (include/fundsp_hip.hpp): tests/host/test_cpp_score.cpp holds the checks, this file builds and
runs it -- host mode here, device mode on the GPU box (like tests/test_cpp_host.py)."""
import os
import subprocess

import pytest

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_cpp_score.cpp")
BIN = os.path.join(ROOT, "tests", "host", "_build", "test_cpp_score")


def build():
    O.build()
    lib = os.path.join(ROOT, "fundsp_amd", "libfundsp_hip.so")
    assert os.path.exists(lib), "build the HIP engine first (__graft_entry__.build())"
    deps = [SRC, os.path.join(ROOT, "include", "fundsp_hip.hpp"), os.path.join(ROOT, "include", "fundsp_hip.h"), lib,
            os.path.join(ROOT, "oracle", "libfundsp_oracle.so")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-Wall", "-Wno-parentheses", "-I" + os.path.join(ROOT, "include"),
        "-I" + os.path.join(ROOT, "oracle"), SRC, "-o", BIN,
        "-L" + os.path.join(ROOT, "fundsp_amd"), "-lfundsp_hip", "-L" + os.path.join(ROOT, "oracle"), "-lfundsp_oracle",
        "-L/opt/rocm/lib", "-lamdhip64",
        "-Wl,-rpath," + os.path.join(ROOT, "fundsp_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
        "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return BIN


def run(mode):
    r = subprocess.run([build(), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failure(s)" in r.stdout


def test_cpp_score_argument_checks():
    run("--host")


@pytest.mark.gpu
def test_cpp_score_matches_the_oracle():
    run("--gpu")
