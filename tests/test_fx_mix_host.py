"""Host-side checks of the effect banks' fused mix-down (no GPU needed): the planar entry point is exported, declared, bound by the Python
table and the Rust shim with one parameter list, refuses a NULL bank; Chain has the mix methods; the chunk option takes multiples of 64."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fdsp_bank_process_mix_planar"


@pytest.fixture(scope="module")
def F():
    import fundsp_amd

    fundsp_amd.lib()
    return fundsp_amd


def test_planar_mix_entry_is_exported_declared_and_bound(F):
    assert hasattr(C.CDLL(F._lib.SO_PATH), NAME), f"{NAME} is not exported by the built library"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fundsp_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{NAME} is not declared in include/fundsp_hip.h"
    n_c = len([a for a in m.group(1).split(",") if a.strip()])
    shim = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust_shim", "src", "lib.rs")).read())
    r = re.search(r"pub fn " + NAME + r"\s*\(([^)]*)\)", shim, flags=re.S)
    assert r, f"{NAME} is not bound by rust_shim"
    assert len([a for a in r.group(1).split(",") if a.strip()]) == n_c == 8
    assert "pub fn render_mix_planar" in shim
    assert NAME in F._lib.SYMBOLS and len(F._lib.SYMBOLS[NAME][1]) == n_c
    assert "process_mix_planar" in open(os.path.join(ROOT, "include", "fundsp_hip.hpp")).read()


def test_planar_mix_entry_refuses_a_null_bank(F):
    L = F.lib()
    assert L.fdsp_bank_process_mix_planar(None, 64, None, 64, None, F.MIX_SUM, F.MODE_PROCESS, None) == F._lib.EINVAL
    assert b"NULL" in L.fdsp_last_error()


def test_chain_has_the_mix_methods(F):
    for m in ("process_mix", "set_pan", "mix_reserve"):
        assert callable(getattr(F.Chain, m, None)), f"Chain lacks {m}"


def test_chunk_option_takes_multiples_of_64(F):
    """one table checks fdsp_set_option and fdsp_bank_set_option (a bank needs a device: tests/test_gpu_fx_mix.py asks the bank's setter)"""
    L = F.lib()
    try:
        for bad in (100, 63, -64):
            assert L.fdsp_set_option(b"fx_mix_chunk_frames", bad) == F._lib.EINVAL, bad
            assert b"multiple of 64" in L.fdsp_last_error()
        assert L.fdsp_set_option(b"fx_mix_chunk_frames", 128) == 0
    finally:
        assert L.fdsp_set_option(b"fx_mix_chunk_frames", 0) == 0
