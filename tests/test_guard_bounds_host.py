"""Host-side check of the guards that the packed sine and SVF paths decide per block / per item from a producer's output bound
(fd_nodes.hpp: OutBound, SineB, FixedSvfB / FixedSvfLpB, HoistOf): FmSvf and SineHzLowpass driven the way the pipeline's stage
loop drives them, bit for bit against the plain step() rendering and the oracle -- phase sweeps around the 2047-turn threshold,
bounds that trip although the phase stays in the domain, initial phases 3000 / -0.0 / 0.0, negative f and m, filter states
around 2^96 and up to 2^127, inf, NaN, ic2eq = -0.0, cutoffs above Nyquist with q = 1e-30 / 1e30 -- and the proof that the
bounded forms really ran unguarded (no tile of an ordinary voice trips; tmax is never raised).  Built with hipcc for the host."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import oracle as O
    O.lib()   # make sure oracle/libfundsp_oracle.so is built
    out = tmp_path_factory.mktemp("guard_bounds") / "check_guard_bounds"
    odir = os.path.join(ROOT, "oracle")
    cmd = [hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unused-result",
           "-I", os.path.join(ROOT, "fundsp_amd", "csrc"), "-I", odir, "-o", str(out),
           os.path.join(ROOT, "tests", "host", "check_guard_bounds.hip"), "-L" + odir, "-lfundsp_oracle", "-Wl,-rpath," + odir]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return str(out)


def test_bounded_guards_match_plain_rendering_and_oracle(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad 0" in r.stdout and "vacuous 0" in r.stdout and "audio trips 0" in r.stdout, r.stdout


def test_python_edge_rows_are_the_host_check_rows(exe):
    """tests/test_gpu_guard_bounds.py renders the rows of tests/guard_bound_rows.py: they are the host check's, bit for bit."""
    from guard_bound_rows import edge_rows, row_bits
    r = subprocess.run([exe, "--rows"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    host = []
    for line in r.stdout.split("\n"):
        w = line.split()
        if len(w) == 9:
            bits = tuple("nan" if (int(x, 16) & 0x7fffffff) > 0x7f800000 else x for x in w[:8])
            host.append(bits + (int(w[8]),))
    mine = [row_bits(x) for x in edge_rows()]
    assert mine == host
