"""One launch plan for compiled and run-time graphs (fundsp_amd/csrc/fd_plan.hpp): the FM voice of BASELINE config 3 as its
ahead-of-time kind and as the same graph compiled at run time, launch for launch on the edges of the plan's conditions.  Both banks
must report the same kernel family, the family must be the one the host decision table (tests/host/check_render_plan.cpp) gives for
the row -- kept here as literals: 1 single wave, 2 stage pipeline, 3 planar pipeline, 4 time split --, and the outputs must be bit-equal."""
import pytest
import torch

from fundsp_amd import LAYOUT_PLANAR, LAYOUT_VOICE_MINOR
from fundsp_amd import graph as GR
from fundsp_amd import workloads as W

pytestmark = pytest.mark.gpu
SR = 48000.0
SINGLE, PIPE, PLANAR, SPLIT = 1, 2, 3, 4


def bank_pair(gpu, V):
    p = W.fm_svf_params(V, SR)
    g = GR.sine_hz(p["f"]) * p["f"] * p["m"] + p["f"] >> GR.sine() >> GR.lowpass_hz(p["fc"], p["q"])
    jit = gpu.Bank.from_graph(g, V, sample_rate=SR)
    jit.set_seed(p["seed"])
    return W.make_fm_svf_bank(V, SR, params=p), jit


def launch_both(banks, T, what, want, **kw):
    """the same launch on both banks (their states advance together): families as `want`, outputs bit-equal"""
    outs = [b.process(T, **kw) for b in banks]
    torch.cuda.synchronize()
    got = [b.get_option("last_kernel") for b in banks]
    print(f"{what}: last_kernel ahead-of-time {got[0]}, run-time {got[1]}, table {want}")
    assert got[0] == got[1], f"{what}: ahead-of-time kind took family {got[0]}, run-time compiled graph {got[1]}"
    assert got[0] == want, f"{what}: family {got[0]}, the decision table says {want}"
    T_ = slice(0, T)
    a, b = (o[..., T_] if kw.get("layout") == LAYOUT_PLANAR else o for o in outs)
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f"{what}: outputs differ"


def test_small_bank_edges_take_the_same_family(gpu):
    """Rows A: voice groups = cus, cus + 1 voice, 2 cus, 2 cus + 1 voice; T one frame short of a block, one block, two; time split on and off."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # time_split 1: the time-split kernels up to two voice groups per CU on whole blocks; else the pipeline from one block on (PipeMinT = 64)
    table = {
        ("cus", 1): {63: SINGLE, 64: SPLIT, 128: SPLIT}, ("cus+1", 1): {63: SINGLE, 64: SPLIT, 128: SPLIT},
        ("2cus", 1): {63: SINGLE, 64: SPLIT, 128: SPLIT}, ("2cus+1", 1): {63: SINGLE, 64: PIPE, 128: PIPE},
        ("cus", 0): {63: SINGLE, 64: PIPE, 128: PIPE}, ("cus+1", 0): {63: SINGLE, 64: PIPE, 128: PIPE},
        ("2cus", 0): {63: SINGLE, 64: PIPE, 128: PIPE}, ("2cus+1", 0): {63: SINGLE, 64: PIPE, 128: PIPE},
    }
    for name, V in (("cus", 64 * cus), ("cus+1", 64 * cus + 1), ("2cus", 128 * cus), ("2cus+1", 128 * cus + 1)):
        banks = bank_pair(gpu, V)
        for split in (1, 0):
            for b in banks:
                b.set_option("time_split", split)
            for T in (63, 64, 128):
                launch_both(banks, T, f"V = {name} ({V}), T = {T}, time_split {split}", table[(name, split)][T], layout=LAYOUT_VOICE_MINOR)


@pytest.fixture(scope="module")
def pair200(gpu):
    return bank_pair(gpu, 200)


# Rows B, 200 voices.  "pipe_split" 0: never the pipeline; 1: a small bank, one whole block -> time split; 2 / 3: the pipeline, forced;
# 4 asks for the loader-wave-only plan, which a graph without inputs does not have (stage counts of the FM voice for "pipe_split"
# 1 / 4 / 2 / 3: 2 / 0 / 2 / 3) -> the single wave (the rows "fm as built" / "fm_rt as built" of tests/host/check_render_plan.cpp)
@pytest.mark.parametrize("split,want", [(0, SINGLE), (1, SPLIT), (2, PIPE), (3, PIPE), (4, SINGLE)])
def test_every_pipe_split_takes_the_same_family(pair200, split, want):
    for b in pair200:
        b.set_option("pipe_split", split)
    launch_both(pair200, 64, f"pipe_split {split}", want, layout=LAYOUT_VOICE_MINOR)


# ... and the planar pipeline's conditions: 16 frames, rows of 16-byte runs
@pytest.mark.parametrize("T,stride,want", [(15, 16, SINGLE), (16, 16, PLANAR), (16, 18, SINGLE)])
def test_planar_rows_take_the_same_family(pair200, T, stride, want):
    for b in pair200:
        b.set_option("pipe_split", 1)
    launch_both(pair200, T, f"planar T = {T}, frame_stride {stride}", want, layout=LAYOUT_PLANAR, frame_stride=stride)
