"""Host checks of the summing convolver banks (fdsp_convolve_matrix_create): the restatement tests/convolve_matrix_ref.py against float64 and
against the reference's own arithmetic, the single-term case against convolve_ref bit for bit, every split the same bits, single faults
of the order changing bits, and what the host decides before any launch -- the spec's refusals and the graph notation."""
import ctypes as C

import numpy as np
import pytest

import convolve_matrix_ref as MR
import convolve_ref as CR
from test_convolve_ref import CAPACITY, conv64, response

B0 = 64
BIG = 1024                      # the block length above 64 that is measured: the plain bank's largest figure belongs to it
KS = (1, 2, 4, 8)               # terms per output
# (M, max_len): B = 64 on both sides of the partition edges, B = 1024 by 3 taps (P = 1) and B + 1 taps (P = 2) under its largest capacity
RESPONSES = [(3, None), (B0 - 1, None), (B0 + 1, None), (337, None), (3, CAPACITY[BIG]), (BIG + 1, CAPACITY[BIG])]
# four times the largest figure of the table in test_restatement_against_float64, per block length
BOUND = {B0: 4 * 1.64e-7, BIG: 4 * 2.37e-7}
MODEL_CONSTANT = 1.0            # err <= MODEL_CONSTANT * sqrt(K P) * log2(2B) * 2^-24


def bank_inputs(K, M, cap, kind, seed):
    """one output of K terms, each with an input of its own: (x [1, K, T], h [K, M], B, T)"""
    rng = np.random.default_rng(seed)
    h = response(M, seed, (K,))
    B = CR.block_length(cap or M)
    T = M + 3 * B + 11
    if kind == "noise":
        x = rng.uniform(-1.0, 1.0, (1, K, T)).astype(np.float32)
    else:
        x = np.zeros((1, K, T), np.float32)
        x[0, np.arange(K), 5 + np.arange(K)] = 1.0          # one impulse per input, a sample apart
    return x, h, B, T


def sum64(x, h):
    return sum(conv64(x[0, t], h[t]) for t in range(h.shape[0]))


def scale(x, h):
    """sum over the output's terms of sum |h_t|, times max |x|"""
    return np.abs(h).astype(np.float64).sum() * np.abs(x).max()


def measure(K, M, cap, kind, seed, ftz=False):
    """(err of the statement, err of the reference's arithmetic, model, B): max |y - y64| / scale"""
    x, h, B, T = bank_inputs(K, M, cap, kind, seed)
    y64 = sum64(x, h)
    y = MR.render(x, h, range(K), [0] * K, max_len=cap, ftz=ftz)[0, 0]
    # Binop<FrameAdd> over convolvers: the nodes' rounded outputs added by f32 adds, left fold
    each = CR.render(x, h, max_len=cap, ftz=ftz)[0]
    fold = each[0]
    for t in range(1, K):
        fold = fold + each[t]
    P = -(-M // B)
    model = np.sqrt(K * P) * np.log2(2 * B) * 2.0 ** -24
    return np.abs(y - y64).max() / scale(x, h), np.abs(fold - y64).max() / scale(x, h), model, B


@pytest.mark.parametrize("kind", ["noise", "impulse"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,cap", RESPONSES)
def test_restatement_against_float64(M, cap, K, kind):
    """max |y - y64| / (sum over the output's terms of sum |h_t| * max |x|) against the float64 convolution sum, K terms of one output with
    an input each, decaying-noise responses, noise input or one impulse per input.  Measured on the restatement, the largest of seeds
    0 .. 7, statement / the reference's arithmetic (the plain bank's outputs added by f32 adds, left fold), noise input:
        M,    B:   K = 1                 K = 2                 K = 4                 K = 8
        3,   64:   1.40e-07 / 1.40e-07   1.13e-07 / 9.49e-08   8.39e-08 / 5.89e-08   1.08e-07 / 6.38e-08
       63,   64:   1.64e-07 / 1.64e-07   1.31e-07 / 8.21e-08   1.24e-07 / 4.78e-08   1.15e-07 / 3.67e-08
       65,   64:   1.08e-07 / 1.08e-07   1.02e-07 / 6.87e-08   1.23e-07 / 5.02e-08   1.03e-07 / 3.36e-08
      337,   64:   4.52e-08 / 4.52e-08   4.11e-08 / 2.96e-08   4.62e-08 / 2.23e-08   7.03e-08 / 1.70e-08
        3, 1024:   1.95e-07 / 1.95e-07   1.55e-07 / 1.49e-07   1.51e-07 / 9.48e-08   1.25e-07 / 7.75e-08
     1025, 1024:   2.37e-07 / 2.37e-07   1.97e-07 / 1.17e-07   1.69e-07 / 6.51e-08   1.30e-07 / 3.66e-08
    and on the impulses at most 4.67e-08 at either block length, in any column (3 taps, K = 1).  K = 1 is the plain bank.  Relative to its
    scale the statement's error falls slowly as terms are added, the reference's arithmetic falls faster: its K separate sums of M
    products each round less than the statement's one running sum of K M products in the head, while the scale grows like K for both.
    The asserted bound is four times the largest figure of the block length, 6.6e-7 at B = 64 and 9.5e-7 at B = 1024 (the margin covers
    other seeds; the test's own seed is none of the eight), and the reference's arithmetic is held to the same bound.  The model
    sqrt(K P) log2(2B) 2^-24 holds with constant 1; the largest ratio measured is 0.39 (63 taps, K = 1)."""
    err, ref_err, model, B = measure(K, M, cap, kind, seed=100 + M)
    assert B == (BIG if cap else B0)
    print(f"M={M} B={B} K={K} {kind}: statement {err:.3g}, reference's arithmetic {ref_err:.3g}, model {model:.3g}")
    assert err <= BOUND[B], (M, B, K, kind, err)
    assert err <= MODEL_CONSTANT * model, (M, B, K, kind, err, model)
    assert ref_err <= BOUND[B], (M, B, K, kind, ref_err)


def test_flushed_build_inside_the_bound():
    """the flushed arithmetic on inputs none of whose operands is subnormal: the same bound"""
    for M, cap in ((B0 + 1, None), (3, CAPACITY[BIG])):
        err, ref_err, model, B = measure(4, M, cap, "noise", seed=100 + M, ftz=True)
        assert err <= BOUND[B] and err <= model and ref_err <= BOUND[B], (M, B, err, ref_err)


MAPS = [([0, 1], [0, 0]), ([0, 1, 0, 1], [0, 0, 1, 1]), ([0, 0], [0, 0]), ([1, 0, 1, 1], [0, 1, 1, 1]), ([2, 0, 1], [0, 1, 2])]


def inputs_for(tin, tout, M, V=2, seed=0, per=False):
    rng = np.random.default_rng(seed)
    B = CR.block_length(M)
    T = M + 3 * B + 11
    x = rng.uniform(-1.0, 1.0, (V, max(tin) + 1, T)).astype(np.float32)
    return x, response(M, seed, (V, len(tin)) if per else (len(tin),))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("M", [1, 3, B0, B0 + 1, 200])
def test_single_term_outputs_are_the_routed_bank(M):
    """an output of one term has convolve_ref's bits: render(x[:, source], h)"""
    for per in (False, True):
        tin = [2, 0, 1, 0]
        x, h = inputs_for(tin, range(4), M, seed=M, per=per)
        y = MR.render(x, h, tin, range(4))
        assert np.array_equal(bits(y), bits(CR.render(x[:, tin], h))), (M, per)
        # ... also next to an output of three terms
        tin, tout = [1, 0, 1, 2], [0, 1, 1, 1]
        y = MR.render(x, h, tin, tout)
        assert np.array_equal(bits(y[:, 0]), bits(CR.render(x[:, [1]], h[..., :1, :])[:, 0])), (M, per)


@pytest.mark.parametrize("tin,tout", MAPS, ids=["".join(map(str, a)) + "_" + "".join(map(str, b)) for a, b in MAPS])
def test_every_split_gives_the_same_bits(tin, tout):
    M = 200
    x, h = inputs_for(tin, tout, M, V=3, seed=5, per=True)
    T = x.shape[-1]
    one = MR.render(x, h, tin, tout)
    assert one.shape == (3, max(tout) + 1, T)
    for splits in ([1] * T, [1, 63, 64, B0 - 1, B0, B0 + 5, 3 * B0 + 7]):
        assert np.array_equal(bits(one), bits(MR.render(x, h, tin, tout, splits=splits))), splits[:3]
    y = MR.render(x, h, tin, tout, events=[(150, "reset")])
    assert np.array_equal(bits(y[..., 150:]), bits(MR.render(x[..., 150:], h, tin, tout)))
    y = MR.render(x, h, tin, tout, events=[(150, h[..., :50])])
    assert np.array_equal(bits(y[..., 150:]), bits(MR.render(x[..., 150:], h[..., :50], tin, tout, max_len=M)))


def test_split_above_the_head_tile():
    """B = 512, three partitions, pieces off the multiples of 256"""
    B, M = 512, 2 * 512 + 77
    tin, tout = [0, 1, 0, 1], [0, 0, 1, 1]
    splits = [1, 254, 3, 255, 258, B - 1, B + 5, 200]
    T = sum(splits) + 130
    rng = np.random.default_rng(8)
    x = rng.uniform(-1.0, 1.0, (2, 2, T)).astype(np.float32)
    h = response(M, 8, (4,))
    one = MR.render(x, h, tin, tout, max_len=CAPACITY[B])
    assert np.array_equal(bits(one), bits(MR.render(x, h, tin, tout, max_len=CAPACITY[B], splits=splits)))


@pytest.mark.parametrize("order", ["swap", "per_term_sums", "per_term_inverses"])
def test_single_faults_of_the_order_change_bits(order):
    """two terms of an output exchanged, each term's sum added after the loops, each term's inverse added: all inside the float64 bound,
    none the statement's bits -- in the head's samples (the first block, where pend = 0) as far as the fault reaches the head, and after"""
    tin, tout = [0, 1, 0, 1], [0, 0, 1, 1]
    x, h = inputs_for(tin, tout, 200, seed=3)
    want = MR.render(x, h, tin, tout)
    got = MR.render(x, h, tin, tout, order=order)
    head, tail = bits(want[..., :B0]) != bits(got[..., :B0]), bits(want[..., B0:]) != bits(got[..., B0:])
    assert tail.any(), order
    assert head.any() == (order != "per_term_inverses"), "the head has no inverse transform"
    y64 = np.stack([[sum(conv64(x[v, tin[t]], h[t]) for t in range(4) if tout[t] == o) for o in range(2)] for v in range(2)])
    sc = np.array([np.abs(h[:2]).sum(), np.abs(h[2:]).sum()])[None, :, None] * np.abs(x).max()
    assert (np.abs(got - y64) / sc).max() <= BOUND[B0]


def test_swapped_terms_are_another_valid_bank():
    """the swap fault is the bank whose rows and inputs are given in the other order: the order is the tables', nothing hidden"""
    x, h = inputs_for([0, 1], [0, 0], 100, seed=4)
    a = MR.render(x, h, [0, 1], [0, 0], order="swap")
    b = MR.render(x[:, ::-1], h[::-1], [0, 1], [0, 0])
    assert np.array_equal(bits(a), bits(b))


# --- what the host decides before any launch ---------------------------------------------------------------------------------------------
def test_header_library_and_shims_agree_on_the_new_symbols():
    import inspect
    import os
    import re

    import fundsp_amd

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fundsp_amd.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "fundsp_hip.h")).read(), flags=re.S)
    shim = re.sub(r"//[^\n]*", "", open(os.path.join(root, "rust_shim", "src", "lib.rs")).read())
    hpp = open(os.path.join(root, "include", "fundsp_hip.hpp")).read()
    raw = C.CDLL(fundsp_amd._lib.SO_PATH)
    for name, nargs in (("fdsp_convolve_matrix_create", 7), ("fdsp_convolve_matrix_create_on", 8)):
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == nargs, f"{name}: not declared with {nargs} parameters in include/fundsp_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert len(fundsp_amd._lib.SYMBOLS[name][1]) == nargs, f"{name}: ctypes signature"
    r = re.search(r"pub fn fdsp_convolve_matrix_create_on\s*\(([^)]*)\)", shim, flags=re.S)   # (the shim binds the `_on` constructors)
    assert r and len([a for a in r.group(1).split(",") if a.strip()]) == 8, "fdsp_convolve_matrix_create_on: rust_shim"
    assert "fdsp_convolve_matrix_create(" in hpp and "static Bank convolve_matrix(" in hpp, "include/fundsp_hip.hpp"
    assert "pub fn convolve_matrix" in shim, "HipBank lacks `convolve_matrix`"
    assert {"source", "target"} <= set(inspect.signature(fundsp_amd.Bank.convolve).parameters)
    assert [f[0] for f in fundsp_amd._lib.ConvolveSpec._fields_] == ["channels", "max_len", "len", "per_instance", "flush_denormals", "response"]


def test_invalid_specs_are_refused_before_any_device_work():
    import fundsp_amd as F
    from fundsp_amd import _lib

    L = F.lib()
    h = np.ones((16, 16), np.float32)
    fp = h.ctypes.data_as(C.POINTER(C.c_float))

    def create(V=3, channels=2, inputs=2, outputs=1, tin=(0, 1), tout=(0, 0), **kw):
        s = _lib.ConvolveSpec()
        s.channels, s.max_len, s.len = channels, kw.get("max_len", 16), kw.get("len", 16)
        s.per_instance, s.flush_denormals = kw.get("per_instance", 0), kw.get("flush_denormals", 0)
        s.response = kw.get("response", fp)
        out = C.c_void_p(1)
        ti = None if tin is None else (C.c_int * len(tin))(*tin)
        to = None if tout is None else (C.c_int * len(tout))(*tout)
        rc = L.fdsp_convolve_matrix_create(V, C.byref(s), inputs, outputs, ti, to, C.byref(out))
        return rc, L.fdsp_last_error(), out.value

    cases = ((dict(channels=0, tin=(), tout=()), b"channels"), (dict(channels=17, tin=(0,) * 17, tout=(0,) * 17), b"channels"),
             (dict(inputs=0), b"inputs"), (dict(inputs=9), b"inputs"), (dict(outputs=0), b"outputs"), (dict(outputs=9), b"outputs"),
             (dict(tin=None), b"term_input NULL"), (dict(tout=None), b"term_output NULL"),
             (dict(tin=(0, 2)), b"term_input[1] = 2"), (dict(tin=(-1, 1)), b"term_input[0] = -1"),
             (dict(tout=(0, 1)), b"term_output[1] = 1"), (dict(tout=(-1, 0)), b"term_output[0] = -1"),
             (dict(outputs=2, tout=(1, 0)), b"non-decreasing"), (dict(outputs=2, tout=(1, 1)), b"output 0"), (dict(outputs=2, tout=(0, 0)), b"output 1"),
             (dict(tin=(1, 1)), b"input 0"), (dict(inputs=3, channels=3, tin=(0, 1, 1), tout=(0, 0, 0)), b"input 2"),
             (dict(V=0), b"instances"), (dict(max_len=0), b"max_len"), (dict(len=17), b"len = 17"), (dict(per_instance=2), b"per_instance"),
             (dict(flush_denormals=-1), b"flush_denormals"), (dict(response=None), b"response NULL"))
    for kw, msg in cases:
        rc, err, out = create(**kw)
        assert rc == _lib.EINVAL and not out, kw
        assert msg in err and err.startswith(b"fdsp_convolve_matrix_create: "), (kw, err)
    assert L.fdsp_convolve_matrix_create(3, None, 1, 1, None, None, C.byref(C.c_void_p())) == _lib.EINVAL
    s = _lib.ConvolveSpec()
    s.channels, s.max_len, s.len, s.response = 2, 16, 16, fp
    two = (C.c_int * 2)(0, 1), (C.c_int * 2)(0, 0)
    assert L.fdsp_convolve_matrix_create(3, C.byref(s), 2, 1, two[0], two[1], None) == _lib.EINVAL
    assert L.fdsp_last_error() == b"fdsp_convolve_matrix_create: out is NULL"
    with pytest.raises(ValueError, match="one output index per term"):
        F.Bank.convolve(2, h[:2], source=[0, 1], target=[0])
    with pytest.raises(ValueError, match="needs source"):
        F.Bank.convolve(2, h[:2], target=[0, 0])


def test_graph_notation_plans_the_matrix():
    from fundsp_amd import Bank
    from fundsp_amd import graph as G

    w = np.arange(12, dtype=np.float32).reshape(4, 3) + 1
    ll, lr, rl, rr = (G.convolve(w, c) for c in range(4))
    g = (ll + rl) ^ (lr + rr)
    assert (g.nin, g.nout) == (2, 2)
    h, tin, tout, I, O = G.convolve_matrix_plan(g)
    assert (tin, tout, I, O) == ([0, 1, 0, 1], [0, 0, 1, 1], 2, 2) and np.array_equal(h, w[[0, 2, 1, 3]])
    # a leaf, a stack, a branch: one term per output, the routed plan's tables
    assert G.convolve_matrix_plan(ll)[1:] == ([0], [0], 1, 1)
    h, tin, tout, I, O = G.convolve_matrix_plan((ll ^ lr) | rr)
    assert (tin, tout, I, O) == ([0, 0, 1], [0, 1, 2], 2, 3) and (tin, I) == tuple(G.convolve_route_plan((ll ^ lr) | rr)[1:])
    # `+` of stacks adds output by output, and the terms are stably ordered by output; the association is flattened to term order
    short = G.convolve([5.0, 6.0])
    h, tin, tout, I, O = G.convolve_matrix_plan((ll | lr) + (rl | short))
    assert (tin, tout, I, O) == ([0, 2, 1, 3], [0, 0, 1, 1], 4, 2)
    assert np.array_equal(h, np.array([w[0], w[2], w[1], [5, 6, 0]], np.float32)), "shorter responses are zero-padded"
    a = G.convolve_matrix_plan((ll + lr) + rl)
    b = G.convolve_matrix_plan(ll + (lr + rl))
    assert a[1:] == b[1:] == ([0, 1, 2], [0, 0, 0], 3, 1) and np.array_equal(a[0], b[0])
    h, tin, tout, I, O = G.convolve_matrix_plan((ll ^ lr) + (rl ^ rr))    # 2 inputs: each side has one
    assert (tin, tout, I, O) == ([0, 1, 0, 1], [0, 0, 1, 1], 2, 2) and np.array_equal(h, w[[0, 2, 1, 3]])
    # anything else is no plan
    for bad in (ll + G.pass_(), G.noise() >> ll, ll & lr, ll * lr, ll - lr, ll + 1.0, ll >> lr):
        assert G.convolve_matrix_plan(bad) is None
    # the limits, named
    sum6 = ll + ll + ll + ll + ll + ll                       # 6 inputs, 6 terms, 1 output
    assert G.convolve_matrix_plan(sum6 ^ sum6)[1:] == ([0, 1, 2, 3, 4, 5] * 2, [0] * 6 + [1] * 6, 6, 2)
    with pytest.raises(ValueError, match="16 terms"):
        G.convolve_matrix_plan(sum6 ^ sum6 ^ sum6)           # 6 inputs, 18 terms, 3 outputs
    with pytest.raises(ValueError, match="8 inputs"):
        G.convolve_matrix_plan(sum6 + ll + ll + ll)          # 9 inputs, 9 terms, 1 output
    branch9 = ll
    for _ in range(8):
        branch9 = branch9 ^ ll                               # 1 input, 9 terms, 9 outputs
    with pytest.raises(ValueError, match="8 outputs"):
        G.convolve_matrix_plan(branch9)
    # from_graph and the older plans answer as before
    assert G.convolve_plan(g) is None and G.convolve_route_plan(g) is None and G.convolve_route_plan(ll + rl) is None
    with pytest.raises(ValueError, match="front >> convolve"):
        Bank.from_graph(g, 2)
    assert g.type == "Branch<Binop<OpAdd,ConvolvePing,ConvolvePing>,Binop<OpAdd,ConvolvePing,ConvolvePing>>"
