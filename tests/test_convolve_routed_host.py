"""Host-side checks of the routed convolver banks (no GPU): the two new C ABI symbols in the header, the library, the ctypes table, the C++
wrapper and the Rust shim; every invalid routing refused before a device is touched; graph.convolve_route_plan on trees of stacks and
branches over convolve(..) leaves."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fdsp_convolve_routed_create": 5, "fdsp_convolve_routed_create_on": 6}


def test_header_library_and_shims_agree_on_the_new_symbols():
    import fundsp_amd

    fundsp_amd.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fundsp_hip.h")).read(), flags=re.S)
    shim = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust_shim", "src", "lib.rs")).read())
    hpp = open(os.path.join(ROOT, "include", "fundsp_hip.hpp")).read()
    raw = C.CDLL(fundsp_amd._lib.SO_PATH)
    for name, nargs in NEW.items():
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == nargs, f"{name}: not declared with {nargs} parameters in include/fundsp_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert len(fundsp_amd._lib.SYMBOLS[name][1]) == nargs, f"{name}: ctypes signature"
    r = re.search(r"pub fn fdsp_convolve_routed_create_on\s*\(([^)]*)\)", shim, flags=re.S)   # (the shim binds the `_on` constructors)
    assert r and len([a for a in r.group(1).split(",") if a.strip()]) == 6, "fdsp_convolve_routed_create_on: rust_shim"
    assert "fdsp_convolve_routed_create(" in hpp and "static Bank convolve_routed(" in hpp, "include/fundsp_hip.hpp"
    assert "pub fn convolve_routed" in shim, "HipBank lacks `convolve_routed`"
    assert "source" in inspect.signature(fundsp_amd.Bank.convolve).parameters
    # the spec itself is unchanged: callers compiled against it stay valid
    assert [f[0] for f in fundsp_amd._lib.ConvolveSpec._fields_] == ["channels", "max_len", "len", "per_instance", "flush_denormals", "response"]


def spec_of(channels, n=16):
    from fundsp_amd import _lib

    h = np.ones(channels * n, np.float32)
    s = _lib.ConvolveSpec()
    s.channels, s.max_len, s.len, s.per_instance, s.flush_denormals = channels, n, n, 0, 0
    s.response = h.ctypes.data_as(C.POINTER(C.c_float))
    return s, h   # (h keeps the taps alive)


BAD = [(2, 0, [0, 0], b"inputs = 0"), (2, -1, [0, 0], b"inputs = -1"), (2, 3, [0, 1], b"inputs = 3"), (2, 1, None, b"source NULL"),
       (2, 1, [0, 1], b"source[1] = 1"), (3, 2, [0, -1, 1], b"source[1] = -1"), (3, 2, [0, 2, 1], b"source[1] = 2"),
       (3, 2, [1, 1, 1], b"input 0"), (4, 3, [0, 2, 2, 0], b"input 1")]


@pytest.mark.parametrize("on", [False, True])
def test_invalid_routings_are_einval_before_a_device_is_touched(on):
    import fundsp_amd
    from fundsp_amd import _lib

    L = fundsp_amd.lib()

    def create(instances, spec, inputs, source):
        out = C.c_void_p(1)   # (a stale value: the call leaves NULL)
        src = None if source is None else (C.c_int * len(source))(*source)
        sp = None if spec is None else C.byref(spec)
        if on:
            rc = L.fdsp_convolve_routed_create_on(-1, instances, sp, inputs, src, C.byref(out))
        else:
            rc = L.fdsp_convolve_routed_create(instances, sp, inputs, src, C.byref(out))
        return rc, out.value, L.fdsp_last_error()

    for channels, inputs, source, msg in BAD:
        s, _h = spec_of(channels)
        rc, out, err = create(3, s, inputs, source)
        assert rc == _lib.EINVAL and not out and msg in err, (channels, inputs, source, rc, out, err)
    s, _h = spec_of(2)
    rc, out, err = create(3, None, 1, [0, 0])
    assert rc == _lib.EINVAL and not out and b"spec NULL" in err
    rc, out, err = create(0, s, 1, [0, 0])
    assert rc == _lib.EINVAL and not out and b"no instances" in err
    s.channels = 9   # what the plain constructor refuses is refused here too
    rc, out, err = create(3, s, 1, [0] * 9)
    assert rc == _lib.EINVAL and not out and b"channels" in err
    if on:
        assert L.fdsp_convolve_routed_create_on(-1, 3, C.byref(spec_of(2)[0]), 1, (C.c_int * 2)(0, 0), None) == _lib.EINVAL
    else:
        assert L.fdsp_convolve_routed_create(3, C.byref(spec_of(2)[0]), 1, (C.c_int * 2)(0, 0), None) == _lib.EINVAL


def test_convolve_route_plan():
    from fundsp_amd import graph as G

    rng = np.random.default_rng(3)
    w = rng.uniform(-1, 1, (4, 12)).astype(np.float32)
    a, b, c, d = (G.convolve(w, i) for i in range(4))
    h, source, inputs = G.convolve_route_plan(a)
    assert (h == w[0:1]).all() and (source, inputs) == ([0], 1)
    h, source, inputs = G.convolve_route_plan(a ^ b)
    assert (h == w[:2]).all() and h.dtype == np.float32 and (source, inputs) == ([0, 0], 1)
    h, source, inputs = G.convolve_route_plan((a ^ b) | (c ^ d))
    assert (h == w).all() and (source, inputs) == ([0, 0, 1, 1], 2)
    h, source, inputs = G.convolve_route_plan((a | b) ^ (c | d))
    assert (h == w).all() and (source, inputs) == ([0, 1, 0, 1], 2)
    h, source, inputs = G.convolve_route_plan(a ^ b ^ c)
    assert (h == w[:3]).all() and (source, inputs) == ([0, 0, 0], 1)
    h, source, inputs = G.convolve_route_plan(a | (b ^ c) | d)
    assert (h == w).all() and (source, inputs) == ([0, 1, 1, 2], 3)
    # a plain stack is the identity map
    h, source, inputs = G.convolve_route_plan(a | b)
    assert (h == w[:2]).all() and (source, inputs) == ([0, 1], 2)
    # shorter responses are zero-padded to the longest
    h, source, inputs = G.convolve_route_plan(G.convolve(w[0, :5]) ^ a ^ G.convolve([2.0]))
    assert h.shape == (3, 12) and (h[0, :5] == w[0, :5]).all() and not h[0, 5:].any() and (h[1] == w[0]).all()
    assert h[2, 0] == 2.0 and not h[2, 1:].any() and (source, inputs) == ([0, 0, 0], 1)
    # eight outputs are a bank, nine are not
    eight = a ^ a ^ a ^ a ^ a ^ a ^ a ^ a
    assert G.convolve_route_plan(eight)[1] == [0] * 8
    with pytest.raises(ValueError, match="1 .. 8"):
        G.convolve_route_plan(eight ^ a)
    # anything but convolvers under the stacks and branches; a pipe
    assert G.convolve_route_plan(G.convolve(w) ^ G.pass_()) is None
    assert G.convolve_route_plan(G.noise() >> a) is None
    assert G.convolve_route_plan(G.noise()) is None
    # convolve_plan keeps reading stacks only
    assert G.convolve_plan(a ^ b) is None and G.convolve_plan((a ^ b) | c) is None
    assert (G.convolve_plan(a | b) == w[:2]).all()
    assert (a ^ b).branch_parts == (a, b) and ((a ^ b).nin, (a ^ b).nout) == (1, 2)
