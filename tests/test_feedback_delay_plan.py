"""Host-side checks of the feedback delay banks (no GPU): the two new C ABI symbols in the header, the library, the ctypes table, the C++
wrapper and the Rust shim; graph.feedback_delay_plan on the reference's echo, ping-pong and comb shapes -- the line form and the loop form
with each filter, 0..3 FIR taps, per-voice parameters, stacki(2, ..) against `a | b` -- and on what stays with the run-time compiler."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fdsp_feedback_delay_create": 4, "fdsp_feedback_delay_create_on": 5}
FIELDS = ["channels", "taps", "filter", "svf_mode", "place", "reverse", "per_instance", "delays", "weights", "cutoff", "q", "gain", "line_gain",
          "outer_gain"]


def cpp_case(mode):
    """build tests/host/test_cpp_feedback_delay.cpp against the engine and the oracle and run it: --host here, --gpu on the device"""
    import oracle as O

    O.build()
    src = os.path.join(ROOT, "tests", "host", "test_cpp_feedback_delay.cpp")
    exe = os.path.join(ROOT, "tests", "host", "_build", "test_cpp_feedback_delay")
    lib = os.path.join(ROOT, "fundsp_amd", "libfundsp_hip.so")
    assert os.path.exists(lib), "build the HIP engine first (__graft_entry__.build())"
    deps = [src, os.path.join(ROOT, "include", "fundsp_hip.hpp"), os.path.join(ROOT, "include", "fundsp_hip.h"), lib,
            os.path.join(ROOT, "oracle", "libfundsp_oracle.so")]
    if not (os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call([
            "g++", "-std=c++17", "-O1", "-Wall", "-Wno-parentheses", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"),
            src, "-o", exe, "-L" + os.path.join(ROOT, "fundsp_amd"), "-lfundsp_hip", "-L" + os.path.join(ROOT, "oracle"), "-lfundsp_oracle",
            "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "fundsp_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
            "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failure(s)" in r.stdout, r.stdout + r.stderr


def test_cpp_host_side_argument_checks():
    cpp_case("--host")


def test_header_library_and_shims_agree_on_the_new_symbols():
    import fundsp_amd

    fundsp_amd.lib()
    text = open(os.path.join(ROOT, "include", "fundsp_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    shim = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rust_shim", "src", "lib.rs")).read())
    hpp = open(os.path.join(ROOT, "include", "fundsp_hip.hpp")).read()
    raw = C.CDLL(fundsp_amd._lib.SO_PATH)
    for name, nargs in NEW.items():
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == nargs, f"{name}: not declared with {nargs} parameters in include/fundsp_hip.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert len(fundsp_amd._lib.SYMBOLS[name][1]) == nargs, f"{name}: ctypes signature"
    r = re.search(r"pub fn fdsp_feedback_delay_create_on\s*\(([^)]*)\)", shim, flags=re.S)   # (the shim binds the `_on` constructors)
    assert r and len([a for a in r.group(1).split(",") if a.strip()]) == 5, "fdsp_feedback_delay_create_on: rust_shim"
    assert "fdsp_feedback_delay_create(" in hpp and "static Bank feedback_delay(" in hpp, "include/fundsp_hip.hpp"
    assert "pub fn feedback_delay" in shim, "HipBank lacks `feedback_delay`"
    # the struct: the same fields in the same order in the header, the ctypes table and the shim
    body = re.search(r"typedef struct fdsp_feedback_delay\s*\{(.*?)\}\s*fdsp_feedback_delay;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.split(None, 1)[1] if decl.strip() else "")]
    names = [n for n in names if n not in ("double", "float", "int", "const")]
    assert names == FIELDS, names
    assert [f[0] for f in fundsp_amd._lib.FeedbackDelay._fields_] == FIELDS
    rs = re.search(r"pub struct FdspFeedbackDelay\s*\{(.*?)\}", shim, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", rs) == FIELDS
    # the header states the grammar, the order of the operations and the rules
    for phrase in ("feedback( L [>> reverse()] [* g] )", "feedback2( L [>> reverse()], Y )", "xin_c = in_c[n] + value_c", "at least 128 samples", "2^18 slots"):
        assert phrase in text, phrase
    assert hasattr(fundsp_amd.Bank, "feedback_delay") and hasattr(fundsp_amd.Bank, "feedback_tree")


def test_invalid_descriptions_are_einval_before_a_device_is_touched():
    import fundsp_amd
    from fundsp_amd import _lib

    L = fundsp_amd.lib()
    d = (C.c_double * 3)(0.005, 0.005, 0.005)
    one = (C.c_float * 3)(0.5, 0.5, 0.5)

    def create(msg, instances=2, sr=48000.0, **kw):
        net = _lib.FeedbackDelay(channels=1, delays=d)
        for k, v in kw.items():
            setattr(net, k, v)
        out = C.c_void_p(1)   # (a stale value: the call leaves NULL)
        rc = L.fdsp_feedback_delay_create(instances, C.byref(net), sr, C.byref(out))
        assert rc == _lib.EINVAL and not out.value and msg in L.fdsp_last_error(), (kw, rc, L.fdsp_last_error())

    create(b"channels", channels=3)
    create(b"channels", channels=0)
    create(b"taps", taps=4)
    create(b"loop form", place=_lib.FDN_IN_LOOP)
    create(b"outer gain", place=_lib.FDN_IN_LOOP, filter=_lib.FDN_FILTER_LOWPOLE, cutoff=C.cast(one, C.POINTER(C.c_float)), outer_gain=C.cast(one, C.POINTER(C.c_float)))
    create(b"reverse", reverse=1)
    create(b"cutoff", filter=_lib.FDN_FILTER_LOWPOLE)
    create(b"weights", taps=2)
    create(b"no instances", instances=0)
    create(b"sample_rate", sr=0.0)
    out = C.c_void_p(1)
    assert L.fdsp_feedback_delay_create(2, None, 48000.0, C.byref(out)) == _lib.EINVAL and not out.value


def same(p, **want):
    assert p is not None and set(p) == set(want), (p, want)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert isinstance(p[k], np.ndarray) and p[k].dtype == v.dtype and p[k].shape == v.shape and (p[k] == v).all(), (k, p[k], v)
        else:
            assert type(p[k]) is type(v) and p[k] == v, (k, p[k], v)


f32 = lambda *x: np.array(x, dtype=np.float32)
f64 = lambda *x: np.array([float(np.float32(v)) for v in x], dtype=np.float64)


def test_the_reference_shapes():
    from fundsp_amd import graph as G

    g3, g6 = G._db_amp(-3.0), G._db_amp(-6.0)
    # README: feedback(delay(1.0) * db_amp(-3.0))
    same(G.feedback_delay_plan(G.feedback(G.delay(1.0) * g3)), place="line", reverse=False, delays=f64(1.0), line_gain=f32(g3))
    # README: feedback((delay(1.0) | delay(1.0)) >> reverse() * db_amp(-6.0)) -- Pipe<Stack, Unop<Reverse, MulScalar>>
    pp = G.feedback((G.delay(1.0) | G.delay(1.0)) >> G.reverse(2) * g6)
    assert pp.type == "Feedback<Pipe<Stack<Delay,Delay>,Unop<Reverse<2>,UMulScalar>>,FbId>"
    same(G.feedback_delay_plan(pp), place="line", reverse=True, delays=f64(1.0, 1.0), outer_gain=float(np.float32(g6)))
    # tests/test_basic.rs: feedback(delay(0.5) * 0.5)
    same(G.feedback_delay_plan(G.feedback(G.delay(0.5) * 0.5)), place="line", reverse=False, delays=f64(0.5), line_gain=f32(0.5))
    # the outer gain around the whole pipe is the same node as the one on reverse()
    same(G.feedback_delay_plan(G.feedback(((G.delay(0.3) | G.delay(0.4)) >> G.reverse(2)) * 0.5)), place="line", reverse=True, delays=f64(0.3, 0.4),
         outer_gain=0.5)
    same(G.feedback_delay_plan(G.feedback((G.delay(0.3) | G.delay(0.4)) * 0.5)), place="line", reverse=False, delays=f64(0.3, 0.4), outer_gain=0.5)
    same(G.feedback_delay_plan(G.feedback((G.delay(0.3) * 0.25 | G.delay(0.4) * 0.75) >> G.reverse(2))), place="line", reverse=True, delays=f64(0.3, 0.4),
         line_gain=f32(0.25, 0.75))
    # one channel: the first gain is the line's, the second the outer one
    same(G.feedback_delay_plan(G.feedback(G.delay(0.5) * 0.5 * 0.9)), place="line", reverse=False, delays=f64(0.5), line_gain=f32(0.5), outer_gain=float(np.float32(0.9)))


FILTERS = [("lowpole", lambda G, c: G.lowpole_hz(c)), ("lowpass", lambda G, c: G.lowpass_hz(c, 0.7)), ("bell", lambda G, c: G.bell_hz(c, 0.7, 2.0)),
           ("highshelf", lambda G, c: G.highshelf_hz(c, 0.7, 0.5))]


@pytest.mark.parametrize("name,mk", FILTERS, ids=[f[0] for f in FILTERS])
def test_line_and_loop_form_with_each_filter(name, mk):
    from fundsp_amd import graph as G

    svf = {} if name == "lowpole" else dict(q=f32(0.7), gain=f32(2.0 if name == "bell" else 0.5 if name == "highshelf" else 1.0))
    svf2 = {k: np.repeat(v, 2) for k, v in svf.items()}
    same(G.feedback_delay_plan(G.feedback(G.delay(0.01) >> mk(G, 900.0) * 0.5)), place="line", reverse=False, delays=f64(0.01), filter=name,
         cutoff=f32(900.0), line_gain=f32(0.5), **svf)
    same(G.feedback_delay_plan(G.feedback(G.delay(0.01) >> mk(G, 900.0))), place="line", reverse=False, delays=f64(0.01), filter=name, cutoff=f32(900.0), **svf)
    same(G.feedback_delay_plan(G.feedback2(G.delay(0.01), mk(G, 900.0) * 0.5)), place="loop", reverse=False, delays=f64(0.01), filter=name,
         cutoff=f32(900.0), line_gain=f32(0.5), **svf)
    two = G.feedback2((G.delay(0.01) | G.delay(0.02)) >> G.reverse(2), mk(G, 900.0) * 0.5 | mk(G, 1200.0) * 0.25)
    same(G.feedback_delay_plan(two), place="loop", reverse=True, delays=f64(0.01, 0.02), filter=name, cutoff=f32(900.0, 1200.0),
         line_gain=f32(0.5, 0.25), **svf2)
    two = G.feedback((G.delay(0.01) >> mk(G, 900.0) | G.delay(0.02) >> mk(G, 1200.0)) * 0.5)
    same(G.feedback_delay_plan(two), place="line", reverse=False, delays=f64(0.01, 0.02), filter=name, cutoff=f32(900.0, 1200.0), outer_gain=0.5, **svf2)


@pytest.mark.parametrize("taps", [0, 1, 2, 3])
def test_taps(taps):
    from fundsp_amd import graph as G

    w = [0.5, 0.25, 0.125][:taps]
    line = lambda t, s: (G.delay(t) >> G.fir(*[x * s for x in w])) if taps else G.delay(t)
    want = dict(weights=np.array([w], dtype=np.float32)) if taps else {}
    same(G.feedback_delay_plan(G.feedback(line(0.01, 1.0) * 0.5)), place="line", reverse=False, delays=f64(0.01), line_gain=f32(0.5), **want)
    want2 = dict(weights=np.array([w, [x * 0.5 for x in w]], dtype=np.float32)) if taps else {}
    same(G.feedback_delay_plan(G.feedback2(line(0.01, 1.0) | line(0.02, 0.5), G.lowpole_hz(500.0) | G.lowpole_hz(600.0))), place="loop", reverse=False,
         delays=f64(0.01, 0.02), filter="lowpole", cutoff=f32(500.0, 600.0), **want2)
    assert G.feedback_delay_plan(G.feedback(G.delay(0.01) >> G.fir(0.1, 0.1, 0.1, 0.1))) is None   # four taps


def test_per_instance_arrays_for_each_parameter():
    from fundsp_amd import graph as G

    V = 5
    ramp = lambda a, b: np.linspace(a, b, V, dtype=np.float32)
    t, c, q, gn, lg, og, w0 = ramp(0.003, 0.006), ramp(500.0, 900.0), ramp(0.5, 0.9), ramp(1.5, 2.5), ramp(0.5, 0.7), ramp(0.8, 0.9), ramp(0.2, 0.4)
    base = dict(place="line", reverse=False)
    same(G.feedback_delay_plan(G.feedback(G.delay(t) * 0.5), V), delays=t.astype(np.float64)[:, None], line_gain=f32(0.5), **base)
    same(G.feedback_delay_plan(G.feedback(G.delay(0.01) * lg), V), delays=f64(0.01), line_gain=lg[:, None], **base)
    same(G.feedback_delay_plan(G.feedback(G.delay(0.01) * 0.5 * og), V), delays=f64(0.01), line_gain=f32(0.5), outer_gain=og, **base)
    same(G.feedback_delay_plan(G.feedback(G.delay(0.01) >> G.fir(w0, 0.25)), V), delays=f64(0.01),
         weights=np.stack([w0, np.full(V, 0.25, np.float32)], axis=-1)[:, None, :], **base)
    same(G.feedback_delay_plan(G.feedback(G.delay(0.01) >> G.lowpole_hz(c)), V), delays=f64(0.01), filter="lowpole", cutoff=c[:, None], **base)
    p = G.feedback_delay_plan(G.feedback(G.delay(0.01) >> G.bell_hz(800.0, q, gn)), V)
    same(p, delays=f64(0.01), filter="bell", cutoff=f32(800.0), q=q[:, None], gain=gn[:, None], **base)
    # two channels, one of them per voice: the scalar side is repeated
    p = G.feedback_delay_plan(G.feedback((G.delay(t) | G.delay(0.004)) >> G.reverse(2) * og), V)
    same(p, place="line", reverse=True, delays=np.stack([t.astype(np.float64), np.full(V, float(np.float32(0.004)))], axis=1), outer_gain=og)
    assert G.feedback_delay_plan(G.feedback(G.delay(t) * 0.5)) is not None        # (without a voice count the lengths only have to agree)
    assert G.feedback_delay_plan(G.feedback(G.delay(t) * 0.5), V + 1) is None     # per-voice arrays of the wrong length
    assert G.feedback_delay_plan(G.feedback(G.delay(t) * lg[:4])) is None         # per-voice arrays of two different lengths
    assert G.feedback_delay_plan(G.feedback((G.delay(t) | G.delay(t[:3])) * 0.5)) is None


def test_stacki_equals_the_stack_operator():
    from fundsp_amd import graph as G

    t, c = [0.003, 0.005], [700.0, 900.0]
    a = G.feedback(G.stacki(2, lambda i: G.delay(t[i]) >> G.fir(0.5, 0.25) >> G.lowpole_hz(c[i]) * 0.5) >> G.reverse(2) * 0.9)
    b = G.feedback((G.delay(t[0]) >> G.fir(0.5, 0.25) >> G.lowpole_hz(c[0]) * 0.5 | G.delay(t[1]) >> G.fir(0.5, 0.25) >> G.lowpole_hz(c[1]) * 0.5) >> G.reverse(2) * 0.9)
    assert a.type != b.type
    pa, pb = G.feedback_delay_plan(a), G.feedback_delay_plan(b)
    same(pa, **pb)
    same(pa, place="line", reverse=True, delays=f64(*t), weights=np.array([[0.5, 0.25]] * 2, dtype=np.float32), filter="lowpole", cutoff=f32(*c),
         line_gain=f32(0.5, 0.5), outer_gain=float(np.float32(0.9)))
    ya = G.feedback2(G.stacki(2, lambda i: G.delay(t[i])), G.stacki(2, lambda i: G.lowpass_hz(c[i], 0.7)))
    yb = G.feedback2(G.delay(t[0]) | G.delay(t[1]), G.lowpass_hz(c[0], 0.7) | G.lowpass_hz(c[1], 0.7))
    same(G.feedback_delay_plan(ya), **G.feedback_delay_plan(yb))


def test_other_graphs_stay_with_the_compiler():
    from fundsp_amd import graph as G

    d = lambda: G.delay(0.01)
    assert G.feedback_delay_plan(G.fdn(G.stacki(2, lambda i: d()))) is None                          # fdn(..): the Hadamard frame
    assert G.feedback_delay_plan(G.fdn2(G.stacki(2, lambda i: d()), G.stacki(2, lambda i: G.lowpole_hz(500.0)))) is None
    assert G.feedback_delay_plan(G.split(2) >> G.fdn(G.stacki(2, lambda i: d())) >> G.join(2)) is None
    assert G.feedback_delay_plan(G.feedback(G.stacki(3, lambda i: d()))) is None                     # N = 3
    assert G.feedback_delay_plan(G.feedback(G.stacki(4, lambda i: d()))) is None                     # N = 4
    assert G.feedback_delay_plan(G.feedback(d() | d() | d())) is None
    assert G.feedback_delay_plan(G.feedback(G.lowpole_hz(500.0) >> d())) is None                     # a filter before the delay
    assert G.feedback_delay_plan(G.feedback(d() >> G.pinkpass())) is None                            # pinkpass in the line
    assert G.feedback_delay_plan(G.feedback(d() >> G.highpole_hz(500.0))) is None
    assert G.feedback_delay_plan(G.feedback(d() >> G.lowpole_hz(500.0) >> G.lowpole_hz(400.0))) is None
    assert G.feedback_delay_plan(G.feedback(d() * 0.5 >> G.lowpole_hz(500.0))) is None               # the gain before the filter
    assert G.feedback_delay_plan(G.feedback(d().seed(3) * 0.5)) is None                              # a node carrying an unused parameter
    assert G.feedback_delay_plan(G.feedback2(d(), G.pass_() * 0.5)) is None                          # the loop form without a filter
    assert G.feedback_delay_plan(G.feedback2(d() >> G.lowpole_hz(500.0), G.lowpole_hz(400.0))) is None
    assert G.feedback_delay_plan(G.feedback2(d() * 0.5, G.lowpole_hz(400.0))) is None
    assert G.feedback_delay_plan(G.feedback((d() | d() >> G.fir(0.5)) * 0.5)) is None                # two lines of two structures
    assert G.feedback_delay_plan(G.feedback((d() >> G.lowpass_hz(500.0, 1.0) | d() >> G.highpass_hz(500.0, 1.0)) * 0.5)) is None   # two SVF modes
    assert G.feedback_delay_plan(G.feedback((d() | d()) * 0.5 * 0.5)) is None                        # two outer gains
    assert G.feedback_delay_plan(G.feedback(d() * 0.5) >> G.lowpole_hz(500.0)) is None               # a pipe around the feedback
    assert G.feedback_delay_plan(G.sine_hz(440.0)) is None and G.feedback_delay_plan(G.reverb4_stereo(20.0, 2.0)) is None
    # the Hadamard planners keep refusing the identity frame
    assert G.fdn_plan(G.feedback(d() * 0.5)) is None and G.fdn_network_plan(G.feedback(d() * 0.5)) is None
