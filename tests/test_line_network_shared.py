"""Host-side checks (no GPU) of what the two line-network families share: fdsp_fdn_network_create and fdsp_feedback_delay_create refuse a bad
description in one text, and graph.fdn_network_plan and graph.feedback_delay_plan read a line `delay [>> fir] [>> F] [* g]` alike."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the shared refusals: (what is wrong, the message behind "<function name>: "); {line} / {loop}: the family's names of its two forms
SHARED = [
    (dict(taps=4), "taps takes 0 (no Fir node) .. 3"),
    (dict(taps=-1), "taps takes 0 (no Fir node) .. 3"),
    (dict(filter=3), "filter takes FDSP_FDN_FILTER_NONE, _LOWPOLE or _SVF"),
    (dict(filter=-1), "filter takes FDSP_FDN_FILTER_NONE, _LOWPOLE or _SVF"),
    (dict(filter="svf", svf_mode=9, cutoff=True, q=True, gain=True), "svf_mode takes FDSP_SVF_LOWPASS .. FDSP_SVF_HIGHSHELF"),
    (dict(filter="svf", svf_mode=-1, cutoff=True, q=True, gain=True), "svf_mode takes FDSP_SVF_LOWPASS .. FDSP_SVF_HIGHSHELF"),
    (dict(place=2), "place takes FDSP_FDN_IN_LINE ({line}) or FDSP_FDN_IN_LOOP ({loop})"),
    (dict(place="loop"), "the loop form ({loop}) needs a filter"),
    (dict(delays=None), "delays NULL"),
    (dict(taps=2), "weights NULL"),
    (dict(filter="lowpole"), "the filter's cutoff is missing"),
    (dict(filter="svf", svf_mode=0), "the filter's cutoff is missing"),
    (dict(filter="svf", svf_mode=0, cutoff=True), "the FixedSvf's q is missing"),
    (dict(filter="svf", svf_mode=6, cutoff=True, q=True), "bell / lowshelf / highshelf need a gain"),
    (dict(filter="svf", svf_mode=8, cutoff=True, q=True), "bell / lowshelf / highshelf need a gain"),
    (dict(sr=0.0), "sample_rate must be positive"),
    (dict(sr=-48000.0), "sample_rate must be positive"),
    (dict(sr=float("nan")), "sample_rate must be positive"),
    (dict(instances=0), "no instances"),
    (dict(delay=-0.005), "a delay is negative or not a number (Delay::new asserts time >= 0)"),
    (dict(delay=float("nan")), "a delay is negative or not a number (Delay::new asserts time >= 0)"),
]
FAMILIES = [("fdsp_fdn_network_create", "FdnNetwork", dict(lines=2, inputs=1, outputs=1), "fdn", "fdn2"),
            ("fdsp_feedback_delay_create", "FeedbackDelay", dict(channels=2), "feedback", "feedback2")]


@pytest.mark.parametrize("fn,struct,own,line,loop", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_both_constructors_refuse_a_bad_description_in_one_text(fn, struct, own, line, loop):
    import fundsp_amd
    from fundsp_amd import _lib

    L = fundsp_amd.lib()
    ones = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    fp = C.cast(ones, C.POINTER(C.c_float))
    for bad, text in SHARED:
        bad = dict(bad)
        d = (C.c_double * 2)(0.005, bad.pop("delay", 0.005))
        net = getattr(_lib, struct)(delays=d, **own)
        instances, sr = bad.pop("instances", 2), bad.pop("sr", 48000.0)
        for k, v in bad.items():
            if k == "filter" and isinstance(v, str):
                v = {"lowpole": _lib.FDN_FILTER_LOWPOLE, "svf": _lib.FDN_FILTER_SVF}[v]
            elif k == "place" and v == "loop":
                v = _lib.FDN_IN_LOOP
            elif k in ("cutoff", "q", "gain"):
                v = fp
            setattr(net, k, v)
        out = C.c_void_p(1)   # (a stale value: the call leaves NULL)
        rc = getattr(L, fn)(instances, C.byref(net), sr, C.byref(out))
        want = (fn + ": " + text.format(line=line, loop=loop)).encode()
        assert rc == _lib.EINVAL and not out.value and L.fdsp_last_error() == want, (fn, bad, rc, L.fdsp_last_error(), want)


def test_a_constructors_own_checks_keep_their_place_among_the_shared_ones():
    import fundsp_amd
    from fundsp_amd import _lib

    L = fundsp_amd.lib()
    d = (C.c_double * 2)(0.005, 0.005)
    one = C.cast((C.c_float * 2)(0.5, 0.5), C.POINTER(C.c_float))

    def err(fn, net):
        out = C.c_void_p(1)
        assert getattr(L, fn)(2, C.byref(net), 48000.0, C.byref(out)) == _lib.EINVAL and not out.value
        return L.fdsp_last_error()

    # network: lines, taps, inputs / outputs, filter
    assert b"lines takes" in err("fdsp_fdn_network_create", _lib.FdnNetwork(lines=3, taps=4, inputs=1, outputs=1, delays=d))
    assert b"taps takes" in err("fdsp_fdn_network_create", _lib.FdnNetwork(lines=2, taps=4, inputs=3, outputs=1, delays=d))
    assert b"inputs / outputs take" in err("fdsp_fdn_network_create", _lib.FdnNetwork(lines=2, inputs=3, outputs=1, filter=7, delays=d))
    # feedback delay: channels, taps, .., loop needs a filter, the outer gain in the loop form, reverse, delays NULL
    assert b"channels takes" in err("fdsp_feedback_delay_create", _lib.FeedbackDelay(channels=3, taps=4, delays=d))
    assert b"needs a filter" in err("fdsp_feedback_delay_create", _lib.FeedbackDelay(channels=1, place=_lib.FDN_IN_LOOP, outer_gain=one, delays=d))
    assert b"no outer gain" in err("fdsp_feedback_delay_create", _lib.FeedbackDelay(channels=1, place=_lib.FDN_IN_LOOP, filter=_lib.FDN_FILTER_LOWPOLE,
                                                                                   cutoff=one, outer_gain=one, reverse=1, delays=d))
    assert b"reverse() needs two channels" in err("fdsp_feedback_delay_create", _lib.FeedbackDelay(channels=1, reverse=1))


# ---- the table filler, on the host --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("san", [(), ("-Xarch_host", "-fsanitize=undefined,float-cast-overflow", "-Xarch_host", "-fno-sanitize-recover=all")],
                         ids=["plain", "ubsan"])
def test_table_filler_for_both_row_types_and_the_ring_limit(tmp_path, san):
    """tests/host/check_line_table.hip: a stand-alone host program (no kernel, no device), once plainly and once under the undefined-behaviour
    sanitizer -- a sample count past `int` is refused before it is converted"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "check_line_table"
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wno-unused-result", *san,
           "-I", os.path.join(ROOT, "fundsp_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
           os.path.join(ROOT, "tests", "host", "check_line_table.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "bad 0" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---- the two recognisers read a line alike ---------------------------------------------------------------------------------------------
V = 3
SHARED_KEYS = ("delays", "weights", "filter", "cutoff", "q", "gain", "line_gain", "place")
FILTERS = [None, "lowpole", "lowpass", "highpass", "bandpass", "notch", "peak", "allpass", "bell", "lowshelf", "highshelf"]
PER_VOICE = np.array([0.9, 1.0, 1.1], dtype=np.float32)   # one value per voice: the scale of the parameter that is an array


def line_parts(G, taps, filt, gained, per):
    """(delay [>> fir], [F], g | None) of one line; `per`: the parameter that is a per-voice array (None: all scalars)"""
    s = lambda name, x: x * PER_VOICE if per == name else x
    x = G.delay(s("delay", 0.01))
    if taps:
        x = x >> G.fir(*[s("w0", 0.5) if j == 0 else 0.25 / j for j in range(taps)])
    if filt is None:
        f = None
    elif filt == "lowpole":
        f = G.lowpole_hz(s("cutoff", 900.0))
    elif filt in ("bell", "lowshelf", "highshelf"):
        f = getattr(G, filt + "_hz")(s("cutoff", 900.0), s("q", 0.7), s("gain", 2.0))
    else:
        f = getattr(G, filt + "_hz")(s("cutoff", 900.0), s("q", 0.7))
    return x, f, (s("g", 0.5) if gained else None)


def both_plans(G, taps, filt, gained, loop, per, voices=V):
    def y(f, g):
        return f if g is None else f * g

    def whole(x, f, g):   # the line form's line
        x = x if f is None else x >> f
        return x if g is None else x * g

    x, f, g = line_parts(G, taps, filt, gained, per)
    if loop:
        net = G.split(2) >> G.fdn2(G.stacki(2, lambda i: x), G.stacki(2, lambda i: y(f, g))) >> G.join(2)
        fbd = G.feedback2(x | x, y(f, g) | y(f, g))
    else:
        net = G.split(2) >> G.fdn(G.stacki(2, lambda i: whole(x, f, g))) >> G.join(2)
        fbd = G.feedback(whole(x, f, g) | whole(x, f, g))
    return G.fdn_network_plan(net, voices), G.feedback_delay_plan(fbd, voices)


def per_voice_choices(taps, filt, gained):
    names = ["delay"] + (["w0"] if taps else []) + (["g"] if gained else [])
    if filt is not None:
        names += ["cutoff"] + ([] if filt == "lowpole" else ["q"]) + (["gain"] if filt in ("bell", "lowshelf", "highshelf") else [])
    return [None] + names


@pytest.mark.parametrize("filt", FILTERS, ids=[str(f) for f in FILTERS])
def test_both_recognisers_read_a_line_alike(filt):
    from fundsp_amd import graph as G

    cases = 0
    for taps, gained, loop in itertools.product((0, 1, 2, 3), (False, True), (False, True)):
        if loop and filt is None:
            continue              # the loop form exists where a filter does
        for per in per_voice_choices(taps, filt, gained):
            a, b = both_plans(G, taps, filt, gained, loop, per)
            what = (taps, filt, gained, loop, per)
            assert a is not None and b is not None, what
            for k in SHARED_KEYS:
                assert (k in a) == (k in b), (what, k)
                if k not in a:
                    continue
                if isinstance(a[k], np.ndarray):
                    assert isinstance(b[k], np.ndarray) and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and (a[k] == b[k]).all(), (what, k, a[k], b[k])
                else:
                    assert type(a[k]) is type(b[k]) and a[k] == b[k], (what, k, a[k], b[k])
            # and what they read is the line that was written
            assert a["place"] == ("loop" if loop else "line") and a.get("filter") == filt and ("weights" in a) == (taps > 0) and ("line_gain" in a) == gained, what
            assert a["delays"].shape == ((V, 2) if per == "delay" else (2,)) and a["delays"].dtype == np.float64, what
            if taps:
                assert a["weights"].shape == ((V, 2, taps) if per == "w0" else (2, taps)), what
            # a per-voice array of another length: None from both
            if per is not None:
                assert both_plans(G, taps, filt, gained, loop, per, voices=V + 1) == (None, None), what
            cases += 1
    assert cases >= (8 if filt is None else 32)


def test_a_second_filter_is_none_from_both():
    from fundsp_amd import graph as G

    for second in (lambda: G.lowpole_hz(400.0), lambda: G.lowpass_hz(400.0, 0.7)):
        line = lambda: G.delay(0.01) >> G.fir(0.5, 0.25) >> G.lowpole_hz(900.0) >> second()
        assert G.fdn_network_plan(G.split(2) >> G.fdn(G.stacki(2, lambda i: line())) >> G.join(2)) is None
        assert G.feedback_delay_plan(G.feedback(line() | line())) is None
        x, y = (lambda: G.delay(0.01)), (lambda: G.lowpole_hz(900.0) >> second() * 0.5)
        assert G.fdn_network_plan(G.split(2) >> G.fdn2(G.stacki(2, lambda i: x()), G.stacki(2, lambda i: y())) >> G.join(2)) is None
        assert G.feedback_delay_plan(G.feedback2(x() | x(), y() | y())) is None
    # two per-voice arrays of two lengths
    t3, g4 = np.full(3, 0.01, np.float32), np.full(4, 0.5, np.float32)
    assert G.fdn_network_plan(G.split(2) >> G.fdn(G.stacki(2, lambda i: G.delay(t3) * g4)) >> G.join(2)) is None
    assert G.feedback_delay_plan(G.feedback(G.delay(t3) * g4 | G.delay(t3) * g4)) is None
