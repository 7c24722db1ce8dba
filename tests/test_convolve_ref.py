"""Host checks of the convolver banks' restatement (tests/convolve_ref.py) and of what the host decides before any launch: the reference's
known answer, the restatement against float64, every split of an input the same bits, spec validation, graph notation and routing."""
import ctypes as C

import numpy as np
import pytest

import convolve_ref as CR

B0 = 64   # the block length of every capacity up to 512 taps


def response(M, seed, shape=()):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, shape + (M,)) * np.exp(-np.arange(M) / (M / 5 + 1))).astype(np.float32)


def test_reference_known_answer():
    """tests/test_basic.rs:698-711: 0, 1, 0, 0, 0 into the response (1, 0.75, 0.5, 0.25) gives 0, 1, 0.75, 0.5, 0.25 within 1e-4 -- and here
    exactly: inside the first block only the head acts, and its products and sums of these values are exact"""
    y = CR.render(np.array([[[0.0, 1.0, 0.0, 0.0, 0.0]]], np.float32), [1.0, 0.75, 0.5, 0.25])[0, 0]
    want = np.array([0.0, 1.0, 0.75, 0.5, 0.25], np.float32)
    assert np.abs(y - want).max() <= 1e-4
    assert np.array_equal(y, want)
    # the same impulse just before a block boundary: the tail carries the response over it, still without latency
    x = np.zeros((1, 1, 2 * B0), np.float32)
    x[0, 0, B0 - 2] = 1.0
    y = CR.render(x, [1.0, 0.75, 0.5, 0.25])[0, 0]
    want = np.zeros(2 * B0, np.float32)
    want[B0 - 2:B0 + 2] = [1.0, 0.75, 0.5, 0.25]
    assert np.abs(y - want).max() <= 1e-4


CASES = [(M, kind) for M in (1, 3, B0 - 1, B0, B0 + 1, 5 * B0 + 17, 48000) for kind in ("noise", "impulse")]
BOUND = 4 * 1.01e-7     # four times the largest value in the table below
MODEL_CONSTANT = 1.0    # err <= MODEL_CONSTANT * sqrt(P) * log2(2B) * 2^-24


@pytest.mark.parametrize("M,kind", CASES)
def test_restatement_against_float64(M, kind):
    """max |y - y64| / (sum |h| * max |x|) against np.convolve in float64, decaying-noise response, input uniform noise or one impulse.
    Measured on the restatement (M, B: noise / impulse), and each as a fraction of the model sqrt(P) * log2(2B) * 2^-24:
        1, 64: 3.92e-08 / 0          (0.094 / 0)         3, 64: 7.17e-08 / 1.16e-08  (0.17 / 0.028)
       63, 64: 1.01e-07 / 6.29e-09   (0.24 / 0.015)     64, 64: 9.17e-08 / 4.48e-09  (0.22 / 0.011)
       65, 64: 8.56e-08 / 5.83e-09   (0.15 / 0.0099)   337, 64: 5.34e-08 / 3.02e-09  (0.052 / 0.0030)
    48000, 1024: 8.71e-09 / 7.53e-11 (0.0019 / 1.7e-05)
    The bound is four times the largest of them (the margin covers other seeds); the model holds with constant 1."""
    rng = np.random.default_rng(M)
    h = response(M, M)
    B = CR.block_length(M)
    assert B == (1024 if M == 48000 else B0)
    T = M + 3 * B + 11
    x = rng.uniform(-1.0, 1.0, T).astype(np.float32) if kind == "noise" else np.eye(1, T, 5, dtype=np.float32)[0]
    y = CR.render(x[None, None], h)[0, 0]
    y64 = np.convolve(x.astype(np.float64), h.astype(np.float64))[:T]
    err = np.abs(y - y64).max() / (np.abs(h).sum() * np.abs(x).max())
    P = -(-M // B)
    model = MODEL_CONSTANT * np.sqrt(P) * np.log2(2 * B) * 2.0 ** -24
    print(f"M={M} B={B} {kind}: err {err:.3g}, model {model:.3g}")
    assert err <= BOUND, (M, kind, err)
    assert err <= model, (M, kind, err, model)


def test_reference_check_wave_cases_within_1e_4():
    """the responses of tests/test_basic.rs:329-330 on noise: the reference's own bar, 1e-4 absolute, against float64"""
    rng = np.random.default_rng(7)
    x = rng.uniform(-1.0, 1.0, 500).astype(np.float32)
    for h in ([1.0, 0.9, 0.8], [0.5, 0.4, 0.3]):
        y = CR.render(x[None, None], h)[0, 0]
        assert np.abs(y - np.convolve(x.astype(np.float64), h)[:500]).max() <= 1e-4


def test_every_split_gives_the_same_bits():
    rng = np.random.default_rng(3)
    M, T = 200, 700
    h = response(M, 1, (2,))
    x = rng.uniform(-1.0, 1.0, (3, 2, T)).astype(np.float32)
    one = CR.render(x, h)
    for splits in ([1] * T, [1, 63, 64, B0 - 1, B0, B0 + 5, 3 * B0 + 7]):
        got = CR.render(x, h, splits=splits)
        assert np.array_equal(one.view(np.uint32), got.view(np.uint32)), splits[:3]
    # per-instance responses, and a reset / a new response in mid-stream start the node over
    hv = response(M, 2, (3, 2))
    y = CR.render(x, hv, events=[(300, "reset")])
    assert np.array_equal(y[..., 300:], CR.render(x[..., 300:], hv))
    y = CR.render(x, hv, max_len=M, events=[(300, hv[..., :50])])
    assert np.array_equal(y[..., 300:], CR.render(x[..., 300:], hv[..., :50], max_len=M))


def test_block_length_rule_matches_the_library():
    import fundsp_amd as F

    L = F.lib()
    for n in (1, 3, 512, 513, 2048, 2049, 4800, 48000, 96000, 131072, 131073, 1 << 21, 1 << 24):
        assert L.fdsp_convolve_block_length(n) == CR.block_length(n), n
    assert CR.block_length(96000) == 1024 and CR.block_length(4800) == 256 and CR.block_length(1 << 24) == 4096


def test_invalid_specs_are_refused_before_any_device_work():
    import fundsp_amd as F
    from fundsp_amd import _lib

    L = F.lib()
    h = np.ones(16, np.float32)
    fp = h.ctypes.data_as(C.POINTER(C.c_float))
    cases = ((dict(channels=0), b"channels"), (dict(channels=9), b"channels"), (dict(max_len=0), b"max_len"), (dict(max_len=(1 << 24) + 1, len=4), b"max_len"),
             (dict(len=0), b"len"), (dict(len=17, max_len=16), b"len = 17"), (dict(per_instance=2), b"per_instance"),
             (dict(flush_denormals=-1), b"flush_denormals"), (dict(response=None), b"response NULL"))
    for kw, msg in cases:
        s = _lib.ConvolveSpec()
        s.channels, s.max_len, s.len = kw.get("channels", 1), kw.get("max_len", 16), kw.get("len", 16)
        s.per_instance, s.flush_denormals = kw.get("per_instance", 0), kw.get("flush_denormals", 0)
        s.response = kw.get("response", fp)
        out = C.c_void_p()
        assert L.fdsp_convolve_create(3, C.byref(s), C.byref(out)) == _lib.EINVAL, kw
        assert msg in L.fdsp_last_error(), (kw, L.fdsp_last_error())
        assert not out.value
    s = _lib.ConvolveSpec()
    s.channels, s.max_len, s.len, s.response = 1, 16, 16, fp
    assert L.fdsp_convolve_create(0, C.byref(s), C.byref(C.c_void_p())) == _lib.EINVAL
    assert L.fdsp_convolve_create(3, None, C.byref(C.c_void_p())) == _lib.EINVAL
    assert L.fdsp_convolve_set_response(None, fp, 16, 0, 1) == _lib.EINVAL


def test_response_rows_are_shaped_on_the_host():
    from fundsp_amd.bank import convolve_response_rows as rows

    h = np.arange(5, dtype=np.float32)
    assert rows(h, None, None).shape == (1, 5) and rows(h, 2, None).shape == (2, 5) and (rows(h, 2, None)[1] == h).all()
    assert rows(np.ones((2, 5)), None, None).shape == (2, 5) and rows(np.ones((1, 5)), 8, 4).shape == (4, 8, 5)
    t = rows(np.ones((4, 2, 5)), None, 4)
    assert t.shape == (4, 2, 5) and t.flags.c_contiguous and t.dtype == np.float32
    for bad, ch, n in ((np.ones((3, 5)), 2, None), (np.ones((2, 2, 5)), None, None), (np.ones((3, 2, 5)), None, 4), (np.ones(0), None, None),
                       (np.ones((9, 5)), None, None), (1.0, None, None)):
        with pytest.raises(ValueError):
            rows(bad, ch, n)


def test_graph_notation_checks_and_routes():
    from fundsp_amd import Bank
    from fundsp_amd import graph as G

    for args in (([],), (np.ones((2, 2, 3)),), ([1.0, 2.0], 1), (np.ones((2, 3)), 2), (np.ones((2, 3)), -1)):
        with pytest.raises(ValueError):
            G.convolve(*args)
    w = np.arange(6, dtype=np.float32).reshape(2, 3)
    c = G.convolve(w, 1)
    assert (c.nin, c.nout) == (1, 1) and G.has_convolve(c) and (c.convolve_response == w[1]).all()
    assert not G.has_convolve(G.noise() >> G.lowpass_hz(1000.0, 1.0))
    assert (G.convolve_plan(c) == w[1:2]).all()
    st = G.convolve(w, 0) | G.convolve([1.0, 2.0, 3.0, 4.0]) | G.convolve(w, 1)
    plan = G.convolve_plan(st)
    assert (st.nin, st.nout) == (3, 3) and plan.shape == (3, 4)
    assert (plan == np.array([[0, 1, 2, 0], [1, 2, 3, 4], [3, 4, 5, 0]], np.float32)).all(), "one channel each, zero-padded to the longest"
    assert G.convolve_plan(G.convolve(w) | G.pass_()) is None and G.convolve_plan(G.noise() >> c) is None
    # the type the hash probe walks carries Convolver::ID = 100
    assert "ID = 100" in c.source and (G.noise() >> c).type == "Pipe<Noise,ConvolvePing>"
    # any other position is refused on the host, with what is supported
    a, b = G.convolve([1.0, 0.9, 0.8]), G.convolve([0.5, 0.4, 0.3])
    for bad in (G.noise() >> a >> G.pass_(), a + G.pass_(), a | G.pass_(), G.pass_() >> (a >> G.pass_()), (G.noise() >> a) | (G.pink() >> b), a & b,
                a >> b):
        with pytest.raises(ValueError, match="front >> convolve"):
            Bank.from_graph(bad, 2)
