"""graph.fdn_network_plan: the filtered / per-instance Hadamard networks (fdn with a line filter, fdn2 with a loop filter, per-line FIR weights,
per-voice parameters) become the arguments of Bank.fdn_network; anything else stays with the run-time compiler.  graph.fdn_plan keeps
refusing all of these shapes.  Host only."""
import numpy as np
import pytest

from fundsp_amd import graph as G

D = [0.01 + 0.001 * i for i in range(32)]


def line_net(n, line, head=None, tail=None):
    return (head or G.split(n)) >> G.fdn(G.stacki(n, line)) >> (tail or G.join(n))


def loop_net(n, x, y, head=None, tail=None):
    return (head or G.split(n)) >> G.fdn2(G.stacki(n, x), G.stacki(n, y)) >> (tail or G.join(n))


def f32(x):
    return float(np.float32(x))


def test_line_form_with_lowpole_gain_and_per_line_weights():
    g = line_net(16, lambda i: G.delay(D[i]) >> G.fir(0.1 * (i + 1), 0.4, 0.2) >> G.lowpole_hz(1000.0 + 10 * i) * 0.9)
    p = G.fdn_network_plan(g)
    assert p["lines"] == 16 and p["place"] == "line" and p["filter"] == "lowpole" and p["inputs"] == 1 and p["outputs"] == 1
    assert p["weights"].shape == (16, 3) and p["weights"][3, 0] == np.float32(0.4) and p["weights"][3, 1] == np.float32(0.4)
    assert p["delays"][5] == f32(D[5]) and p["cutoff"][2] == np.float32(1020.0) and p["line_gain"][7] == np.float32(0.9)
    assert "q" not in p and G.fdn_plan(g) is None


def test_loop_form_fdn2_with_svf():
    g = loop_net(8, lambda i: G.delay(D[i]) >> G.fir(0.5, 0.5), lambda i: G.highshelf_hz(3000.0, 0.7, 0.5) * 0.8,
                 G.multisplit(2, 4), G.multijoin(2, 4))
    p = G.fdn_network_plan(g)
    assert p["place"] == "loop" and p["filter"] == "highshelf" and p["inputs"] == 2 and p["outputs"] == 2
    assert p["q"][0] == np.float32(0.7) and p["gain"][0] == np.float32(0.5) and p["line_gain"][0] == np.float32(0.8)
    assert p["weights"].shape == (8, 2)
    assert G.fdn_plan(g) is None
    g = loop_net(4, lambda i: G.delay(D[i]), lambda i: G.lowpole_hz(2000.0))   # no Fir node, no gain
    p = G.fdn_network_plan(g)
    assert "weights" not in p and "line_gain" not in p and p["filter"] == "lowpole"


@pytest.mark.parametrize("n", [2, 32])
def test_no_fir_node_and_gain_only(n):
    p = G.fdn_network_plan(line_net(n, lambda i: G.delay(D[i]) >> G.lowpass_hz(5000.0, 1.0)))
    assert p["lines"] == n and "weights" not in p and p["filter"] == "lowpass"
    p = G.fdn_network_plan(line_net(n, lambda i: G.delay(D[i]) * 0.7))
    assert "filter" not in p and p["line_gain"][0] == np.float32(0.7)
    assert G.fdn_plan(line_net(n, lambda i: G.delay(D[i]) * 0.7)) is None


def test_per_voice_arrays():
    V = 5
    room = np.linspace(1.0, 2.0, V, dtype=np.float32)
    g = line_net(4, lambda i: G.delay(room * np.float32(D[i])) >> G.fir(0.3, 0.3) >> G.lowpole_hz(np.full(V, 800.0 + i, np.float32)))
    p = G.fdn_network_plan(g, V)
    assert p["delays"].shape == (V, 4) and p["cutoff"].shape == (V, 4) and p["weights"].shape == (4, 2)
    assert p["delays"][4, 1] == float(np.float32(room[4] * np.float32(D[1])))
    assert G.fdn_network_plan(g) is not None                        # (without a voice count the lengths only have to agree)
    assert G.fdn_network_plan(g, V + 1) is None                     # per-voice arrays of the wrong length
    assert G.fdn_plan(g) is None
    # arrays of two different lengths
    h = line_net(4, lambda i: G.delay(np.full(3 if i else 4, D[i], np.float32)) >> G.lowpole_hz(900.0))
    assert G.fdn_network_plan(h) is None


def test_refusals():
    lp = lambda i: G.delay(D[i]) >> G.lowpole_hz(1000.0)
    assert G.fdn_network_plan(line_net(3, lp)) is None                                            # not a power of two
    assert G.fdn_network_plan(line_net(64, lambda i: G.delay(0.01) >> G.lowpole_hz(1000.0))) is None   # more lines than the kernel holds
    # a feedback2 without the Hadamard
    g = G.split(4) >> G.feedback2(G.stacki(4, lambda i: G.delay(D[i])), G.stacki(4, lambda i: G.lowpole_hz(1000.0))) >> G.join(4)
    assert G.fdn_network_plan(g) is None
    assert G.fdn_network_plan(G.split(4) >> G.feedback(G.stacki(4, lp)) >> G.join(4)) is None
    # line filters outside the set
    assert G.fdn_network_plan(line_net(4, lambda i: G.delay(D[i]) >> G.highpole_hz(1000.0))) is None
    assert G.fdn_network_plan(line_net(4, lambda i: G.delay(D[i]) >> G.moog_hz(1000.0, 0.5))) is None
    assert G.fdn_network_plan(line_net(4, lambda i: G.delay(D[i]) >> G.lowpole_hz(1000.0) >> G.lowpole_hz(900.0))) is None
    # the loop form needs a filter in y and nothing but delay >> fir in x
    assert G.fdn_network_plan(loop_net(4, lambda i: G.delay(D[i]), lambda i: G.pass_() * 0.5)) is None
    assert G.fdn_network_plan(loop_net(4, lambda i: G.delay(D[i]) >> G.lowpole_hz(900.0), lambda i: G.lowpole_hz(900.0))) is None
    # a gain in front of the filter, a SVF mode that differs between lines
    assert G.fdn_network_plan(line_net(4, lambda i: G.delay(D[i]) * 0.5 >> G.lowpole_hz(900.0))) is None
    assert G.fdn_network_plan(line_net(4, lambda i: G.delay(D[i]) >> (G.lowpass_hz(900.0, 1.0) if i else G.highpass_hz(900.0, 1.0)))) is None
    # heads and tails that are not split / join of N
    assert G.fdn_network_plan(G.split(4) >> G.fdn(G.stacki(4, lp)) >> G.join(4) >> G.lowpole_hz(500.0)) is None
    assert G.fdn_network_plan(G.multisplit(4, 1) >> G.fdn(G.stacki(4, lp)) >> G.join(4)) is None
    assert G.fdn_network_plan(G.sine_hz(440.0)) is None and G.fdn_network_plan(G.reverb4_stereo(20.0, 2.0)) is None


def test_the_uniform_fdn_shape_is_also_a_network_and_lane_per_frame():
    g = line_net(16, lambda i: G.delay(D[i]) >> G.fir(0.2, 0.4, 0.2))
    assert G.fdn_plan(g) is not None
    p = G.fdn_network_plan(g)
    assert p["weights"].shape == (16, 3) and "filter" not in p
    assert G.lane_per_frame_shape(line_net(4, lambda i: G.delay(D[i]) >> G.lowpole_hz(1000.0)))
    assert G.lane_per_frame_shape(loop_net(4, lambda i: G.delay(D[i]), lambda i: G.lowpole_hz(1000.0)))
