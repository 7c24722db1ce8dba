"""The ring limit of the lane-per-frame line networks, in both families (fdsp_fdn_network_create, fdsp_feedback_delay_create): a ring holds at
most 2^18 slots, so a delay of 2^18 - 1 samples is the longest.  One more sample is refused, and so is a delay whose sample count has no
`int` value (1e5 s at 48 kHz: below the constructors' bound of 1e6 s) -- both with FDSP_EINVAL, "2^18" in the message and no bank."""
import ctypes as C

import numpy as np
import pytest

from fundsp_amd import LAYOUT_PLANAR, _lib

pytestmark = pytest.mark.gpu
SR = 48000.0
V = 2
FAMILIES = [("fdsp_fdn_network_create", lambda d: _lib.FdnNetwork(lines=2, inputs=1, outputs=1, delays=d)),
            ("fdsp_feedback_delay_create", lambda d: _lib.FeedbackDelay(channels=2, delays=d))]


@pytest.mark.parametrize("fn,mk", FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize("delay", [2 ** 18 / SR, 1e5], ids=["2^18 samples", "1e5 s"])
def test_a_ring_of_more_than_2_18_slots_is_refused(gpu, fn, mk, delay):
    L = gpu.lib()
    d = (C.c_double * 2)(0.005, delay)
    if delay < 1e5:
        assert round(d[1] * SR) == 2 ** 18   # (the ring is one slot longer)
    net = mk(d)
    h = C.c_void_p(1)
    rc = getattr(L, fn)(V, C.byref(net), SR, C.byref(h))
    assert rc == _lib.EINVAL and not h.value and b"2^18" in L.fdsp_last_error() and L.fdsp_last_error().startswith(fn.encode()), (rc, h.value, L.fdsp_last_error())


@pytest.mark.parametrize("family", ["fdn_network", "feedback_delay"])
def test_the_longest_ring_is_created_and_renders(gpu, family):
    import torch

    delays = [0.005, (2 ** 18 - 1) / SR]
    assert round(delays[1] * SR) == 2 ** 18 - 1
    if family == "fdn_network":
        b = gpu.Bank.fdn_network(V, 2, delays, sample_rate=SR)
    else:
        b = gpu.Bank.feedback_delay(V, delays, sample_rate=SR)
    T = 65   # a block and a ragged one
    x = np.random.default_rng(5).random((V, b.inputs(), T), dtype=np.float32)
    y = b.process(T, torch.from_numpy(x).cuda(), layout=LAYOUT_PLANAR)
    torch.cuda.synchronize()
    y = y.cpu().numpy()[:, :, :T]
    # every delay is longer than the launch and the rings start empty: the lines give 0.0, and so do the join and the identity frame
    assert y.shape == (V, b.outputs(), T) and (y == 0.0).all()
