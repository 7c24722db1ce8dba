"""numpy restatement of the summing convolver banks' contract (the last bullet of fundsp_amd/csrc/fd_convolve.hpp), for the tests.

A summing bank has I inputs, O outputs and NT terms: term t convolves input tin[t] with response row t and belongs to output tout[t]
(non-decreasing).  Block spectra are per (instance, input), response tables per (row, term), Z, pend and y per (instance, output).  The
tail of an output is ONE running sum over its terms in increasing t and, inside a term, over the partitions in increasing p; one inverse
transform gives pend.  The head is one running sum too: the first term starts it with h[0] * x[n], every later term adds h[0] * x[n] and
then the taps in increasing i.  Everything else -- the block length, the transforms, the response spectra, `_Ops` and its flush rule -- is
convolve_ref's, which this file builds on.

`order` names single faults of that order, for the tests that show the order matters: "swap" exchanges the first two terms of every output
that has two, "per_term_sums" adds each term's own partition sum (and head sum) after the loops, "per_term_inverses" inverse-transforms
every term's sum and adds the rounded results.
"""
import numpy as np

import convolve_ref as CR
import resynth_ref as R

f32 = np.float32


def check_terms(term_input, term_output):
    """(tin, tout, I, O) of valid term tables"""
    tin, tout = [int(i) for i in term_input], [int(o) for o in term_output]
    assert 1 <= len(tin) == len(tout) <= 16
    I, O = max(tin) + 1, max(tout) + 1
    assert 1 <= I <= 8 and 1 <= O <= 8 and min(tin) >= 0
    assert all(a <= b for a, b in zip(tout[:-1], tout[1:])), "term_output is non-decreasing"
    assert sorted(set(tout)) == list(range(O)) and sorted(set(tin)) == list(range(I))
    return tin, tout, I, O


class MatrixConvolver(CR.Convolver):
    """V instances, response h [NT, M] or [V, NT, M]; x [V, I, T] -> y [V, O, T]"""

    def __init__(self, h, term_input, term_output, instances, max_len=None, ftz=False, block=None, order=None):
        self.tin, self.tout, self.I, self.O = check_terms(term_input, term_output)
        self.terms = [[t for t in range(len(self.tin)) if self.tout[t] == o] for o in range(self.O)]
        if order == "swap":
            self.terms = [[ts[1], ts[0]] + ts[2:] if len(ts) > 1 else ts for ts in self.terms]
        self.order = order
        super().__init__(h, instances, max_len=max_len, ftz=ftz, block=block)

    def set_response(self, h):
        super().set_response(h)          # taps and spectra per (row, term): the parent's "channels" are the terms
        assert self.C == len(self.tin)

    def reset(self):
        self.n = 0
        self.x = np.zeros((self.V, self.I, 0), dtype=f32)
        self.Xr, self.Xi = [], []
        self.pend = np.zeros((self.V, self.O, self.B), dtype=f32)

    def _complete_block(self, j):
        B, op = self.B, self.op
        seg = np.zeros((self.V, self.I, 2 * B), dtype=f32)
        seg[..., :B] = self.x[..., j * B:(j + 1) * B]
        Xr, Xi = R.rfft(seg, self.tw, op)
        self.Xr.append(Xr)
        self.Xi.append(Xi)
        j1 = j + 1
        zero = np.zeros((self.V, B + 1), dtype=f32)
        pend = np.empty((self.V, self.O, B), dtype=f32)
        split = self.order in ("per_term_sums", "per_term_inverses")
        for o, ts in enumerate(self.terms):
            Zr, Zi, sums = zero, zero, []
            for t in ts:
                i = self.tin[t]
                for p in range(min(self.P, j1)):
                    ar, ai = self.Xr[j1 - 1 - p][:, i], self.Xi[j1 - 1 - p][:, i]
                    br, bi = self.Gr[:, t, p], self.Gi[:, t, p]          # rows broadcast over the instances
                    pr = op.sub(op.mul(ar, br), op.mul(ai, bi))
                    pi = op.add(op.mul(ar, bi), op.mul(ai, br))
                    Zr, Zi = op.add(Zr, pr), op.add(Zi, pi)
                if split:                                        # (the faults) every term its own sum from zero
                    sums.append((Zr, Zi))
                    Zr, Zi = zero, zero
            if self.order == "per_term_sums":
                Zr, Zi = sums[0]
                for qr, qi in sums[1:]:
                    Zr, Zi = op.add(Zr, qr), op.add(Zi, qi)
            if self.order == "per_term_inverses":
                ys = [R.irfft_re(qr, qi, self.tw, op)[..., :B] for qr, qi in sums]
                pend[:, o] = ys[0]
                for q in ys[1:]:
                    pend[:, o] = op.add(pend[:, o], q)
            else:
                pend[:, o] = R.irfft_re(Zr, Zi, self.tw, op)[..., :B]
        self.pend = pend
        if j1 - 1 - (self.P - 1) > 0:                            # spectra no later boundary reads
            self.Xr[j1 - self.P - 1] = self.Xi[j1 - self.P - 1] = None

    def process(self, x):
        """x [V, I, T] -> y [V, O, T], continuing from the samples so far"""
        x = np.asarray(x, dtype=f32)
        B, op, M = self.B, self.op, self.M
        T = x.shape[-1]
        y = np.empty((self.V, self.O, T), dtype=f32)
        self.x = np.concatenate([self.x, x], axis=-1)
        t0 = 0
        while t0 < T:
            j, r0 = divmod(self.n, B)
            cnt = min(B - r0, T - t0)                            # the samples of this call inside block j
            for o, ts in enumerate(self.terms):
                a, sums = None, []
                for t in ts:
                    xb = self.x[:, self.tin[t], j * B:j * B + r0 + cnt]
                    ht = self.h[:, t]                            # [rows, Hcap]
                    first = op.mul(ht[:, 0:1], xb[:, r0:])
                    a = first if a is None else op.add(a, first)
                    for i in range(1, min(r0 + cnt - 1, M - 1) + 1):
                        k = max(i - r0, 0)                       # tap i meets the samples r >= i of the block
                        a[:, k:] = op.add(a[:, k:], op.mul(ht[:, i:i + 1], xb[:, r0 + k - i:r0 + cnt - i]))
                    if self.order == "per_term_sums":            # (the fault) every term its own sum
                        sums.append(a)
                        a = None
                if sums:
                    a = sums[0]
                    for q in sums[1:]:
                        a = op.add(a, q)
                y[:, o, t0:t0 + cnt] = op.add(self.pend[:, o, r0:r0 + cnt], a)
            self.n += cnt
            t0 += cnt
            if self.n % B == 0:
                self._complete_block(j)
        return y


def render(x, h, term_input, term_output, max_len=None, ftz=False, block=None, splits=None, events=(), order=None):
    """y [V, O, T] of a fresh summing bank fed x [V, I, T].  `splits`, `events`: as convolve_ref.render."""
    x = np.asarray(x, dtype=f32)
    V, _, T = x.shape
    cv = MatrixConvolver(h, term_input, term_output, V, max_len=max_len, ftz=ftz, block=block, order=order)
    assert x.shape[1] == cv.I
    cuts = {0, T}
    if splits is not None:
        cuts |= set(np.cumsum(splits).tolist())
    ev = {}
    for S, what in events:
        ev[int(S)] = what
        cuts.add(int(S))
    cuts = sorted(c for c in cuts if 0 <= c <= T)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a in ev:
            if isinstance(ev[a], str):
                cv.reset()
            else:
                cv.set_response(ev[a])
        parts.append(cv.process(x[..., a:b]))
    return np.concatenate(parts, axis=-1) if parts else np.zeros((V, cv.O, 0), f32)
