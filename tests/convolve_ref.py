"""numpy restatement of the convolver banks' contract (fundsp_amd/csrc/fd_convolve.hpp), for the tests.

Uniformly partitioned FFT convolution over COMPLETE blocks with a direct head, every operation one f32 rounding in the order the header
states, vectorised over instances and channels; `ftz=True` flushes every operand and result below 2^-126 to a zero of the same sign
(resynth_ref._Ops: a result on its exact value, before rounding, as the hardware does).  The transforms are resynth_ref's (the project's
cfft, the real-FFT split, the inverse), as the kernels share them.

Because only complete blocks are transformed and every output sample is a function of the absolute sample index, rendering in one piece, sample
by sample or in ragged pieces is the same computation: `Convolver.process` may be called with any split.
"""
import math

import numpy as np

import resynth_ref as R

f32 = np.float32


def block_length(max_len):
    """cv_block_length: the power of two at or above sqrt(8 * max_len), 64 .. 4096"""
    B = 64
    while B < 4096 and B * B < 8 * int(max_len):
        B *= 2
    return B


def blocks_per_chunk(V, C, B):
    """KB of fd_convolve.hpp: a launch is cut into chunks of at most KB * B samples, KB = clamp(256 MiB / (V * C * (B + 1) * 8 B), 8, 64)"""
    return min(max((256 << 20) // (int(V) * int(C) * (int(B) + 1) * 8), 8), 64)


def twiddles(N):
    tw = np.empty((N // 2, 2), dtype=f32)
    for j in range(N // 2):
        ang = 6.283185307179586476925286766559 * j / N
        tw[j, 0] = f32(math.cos(ang))
        tw[j, 1] = f32(-math.sin(ang))
    return tw


class Convolver:
    """V instances x C channels, response h [C, M] or [V, C, M]; max_len (default M) picks the block length."""

    def __init__(self, h, instances, max_len=None, ftz=False, block=None):
        self.V = int(instances)
        self.op = R._Ops(ftz)
        h = np.asarray(h, dtype=f32)
        self.max_len = int(max_len) if max_len is not None else h.shape[-1]
        self.B = int(block) if block is not None else block_length(self.max_len)
        self.tw = twiddles(2 * self.B)
        self.set_response(h)

    def set_response(self, h):
        """new taps, their partitions' spectra, and the history cleared"""
        h = np.asarray(h, dtype=f32)
        if h.ndim == 1:
            h = h[None]
        if h.ndim == 2:
            h = h[None]
        h = np.broadcast_to(h, (h.shape[0], h.shape[1], h.shape[2]))
        B, op = self.B, self.op
        self.C, self.M = h.shape[1], h.shape[2]
        assert self.M <= self.max_len
        self.P = (self.M + B - 1) // B
        hp = np.zeros(h.shape[:2] + ((self.P + 1) * B,), dtype=f32)
        hp[..., :self.M] = h
        self.h = hp
        # g_p[i] = h[(p+1)B + i] (i < B), 0 (i = B), h[pB + i - B] (i > B)
        g = np.empty(h.shape[:2] + (self.P, 2 * B), dtype=f32)
        for p in range(self.P):
            g[..., p, :B] = hp[..., (p + 1) * B:(p + 2) * B]
            g[..., p, B:] = hp[..., p * B:(p + 1) * B]
            g[..., p, B] = 0.0
        self.Gr, self.Gi = R.rfft(g, self.tw, op)       # [rows, C, P, B + 1]
        self.reset()

    def reset(self):
        self.n = 0
        self.x = np.zeros((self.V, self.C, 0), dtype=f32)      # the whole input since the reset (a test's lengths are small)
        self.Xr, self.Xi = [], []                              # spectra of the complete blocks
        self.pend = np.zeros((self.V, self.C, self.B), dtype=f32)   # pend_j of the current block j (pend_0 = +0.0)

    def _complete_block(self, j):
        """the count reached (j + 1)B: X_j, then pend_{j+1}"""
        B, op = self.B, self.op
        seg = np.zeros((self.V, self.C, 2 * B), dtype=f32)
        seg[..., :B] = self.x[..., j * B:(j + 1) * B]
        Xr, Xi = R.rfft(seg, self.tw, op)
        self.Xr.append(Xr)
        self.Xi.append(Xi)
        j1 = j + 1
        Zr = np.zeros((self.V, self.C, B + 1), dtype=f32)
        Zi = np.zeros_like(Zr)
        for p in range(min(self.P, j1)):
            ar, ai = self.Xr[j1 - 1 - p], self.Xi[j1 - 1 - p]
            br, bi = self.Gr[:, :, p], self.Gi[:, :, p]          # rows broadcast over the instances
            pr = op.sub(op.mul(ar, br), op.mul(ai, bi))
            pi = op.add(op.mul(ar, bi), op.mul(ai, br))
            Zr, Zi = op.add(Zr, pr), op.add(Zi, pi)
        self.pend = R.irfft_re(Zr, Zi, self.tw, op)[..., :B]
        if j1 - 1 - (self.P - 1) > 0:                            # spectra no later boundary reads
            self.Xr[j1 - self.P - 1] = self.Xi[j1 - self.P - 1] = None

    def process(self, x):
        """x [V, C, T] -> y [V, C, T], continuing from the samples so far"""
        x = np.asarray(x, dtype=f32)
        B, op, M = self.B, self.op, self.M
        T = x.shape[-1]
        y = np.empty((self.V, self.C, T), dtype=f32)
        self.x = np.concatenate([self.x, x], axis=-1)
        t = 0
        while t < T:
            j, r0 = divmod(self.n, B)
            cnt = min(B - r0, T - t)                            # the samples of this call inside block j
            xb = self.x[..., j * B:j * B + r0 + cnt]
            a = op.mul(self.h[..., 0:1], xb[..., r0:])
            for i in range(1, min(r0 + cnt - 1, M - 1) + 1):
                k = max(i - r0, 0)                              # tap i meets the samples r >= i of the block: a[k:] (slices, at 4096 taps)
                a[..., k:] = op.add(a[..., k:], op.mul(self.h[..., i:i + 1], xb[..., r0 + k - i:r0 + cnt - i]))
            y[..., t:t + cnt] = op.add(self.pend[..., r0:r0 + cnt], a)
            self.n += cnt
            t += cnt
            if self.n % B == 0:
                self._complete_block(j)
        return y


def render(x, h, max_len=None, ftz=False, block=None, splits=None, events=()):
    """y [V, C, T] of fresh convolvers fed x [V, C, T].  `splits`: lengths of the pieces to render in (default: one piece).
    `events`: [(S, "reset") | (S, h_new)] -- reset() / set_response(h_new) called before sample S."""
    x = np.asarray(x, dtype=f32)
    V, _, T = x.shape
    cv = Convolver(h, V, max_len=max_len, ftz=ftz, block=block)
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
    return np.concatenate(parts, axis=-1) if parts else np.zeros_like(x)
