"""numpy restatement of the resynthesizer banks' closure path (fundsp_amd/csrc/fd_resynth_fn.hpp), for the tests.

The forward and inverse transforms, the window and the overlap-add are tests/resynth_ref.py's; between them a Python per-bin closure runs
vectorised over instances, frames and bins, in explicit f32 / f64 steps: `closure(fft)` sees a `Window` whose `i` is the array of bin numbers
and whose methods mirror the device view (at, set, frequency, time, param, state).  A conditional of the C++ functor becomes `where=`.  With
`state > 0` the frames are walked in increasing order and the state [V, bins, state] is carried from one to the next.  `ftz=True` flushes
every f32 operand and result below 2^-126 like resynth_ref._Ops (f64 values are never flushed).
"""
import numpy as np

import resynth_ref as R

f32 = np.float32


class Ops(R._Ops):
    def div(self, a, b): return self.fl(self.fl(a) / self.fl(b))
    def sqrt(self, a): return self.fl(np.sqrt(self.fl(a)))

    def cmul(self, a, b):
        """Complex32 * Complex32: (a.re*b.re - a.im*b.im, a.re*b.im + a.im*b.re), every operation rounded"""
        return (self.sub(self.mul(a[0], b[0]), self.mul(a[1], b[1])), self.add(self.mul(a[0], b[1]), self.mul(a[1], b[0])))

    def cadd(self, a, b): return (self.add(a[0], b[0]), self.add(a[1], b[1]))
    def csub(self, a, b): return (self.sub(a[0], b[0]), self.sub(a[1], b[1]))
    def cscale(self, a, g): return (self.mul(a[0], g), self.mul(a[1], g))


class Window:
    """FftWindow for K frames of V instances at once.  Shapes broadcast to [V, K, bins]."""

    def __init__(self, N, Xr, Xi, O, params, state, samples, sr, op):
        self.N, self.op = N, op
        self.Xr, self.Xi = Xr, Xi                     # [V, K, I, bins]
        V, K, self.I, NB = Xr.shape
        self.O = O
        self.Yr = np.zeros((V, K, O, NB), dtype=f32)   # clear_output
        self.Yi = np.zeros_like(self.Yr)
        self.i = np.arange(NB)[None, None, :]
        self._p = params                              # [V, P] or None
        self._s = state                               # [V, bins, S] or None
        self._samples = np.asarray(samples, dtype=np.uint64)[None, :, None]   # [1, K, 1]: k H
        self._srf = f32(sr)                           # FftWindow::set_sample_rate(sample_rate as f32)

    def inputs(self): return self.I
    def outputs(self): return self.O
    def length(self): return self.N
    def bins(self): return self.N // 2 + 1

    def at(self, channel, j):
        """(re, im) of input bin j (an integer array, any values): zero out of range"""
        V, K, _, NB = self.Xr.shape
        if not 0 <= channel < self.I:
            z = np.zeros((V, K, NB), dtype=f32)
            return z, z.copy()
        j = np.broadcast_to(np.asarray(j, dtype=np.int64), (V, K, NB))
        ok = (j >= 0) & (j < NB)
        jc = np.clip(j, 0, NB - 1)
        re = np.take_along_axis(self.Xr[:, :, channel, :], jc, axis=2)
        im = np.take_along_axis(self.Xi[:, :, channel, :], jc, axis=2)
        return np.where(ok, re, f32(0.0)).astype(f32), np.where(ok, im, f32(0.0)).astype(f32)

    def set(self, channel, value, where=True):
        """fft.set(channel, i, value) for the calling bins `where` holds; a channel out of range is dropped"""
        if not 0 <= channel < self.O:
            return
        m = np.broadcast_to(where, self.Yr[:, :, channel, :].shape)
        self.Yr[:, :, channel, :] = np.where(m, np.asarray(value[0], dtype=f32), self.Yr[:, :, channel, :])
        self.Yi[:, :, channel, :] = np.where(m, np.asarray(value[1], dtype=f32), self.Yi[:, :, channel, :])

    def frequency(self, j):
        return (f32(self._srf / f32(self.N)) * np.asarray(j).astype(f32)).astype(f32)

    def sample_rate(self): return np.float64(self._srf)
    def latency(self): return np.float64(self.N) / np.float64(self._srf)
    def time(self): return (self._samples - np.uint64(self.N >> 1)).astype(np.float64) / np.float64(self._srf)
    def time_at(self, j): return (self._samples - np.uint64(self.N) + np.asarray(j).astype(np.uint64)).astype(np.float64) / np.float64(self._srf)
    def windows_per_second(self): return np.float64(4.0) * np.float64(self._srf) / np.float64(self.N)
    def delta_time(self): return np.float64(self.N) / (np.float64(4.0) * np.float64(self._srf))

    def param(self, p):
        """[V, 1, 1]; 0.0 out of range"""
        if self._p is None or not 0 <= p < self._p.shape[1]:
            return np.zeros((self.Xr.shape[0], 1, 1), dtype=f32)
        return self._p[:, p][:, None, None]

    def param_at(self, base, j):
        """fft.param(base + j) for a bin-number array j: [V, K, bins]"""
        idx = np.broadcast_to(base + np.asarray(j, dtype=np.int64), self.Yr[:, :, 0, :].shape)
        P = 0 if self._p is None else self._p.shape[1]
        ok = (idx >= 0) & (idx < P)
        if P == 0:
            return np.zeros(idx.shape, dtype=f32)
        v = np.take_along_axis(np.broadcast_to(self._p[:, None, :], idx.shape[:2] + (P,)), np.clip(idx, 0, P - 1), axis=2)
        return np.where(ok, v, f32(0.0)).astype(f32)

    def state(self, s): return self._s[:, :, s][:, None, :]            # [V, 1, bins] (one frame at a time)
    def set_state(self, s, value): self._s[:, :, s] = np.broadcast_to(np.asarray(value, dtype=f32), (self._s.shape[0], 1, self._s.shape[1]))[:, 0, :]


def overlap_add(frames, N, T, op, hz):
    """y [V, O, T] from frames [V, K, O, N], frame index k - 4: (((0 + a_w0) + a_w1) + a_w2) + a_w3, frame k in window (-k) mod 4"""
    V, _, O, _ = frames.shape
    H = N // 4
    y = np.zeros((V, O, T), dtype=f32)
    t = np.arange(T)
    m = t // H
    for w in range(4):
        k = m - ((m + w) % 4)
        live = k >= 4
        kk, tt = k[live], t[live]
        pos = tt - kk * H
        a = op.mul(frames[:, kk - 4, :, pos], hz[pos][:, None, None])
        y[:, :, live] = op.add(y[:, :, live], np.transpose(a, (1, 2, 0)))
    return y


def render(x, N, closure, outputs=1, params=None, state=0, sample_rate=44100.0, changes=(), ftz=False, cosf=None, tabs=None):
    """y [V, O, T] of V fresh closure resynthesizers fed x [V, I, T].

    params: [P] or [V, P]; `changes`: [(S, dict(sample_rate=.., params=..))] -- a setter called before sample S: it applies to the frames that
    complete at sample counts k H > S."""
    x = np.asarray(x, dtype=f32)
    V, I, T = x.shape
    O, H, NB = int(outputs), N // 4, N // 2 + 1
    op = Ops(ftz)
    hann, tw = tabs if tabs is not None else R.tables(N, cosf)
    hz = (hann * f32(f32(2.0) / f32(3.0))).astype(f32)

    def table(p):
        return None if p is None else np.ascontiguousarray(np.broadcast_to(np.asarray(p, dtype=f32), (V, np.shape(p)[-1])))

    segs = [(-1, dict(sample_rate=sample_rate, params=params))]
    for S, upd in sorted(changes, key=lambda c: c[0]):
        p = dict(segs[-1][1])
        p.update(upd)
        segs.append((S, p))
    ks = np.arange(4, T // H + 1)
    ks = ks[ks * H < T]
    frames = np.zeros((V, len(ks), O, N), dtype=f32)
    st = np.zeros((V, NB, state), dtype=f32) if state > 0 else None
    for si, (S, p) in enumerate(segs):
        S_next = segs[si + 1][0] if si + 1 < len(segs) else None
        sel = np.nonzero((ks * H > S) & ((ks * H <= S_next) if S_next is not None else True))[0]
        if len(sel) == 0:
            continue
        idx = (ks[sel] * H - N)[:, None] + np.arange(N)[None, :]
        Xr, Xi = R.rfft(op.mul(x[:, :, idx], hann), tw, op)             # [V, I, K, bins]
        Xr, Xi = np.ascontiguousarray(Xr.transpose(0, 2, 1, 3)), np.ascontiguousarray(Xi.transpose(0, 2, 1, 3))
        groups = [slice(a, a + 1) for a in range(len(sel))] if state > 0 else [slice(0, len(sel))]
        for g in groups:
            w = Window(N, Xr[:, g], Xi[:, g], O, table(p["params"]), st, ks[sel][g] * H, p["sample_rate"], op)
            closure(w)
            for o in range(O):
                frames[:, sel[g], o, :] = R.irfft_re(w.Yr[:, :, o, :], w.Yi[:, :, o, :], tw, op)
    return overlap_add(frames, N, T, op, hz)
