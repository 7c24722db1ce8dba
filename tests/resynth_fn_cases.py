"""The closures the resynth_fn tests share: each as the C++ functor the library compiles and as the Python closure tests/resynth_fn_ref.py
runs.  Only operations whose f32 / f64 result IEEE fixes (add, subtract, multiply, comparisons, selects), so numpy gives the expected bits.
Every functor is loop-free."""
import numpy as np

f32 = np.float32


class Case:
    def __init__(self, functor, source, closure, inputs=1, outputs=1, params=0, state=0):
        self.functor, self.source, self.closure = functor, source, closure
        self.inputs, self.outputs, self.params, self.state = inputs, outputs, params, state

    def spec(self, N):
        return dict(window=N, functor=self.functor, source=self.source, inputs=self.inputs, outputs=self.outputs, state=self.state)


def _functor(name, params, state, body):
    return (f"struct {name} {{\n    static constexpr int PARAMS = {params}, STATE = {state};\n"
            f"    template <class W> static __device__ void bin(W& fft, int i) {{\n{body}\n    }}\n}};\n")


def stock(proc, N, I, O, src):
    """The stock processor `proc` with the source map `src` as a functor: band takes (lo, hi) per output as parameters 2o, 2o + 1, gain one
    value per output and bin as parameter o * bins + i."""
    NB = N // 2 + 1
    lines = []
    for o, s in enumerate(src):
        if s < 0:
            continue
        if proc == "pass":
            lines.append(f"        fft.set({o}, i, fft.at({s}, i));")
        elif proc == "band":
            lines.append(f"        if (fft.param({2 * o}) <= fft.frequency(i) && fft.frequency(i) <= fft.param({2 * o + 1})) fft.set({o}, i, fft.at({s}, i));")
        else:
            lines.append(f"        fft.set({o}, i, fft.at({s}, i) * fft.param({o * NB} + i));")
    P = {"pass": 0, "band": 2 * O, "gain": O * NB}[proc]

    def closure(fft):
        for o, s in enumerate(src):
            if s < 0:
                continue
            x = fft.at(s, fft.i)
            if proc == "pass":
                fft.set(o, x)
            elif proc == "band":
                fr = fft.frequency(fft.i)
                fft.set(o, x, where=(fft.param(2 * o) <= fr) & (fr <= fft.param(2 * o + 1)))
            else:
                fft.set(o, fft.op.cscale(x, fft.param_at(o * NB, fft.i)))

    name = f"Stock{proc.capitalize()}{N if proc == 'gain' else ''}x{I}x{O}x" + "".join("n" if s < 0 else str(s) for s in src)
    return Case(name, _functor(name, P, 0, "\n".join(lines)), closure, I, O, P)


def stock_params(proc, V, O, NB, band=None, gain=None):
    """the stock tables as the functor's parameter table [V, P] (None for pass)"""
    if proc == "band":
        return np.ascontiguousarray(np.broadcast_to(np.asarray(band, dtype=f32), (V, O, 2))).reshape(V, 2 * O)
    if proc == "gain":
        return np.ascontiguousarray(np.broadcast_to(np.asarray(gain, dtype=f32), (V, O, NB))).reshape(V, O * NB)
    return None


def _gate(fft):
    x = fft.at(0, fft.i)
    op = fft.op
    fft.set(0, x, where=op.add(op.mul(x[0], x[0]), op.mul(x[1], x[1])) >= fft.param(0))


GATE = Case("Gate", _functor("Gate", 1, 0, "        const Cf x = fft.at(0, i);\n"
                             "        if (x.re * x.re + x.im * x.im >= fft.param(0)) fft.set(0, i, x);"), _gate, params=1)


def _shift(fft):
    fft.set(0, fft.at(0, fft.i - fft.param(0).astype(np.int64)))


SHIFT = Case("Shift", _functor("Shift", 1, 0, "        fft.set(0, i, fft.at(0, i - (int)fft.param(0)));"), _shift, params=1)


def _cross(fft):
    fft.set(0, fft.op.cmul(fft.at(0, fft.i), fft.at(1, fft.i)))


CROSS = Case("Cross", _functor("Cross", 0, 0, "        fft.set(0, i, fft.at(0, i) * fft.at(1, i));"), _cross, inputs=2)


def _mid_side(fft):
    a, b, op = fft.at(0, fft.i), fft.at(1, fft.i), fft.op
    fft.set(0, op.cscale(op.cadd(a, b), f32(0.5)))
    fft.set(1, op.cscale(op.csub(a, b), f32(0.5)))


MID_SIDE = Case("MidSide", _functor("MidSide", 0, 0, "        const Cf a = fft.at(0, i), b = fft.at(1, i);\n"
                                    "        fft.set(0, i, (a + b) * 0.5f);\n        fft.set(1, i, (a - b) * 0.5f);"), _mid_side, inputs=2, outputs=2)


def _switch(fft):
    x = fft.at(0, fft.i)
    late = fft.time() >= fft.param(0).astype(np.float64)
    fft.set(0, x, where=late)
    fft.set(0, fft.op.cscale(x, f32(0.25)), where=~late)


SWITCH = Case("Switch", _functor("Switch", 1, 0, "        const Cf x = fft.at(0, i);\n"
                                 "        if (fft.time() >= (double)fft.param(0)) fft.set(0, i, x);\n        else fft.set(0, i, x * 0.25f);"), _switch, params=1)


def _smooth(fft):
    x, op, a = fft.at(0, fft.i), fft.op, fft.param(0)
    for s in (0, 1):
        fft.set_state(s, op.add(fft.state(s), op.mul(op.sub(x[s], fft.state(s)), a)))
    fft.set(0, (fft.state(0).copy(), fft.state(1).copy()))


SMOOTH = Case("Smooth", _functor("Smooth", 1, 2, "        const Cf x = fft.at(0, i);\n        const float a = fft.param(0);\n"
                                 "        fft.state(0) = fft.state(0) + (x.re - fft.state(0)) * a;\n"
                                 "        fft.state(1) = fft.state(1) + (x.im - fft.state(1)) * a;\n"
                                 "        fft.set(0, i, Cf{fft.state(0), fft.state(1)});"), _smooth, params=1, state=2)


def _foreign(fft):
    op = fft.op   # the writes to bin i + 1 and to channels 1 and -1 are dropped; the reads beyond the channels and the bins give zero
    fft.set(0, op.cadd(op.cadd(fft.at(0, fft.i), fft.at(3, fft.i)), fft.at(0, -1 - fft.i)))


FOREIGN = Case("Foreign", _functor("Foreign", 0, 0, "        fft.set(0, i + 1, Cf{1.0f, 1.0f});\n        fft.set(1, i, Cf{1.0f, 1.0f});\n"
                                   "        fft.set(-1, i, Cf{1.0f, 1.0f});\n        fft.set(0, i, fft.at(0, i) + fft.at(3, i) + fft.at(0, -1 - i));"), _foreign)

CLOSURES = dict(gate=GATE, shift=SHIFT, cross=CROSS, mid_side=MID_SIDE, switch=SWITCH, smooth=SMOOTH)


def case_params(name, V, N, seed=0):
    """per-instance parameters [V, P] of a closure case (None without parameters)"""
    rng = np.random.default_rng(seed + 50)
    if name == "gate":
        return rng.uniform(0.0, 0.02 * N, (V, 1)).astype(f32)
    if name == "shift":
        return rng.integers(-3, N // 2 + 3, (V, 1)).astype(f32)     # beyond both ends too
    if name == "switch":
        return rng.uniform(0.0, 3.0 * N / 44100.0, (V, 1)).astype(f32)
    if name == "smooth":
        return rng.uniform(0.05, 0.9, (V, 1)).astype(f32)
    return None
