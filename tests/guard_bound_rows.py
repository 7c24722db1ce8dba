"""The edge rows of the guard-bound tests: one FM voice each -- f, m, fc, q, the two sines' initial phases, the filter's preset
state, and whether that state is preset.  The same list as edge_rows() of tests/host/check_guard_bounds.hip, value for value
(tests/test_guard_bounds_host.py compares the bit patterns), for the banks of tests/test_gpu_guard_bounds.py."""
import numpy as np

F = np.float32


def edge_rows():
    sr = F(48000.0)
    inf = F(np.inf)
    rows = []

    def turns(t):  # the frequency whose 64-frame block sweeps t turns of phase
        return F(F(F(t) * sr) / F(64.0))

    def row(f, m, fc, q, ph_mod, ph_car, ic1, ic2, preset):
        rows.append((F(f), F(m), F(fc), F(q), F(ph_mod), F(ph_car), F(ic1), F(ic2), bool(preset)))

    for t in (2040.0, 2046.0, 2046.9, 2047.0, 2047.1, 2047.9, 2048.0, 2048.1, 2050.0, -2046.9, -2047.1, -2050.0):
        row(turns(t), 0.0, 1000.0, 1.0, 0.0, 0.0, 0.0, 0.0, False)
    for fm in (turns(2046.0) / F(16.0), turns(2048.0) / F(16.0), turns(1000.0), turns(2040.0)):
        row(1000.0, F(fm) / F(1000.0), 2000.0, 0.7, 0.25, 0.5, 0.0, 0.0, False)
    row(100.0, 1.0e6, 500.0, 2.0, 0.0, 0.0, 0.0, 0.0, False)
    row(1000.0, 500.0, 500.0, 2.0, 0.0, 0.0, 0.0, 0.0, False)
    for ph in (3000.0, -0.0, 0.0, 2046.5, -3000.0):
        for which in (0, 1):
            row(440.0, 2.0, 1200.0, 1.0, 0.125 if which else ph, ph if which else 0.125, 0.0, 0.0, False)
    row(-440.0, 2.0, 1200.0, 1.0, 0.3, 0.6, 0.0, 0.0, False)
    row(440.0, -3.0, 1200.0, 1.0, 0.3, 0.6, 0.0, 0.0, False)
    row(-1760.0, -7.9, 5000.0, 3.0, 0.9, 0.1, 0.0, 0.0, False)
    top95 = np.array([0x6F7FFFFF], dtype=np.uint32).view(F)[0]   # 0x1.fffffep95
    top127 = np.array([0x7F7FFFFF], dtype=np.uint32).view(F)[0]  # 0x1.fffffep127
    p = lambda e: F(2.0) ** F(e)
    for s in (p(95), p(96), p(97), p(126), p(127), -p(95), -p(96), -p(97), -p(126), -p(127), inf, -inf, F(np.nan), top95, top127):
        for which in (0, 1):
            row(220.0, 1.5, 800.0, 0.8, 0.2, 0.4, 0.0 if which else s, s if which else 0.0, True)
    row(220.0, 1.5, 800.0, 0.8, 0.2, 0.4, 0.0, -0.0, True)
    row(220.0, 1.5, 800.0, 0.8, 0.2, 0.4, p(120), -p(120), True)
    for fc in (30000.0, 47000.0, 23999.0, 24001.0, 71000.0):
        for q in (1.0, 1.0e-30, 1.0e30):
            row(330.0, 1.0, fc, q, 0.1, 0.2, 0.0, 0.0, False)
            row(330.0, 1.0, fc, q, 0.1, 0.2, p(90), -p(60), True)
    row(330.0, 1.0, 1000.0, 1.0e-30, 0.1, 0.2, 0.0, 0.0, False)
    row(330.0, 1.0, 1000.0, 1.0e30, 0.1, 0.2, 0.0, 0.0, False)
    return rows


def row_bits(r):
    """The row as check_guard_bounds --rows prints it (NaN by its being a NaN: the payload is the platform's)."""
    return tuple("nan" if np.isnan(x) else "%08x" % np.array([x], dtype=F).view(np.uint32)[0] for x in r[:8]) + (int(r[8]),)
