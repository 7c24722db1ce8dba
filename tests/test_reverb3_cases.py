"""The tables of reverb3_cases.py claim what is true -- checked on the host, so that an edit which thins them fails where every change is
tested, not only on a GPU: the rate table against the restated delay arithmetic, the restatement against rv3_make_const itself
(tests/host/check_reverb3_const.hip, built for the host: no kernel, no device), and every property the cuts are there for."""
import os
import shutil
import subprocess

import pytest

import reverb3_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (512, 1024, 2048, 4096, 8192, 16384)


def test_rate_table_rows_hold_what_they_claim():
    for rate, shortest, longest, cap, why in K.RATES:
        c = K.make_const(rate)
        assert c["ok"] and (c["shortest"], c["longest"], c["cap"]) == (shortest, longest, cap), (rate, c["shortest"], c["longest"], c.get("cap"))
        assert c["ring_stride"] == 72 * (cap + 64) and len(c["all"]) == 72
        assert cap // 2 - 64 < longest <= cap - 64 and shortest >= K.SHORTEST_LEGAL
        assert c["dblk"][0] == longest and K.short_line(c) == shortest         # L_long is block 0's delay, L_short an allpass line
        if why == K.FULL:
            assert longest == cap - 64
            assert K.make_const(rate + 40.0)["cap"] == 2 * cap                  # ... and the step is right behind it
        elif why == K.FIRST:
            assert longest == cap // 2 - 63
        elif why == K.FLOOR:
            assert shortest == K.SHORTEST_LEGAL
        else:
            assert why == K.PLAIN
    assert sorted({r[3] for r in K.RATES}) == list(CAPS)
    assert sorted(r[3] for r in K.FULL_RATES) == list(CAPS)                     # every capacity has its full ring ...
    assert sorted(r[3] for r in K.RATES if r[4] == K.FIRST) == list(CAPS[1:5])  # ... and 1024 .. 8192 their emptiest
    assert {r[0] for r in K.EDGE_RATES} == {r[0] for r in K.FULL_RATES} | {K.ACCEPTED_LOW}
    assert any(r[3] == 1024 for r in K.FULL_RATES)                              # the staging case's row


def test_refusal_boundaries():
    low, ok, high = K.make_const(K.REFUSED_LOW), K.make_const(K.ACCEPTED_LOW), K.make_const(K.REFUSED_HIGH)
    assert not low["ok"] and low["shortest"] == 128 and low["longest"] <= K.LONGEST_LEGAL       # refused for the shortest line alone
    assert ok["ok"] and ok["shortest"] == 129 and K.ACCEPTED_LOW == K.REFUSED_LOW + 1.0
    assert not high["ok"] and high["shortest"] > 128 and high["longest"] > K.LONGEST_LEGAL      # ... and for the longest alone
    # the largest ring that is accepted keeps every byte offset of the kernel below 2^31 (32-bit offsets into a buffer resource of
    # ring_stride * 4 bytes): (71 * CP + cap + 63) * 4 with cap = 2^21
    cap = 256
    while cap < K.LONGEST_LEGAL + 64:
        cap <<= 1
    assert cap == 1 << 21 and 72 * (cap + 64) * 4 < 2 ** 31


def test_cuts_place_every_edge():
    for rate, _, longest, cap, _ in K.RATES:
        c = K.make_const(rate)
        cs = K.cuts(c)
        T = K.total(cap)
        assert cs[0] == 0 and cs[-1] == T == 3 * cap + 64 * 3 + 13 and all(a < e for a, e in K.launches(cs)), (rate, cs)
        ls = K.launches(cs)
        # a ragged launch ending at cap - 91; a launch beginning at cap - 10, whose window straddles the wrap
        assert any(e == cap - 91 and (e - a) % 64 for a, e in ls)
        assert any(a == cap - 10 and e > cap for a, e in ls)
        # a launch beginning at wp == 37 with a full block there: lanes 0 .. 26 write the mirror, the others do not
        assert any(a % cap == 37 and e - a >= 64 for a, e in ls)
        # a launch beginning at wp == 64 that runs aligned through the block at wp == cap - 64
        assert any(a % cap == 64 and e - a >= cap - 64 for a, e in ls)
        bl = K.blocks(cs, cap)
        wide = {wp for t, wp, size in bl if K.is_wide(wp, size, cap, t % 512)}
        slow = {wp for t, wp, size in bl if not K.is_wide(wp, size, cap, t % 512)}
        assert {64, cap - 64} <= wide and any(wp % 64 for wp in wide)          # the first and the last wide block, and one off the grid
        assert any(wp + 64 > cap for wp in slow) and any(0 < wp < 64 for wp in slow)
        if cap > 512:   # the two halves of the wide condition disagree: the main ring's window is fine, the pre ring's wraps
            assert any(64 <= wp <= cap - 64 and size == 64 and not 64 <= t % 512 <= 448 for t, wp, size in bl)
        # for the longest line and the shortest allpass line: a launch whose first block is full and reads from slot cap - 1 on,
        # through the whole mirror, samples that were written (not the ring's initial zeros)
        for d in (c["dblk"][0], K.short_line(c)):
            hit = [(a, e) for a, e in ls if (a - d) % cap == cap - 1 and e - a >= 64]
            assert hit and all(a - d >= cap - 1 for a, e in hit), (rate, d, cs)
        # three launches shorter than a block in a row
        sizes = [e - a for a, e in ls]
        assert any(sizes[i:i + 3] == [1, 1, 62] for i in range(len(sizes)))
        # before the last launch every line has been read from a slot written after the ring's first wrap
        last = cs[-2]
        assert all(last - 1 - d >= cap for d in c["all"]), (rate, last)
        assert T // 2 < last                                                    # (the noise stops before it: the last launch is all tail)
        # after reset(): cap + 100 frames, the pre rings' write position keeps the phase the first render left (T mod 512 = 205)
        rs = K.reset_cuts(cap)
        assert rs[0] == 0 and rs[-1] == cap + 100 and T % 512 == 205
        rb = [(wp, size, (T + t) % 512) for t, wp, size in K.blocks(rs, cap)]
        assert any(K.is_wide(wp, size, cap) and not K.is_wide(wp, size, cap, wq) for wp, size, wq in rb)   # main ring wide, pre ring not
        assert any(K.is_wide(wp, size, cap, wq) for wp, size, wq in rb)


def test_rate_change_pairs_and_stops():
    seen = set()
    for a, b in K.MIGRATE_PAIRS:
        ca, cb = K.make_const(a), K.make_const(b)
        assert ca["ok"] and cb["ok"] and ca["cap"] != cb["cap"]                 # from.cap != to.cap: a swapped mask or stride shows
        seen.add(ca["cap"] < cb["cap"])
        stops = {s: K.first_render(s, ca["cap"]) for s in K.STOPS}
        assert stops["unaligned"] > 2 * ca["cap"] and stops["unaligned"] % 64
        assert stops["unaligned"] % ca["cap"] < ca["shortest"]                  # wold < every d: each old read reaches back across the wrap
        assert stops["wold0"] == 2 * ca["cap"] and stops["wold0"] % ca["cap"] == 0
        assert stops["early"] == 70 < ca["shortest"]
        ac = K.after_cuts(cb)
        assert ac[1] >= 64 and ac[1] % 64 and ac[-1] > cb["cap"] + 64 and ac[-1] > cb["longest"]
        # the feedback sample (slot cap - 1 of block 0's delay ring) has crossed all eight block delays, with a ring's worth to spare
        assert K.loop_trip(cb) == sum(cb["dblk"]) > 8 * cb["shortest"] and ac[-1] >= K.loop_trip(cb) + cb["cap"]
    assert seen == {True, False}                                                # into a larger and into a smaller ring
    assert [(K.make_const(a)["cap"], K.make_const(b)["cap"]) for a, b in K.MIGRATE_PAIRS] == [(2048, 512), (512, 4096), (4096, 512), (2048, 512)]
    full = K.make_const(K.MIGRATE_PAIRS[2][1])
    assert full["longest"] == full["cap"] - 64                                  # 96 000 -> 17 554: into a full ring
    # half a hertz down: the same 72 distances at another rate.  Half a hertz UP is not that: two lines grow by a sample
    a, up, down = (K.make_const(s)["all"] for s in (48000.0, 48000.5, 47999.5))
    assert down == a and sorted(y - x for x, y in zip(a, up)) == [0] * 70 + [1, 1]
    assert K.make_const(22050.0)["cap"] == 1024                                 # the from_graph case's ring
    # at the diffusion of these cases the direct way round the loop keeps a moved sample far above the rounding of the tail (2^-24)
    eta, a = 0.5 * (1.0 - K.DIFFUSION_MOVED) + 0.9 * K.DIFFUSION_MOVED, 0.001 ** (0.035 / 2.0)
    assert (a * eta ** 8) ** 8 > 2.0 ** -24 * 1000


@pytest.fixture(scope="module")
def host_rows(tmp_path_factory):
    """{rate: (ok, cap, stride, dap0, dap1, dblk)} as rv3_make_const gives them"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("reverb3_const") / "check_reverb3_const"
    cmd = [hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unused-result",
           "-I", os.path.join(ROOT, "fundsp_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "host", "check_reverb3_const.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)] + [repr(s) for s in K.HOST_RATES], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    rows = {}
    for i in range(0, len(K.HOST_RATES) * 4, 4):
        w = lines[i].split()
        assert w[0] == "rate" and w[2] == "ok" and w[4] == "cap" and w[6] == "stride", lines[i]
        d = [[int(x) for x in lines[i + k].split()[1:]] for k in (1, 2, 3)]
        assert [lines[i + k].split()[0] for k in (1, 2, 3)] == ["dap0", "dap1", "dblk"]
        rows[float(w[1])] = (int(w[3]), int(w[5]), int(w[7]), d[0], d[1], d[2])
    return rows


def test_restatement_equals_rv3_make_const(host_rows):
    assert sorted(host_rows) == K.HOST_RATES
    assert {r[0] for r in K.RATES} | {K.REFUSED_LOW, K.REFUSED_HIGH} <= set(host_rows)
    for sr, (ok, cap, stride, dap0, dap1, dblk) in host_rows.items():
        c = K.make_const(sr)
        assert bool(ok) == c["ok"], sr
        # (a refused rate has its distances filled in up to the decision: all of them)
        assert dap0 == [d for row in c["dap0"] for d in row], sr
        assert dap1 == [d for row in c["dap1"] for d in row], sr
        assert dblk == c["dblk"], sr
        if ok:
            assert (cap, stride) == (c["cap"], c["ring_stride"]), sr
        else:
            assert (cap, stride) == (0, 0), sr
    assert not host_rows[K.REFUSED_LOW][0] and not host_rows[K.REFUSED_HIGH][0] and host_rows[K.ACCEPTED_LOW][0]
