// check_line_table.hip -- host: the per-line table filler of the line networks (fundsp_amd/csrc/fd_line_table.hpp) for both row types, on
// ordinary descriptions and on delays whose sample count passes 2^18 or has no `int` value.  No kernel, no device; built for the host
// (also under the undefined-behaviour sanitizer: the sample count must be refused before it is converted).  Prints "bad <n>".
#include <cmath>
#include <cstdio>

#include "fd_fbdelay.hpp"
#include "fd_line_table.hpp"

using namespace fd;

static int bad = 0;
#define CHECK(x) do { if (!(x)) { bad++; std::printf("line %d: %s\n", __LINE__, #x); } } while (0)

template <class Row>
static void family(int N) {
    const double sr = 48000.0;
    FdnxDesc d;
    d.lines = N; d.taps = 2; d.per_instance = 1; d.has_gain = 1; d.filter = FDNX_LOWPOLE;
    const size_t V = 3, M = V * N;
    for (size_t i = 0; i < M; i++) {
        d.delay.push_back(0.003 + 0.0011 * (double)i);
        d.w.push_back(0.5f + (float)i); d.w.push_back(0.25f + (float)i);
        d.cutoff.push_back(500.0f + 100.0f * (float)i);
        d.q.push_back(0.7f); d.gain.push_back(2.0f);
        d.line_gain.push_back(0.5f - 0.01f * (float)i);
    }
    std::vector<Row> tab;
    LineSpan s = line_table_fill(d, V, sr, tab);
    CHECK(tab.size() == V);
    int lo = 1 << 30, hi = 0;
    for (size_t p = 0; p < V; p++)
        for (int k = 0; k < N; k++) {
            const size_t i = p * N + k;
            const int len = (int)std::round(d.delay[i] * sr) + 1;
            lo = len < lo ? len : lo; hi = len > hi ? len : hi;
            CHECK(tab[p].len[k] == len);
            CHECK(tab[p].w[0][k] == d.w[2 * i] && tab[p].w[1][k] == d.w[2 * i + 1] && tab[p].w[2][k] == 0.0f);
            CHECK(tab[p].co[0][k] > 0.0f && tab[p].co[0][k] < 1.0f && tab[p].co[1][k] == 1.0f - tab[p].co[0][k]);
            CHECK(tab[p].g[k] == d.line_gain[i]);
        }
    CHECK(s.shortest == lo && s.longest == hi);
    const int cap = line_ring_cap(hi);
    CHECK(cap >= 256 && (cap & (cap - 1)) == 0 && cap >= hi && (cap == 256 || cap / 2 < hi));
    // one row for the bank, a FixedSvf, no gain node: g = 1
    d.per_instance = 0; d.has_gain = 0; d.filter = FDNX_SVF; d.svf_mode = 6;
    s = line_table_fill(d, V, sr, tab);
    CHECK(tab.size() == 1 && s.shortest > 0);
    for (int k = 0; k < N; k++) {
        const SvfCoefs c = svf_coefs(6, (float)sr, d.cutoff[k], d.q[k], d.gain[k]);
        CHECK(tab[0].co[0][k] == c.a1 && tab[0].co[3][k] == c.m0 && tab[0].co[5][k] == c.m2 && tab[0].g[k] == 1.0f);
    }
    // the ring limit: 2^18 - 1 samples is the longest delay; beyond it the fill is refused before any conversion to int
    d.filter = FDNX_NONE; d.taps = 0;
    d.delay[N - 1] = (double)((1 << 18) - 1) / sr;
    s = line_table_fill(d, V, sr, tab);
    CHECK(s.longest == (1 << 18) && line_ring_cap(s.longest) == (1 << 18) && tab[0].len[N - 1] == (1 << 18));
    const double too_long[] = {(double)(1 << 18) / sr, 1e5, 999999.0, 2147483647.0 / sr, 2147483648.0 / sr, 1e300};
    for (double t : too_long) {
        d.delay[N - 1] = t;
        CHECK(line_table_fill(d, V, sr, tab).shortest < 0);
        CHECK(line_table_fill(d, V, 192000.0, tab).shortest < 0);
    }
    d.delay[N - 1] = std::nan("");
    CHECK(line_table_fill(d, V, sr, tab).shortest < 0);
}

int main() {
    family<FdnxInst>(2);
    family<FdnxInst>(32);
    family<FbInst>(1);
    family<FbInst>(2);
    std::printf("bad %d\n", bad);
    return bad != 0;
}
