// tests/host/svf_par_dump.cpp -- fd_svf_par.hpp alone, host compiler (-O2 -ffp-contract=off): writes out what the header computes so
// that tests/test_svf_par_ref.py can compare the numpy restatement (tests/svf_par_ref.py) with it bit for bit.
//   svf_par_dump block IN OUT   IN:  int32 V, T, LC; float co[V][6] (a1 a2 a3 m0 m1 m2); float s[V][2]; float x[V][T]     (T % 64 == 0)
//                               OUT: float y[V][T]; float s[V][2] (the end state); float tables[V][2 LC + 4] (rx[LC] ry[LC] p00 p01 p10 p11)
//                               one launch per voice: svfp_tables<LC>, then svfp_block<LC> block after block; LC = 32 or 16
//   svf_par_dump fma IN OUT     IN:  int32 N; float a[N], b[N], c[N]      OUT: float __builtin_fmaf(a, b, c)[N]
#include <cstdio>
#include <cstring>
#include <vector>
#include "fd_svf_par.hpp"
using namespace fd;

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

template <int LC>
static void run(int V, int T, const std::vector<float>& co, std::vector<float>& s, const std::vector<float>& x, std::vector<float>& y,
                std::vector<float>& tb) {
    constexpr int W = 2 * LC + 4;
    tb.resize((size_t)V * W);
    for (int v = 0; v < V; v++) {
        const SvfpCoefs k{co[v * 6], co[v * 6 + 1], co[v * 6 + 2], co[v * 6 + 3], co[v * 6 + 4], co[v * 6 + 5]};
        SvfpTables<LC> t;
        svfp_tables<LC>(k, t);
        float* q = &tb[(size_t)v * W];
        for (int n = 0; n < LC; n++) q[n] = t.rx[n], q[LC + n] = t.ry[n];
        q[2 * LC] = t.p00, q[2 * LC + 1] = t.p01, q[2 * LC + 2] = t.p10, q[2 * LC + 3] = t.p11;
        for (int t0 = 0; t0 < T; t0 += 64) svfp_block<LC>(k, t, &x[(size_t)v * T + t0], &y[(size_t)v * T + t0], s[v * 2], s[v * 2 + 1]);
    }
}

int main(int argc, char** argv) {
    if (argc != 4) return fprintf(stderr, "usage: svf_par_dump block|fma IN OUT\n"), 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return perror(argv[2]), 2;
    std::vector<float> out;
    if (!strcmp(argv[1], "fma")) {
        int n = 0;
        if (!rd(f, &n, 1) || n < 0) return fprintf(stderr, "bad header\n"), 2;
        std::vector<float> a(n), b(n), c(n);
        if (!rd(f, a.data(), n) || !rd(f, b.data(), n) || !rd(f, c.data(), n)) return fprintf(stderr, "short input\n"), 2;
        out.resize(n);
        for (int i = 0; i < n; i++) out[i] = __builtin_fmaf(a[i], b[i], c[i]);
    } else if (!strcmp(argv[1], "block")) {
        int h[3] = {0, 0, 0};
        if (!rd(f, h, 3) || h[0] < 0 || h[1] < 0 || h[1] % 64 || (h[2] != 32 && h[2] != 16)) return fprintf(stderr, "bad header\n"), 2;
        const int V = h[0], T = h[1];
        std::vector<float> co((size_t)V * 6), s((size_t)V * 2), x((size_t)V * T), y((size_t)V * T), tb;
        if (!rd(f, co.data(), co.size()) || !rd(f, s.data(), s.size()) || !rd(f, x.data(), x.size())) return fprintf(stderr, "short input\n"), 2;
        if (h[2] == 32) run<32>(V, T, co, s, x, y, tb); else run<16>(V, T, co, s, x, y, tb);
        out = y;
        out.insert(out.end(), s.begin(), s.end());
        out.insert(out.end(), tb.begin(), tb.end());
    } else {
        return fprintf(stderr, "unknown mode %s\n", argv[1]), 2;
    }
    fclose(f);
    f = fopen(argv[3], "wb");
    if (!f) return perror(argv[3]), 2;
    const bool ok = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 2;
}
