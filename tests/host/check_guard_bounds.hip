// tests/host/check_guard_bounds.hip -- host-side check (hipcc, host only) of the packed-path guards that are decided per
// block / per item from a producer's output bound (fd_nodes.hpp: OutBound, SineB, FixedSvfB / FixedSvfLpB, HoistOf).
// FmSvf and SineHzLowpass are driven the way pipe_stage drives a stage: begin_block, the tile snapshot, item_begin every 8
// frames, step2<PH_SIMD>, tripped(), the scalar re-render, end_simd, the remainder -- as HoistOf<G>, HoistOf<LpOf<G>> and
// (today's per-frame guards) G itself -- and compared bit for bit (NaN == NaN) with the plain step() rendering and, where
// the filter starts from rest, with the oracle's process().
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#define FD_HOST_ONLY 1
#include "fd_nodes.hpp"
extern "C" {
#include "fundsp_oracle.h"
}
using namespace fd;
using SineHz = Pipe<Constant<1>, Sine>;
using SineHzLowpass = Pipe<SineHz, FixedSvf>;
using FmMod = Unop<Unop<Unop<SineHz, UMulScalar>, UMulScalar>, UAddScalar>;
using FmSvf = Pipe<Pipe<FmMod, Sine>, FixedSvf>;
using FmSvfB = HoistOf<FmSvf>::type;
using FmSvfLB = HoistOf<LpOf<FmSvf>::type>::type;
using ShlB = HoistOf<SineHzLowpass>::type;
using ShlLB = HoistOf<LpOf<SineHzLowpass>::type>::type;
// the bounded forms are really chosen for the two headline graphs, and only behind a producer that states a bound
static_assert(SameType<FmSvfB, Pipe<Pipe<Unop<Unop<Unop<Pipe<Constant<1>, SineB>, UMulScalar>, UMulScalar>, UAddScalar>, SineB>, FixedSvfB>>::v, "FmSvf hoists both sines and the filter");
static_assert(SameType<FmSvfLB, Pipe<Pipe<Unop<Unop<Unop<Pipe<Constant<1>, SineB>, UMulScalar>, UMulScalar>, UAddScalar>, SineB>, FixedSvfLpB>>::v, "... and the lowpass twin");
static_assert(SameType<ShlB, Pipe<Pipe<Constant<1>, SineB>, FixedSvfB>>::v, "SineHzLowpass hoists");
static_assert(SameType<HoistOf<Pipe<Pass, Sine>>::type, Pipe<Pass, Sine>>::v && SameType<HoistOf<Pipe<Pipe<Pass, Sine>, FixedSvf>>::type, Pipe<Pipe<Pass, Sine>, FixedSvfB>>::v &&
              SameType<HoistOf<Pipe<Noise, FixedSvf>>::type, Pipe<Noise, FixedSvf>>::v && SameType<HoistOf<Sine>::type, Sine>::v && SameType<HoistOf<FixedSvf>::type, FixedSvf>::v,
              "a Sine / FixedSvf fed from an input stream or from a producer without a bound keeps its per-frame guard");
static_assert(sizeof(FmSvfB) == sizeof(FmSvf) && sizeof(FmSvfLB) == sizeof(FmSvf) && sizeof(ShlB) == sizeof(SineHzLowpass), "layout-identical twins");

static bool same(float a, float b) { return (a != a && b != b) || f2u(a) == f2u(b); }

// what pipe_stage does with one stage that holds the whole graph (tiles of SUB frames inside 64-frame blocks)
template <class G>
static unsigned long render_packed(G& g, int T, int SUB, std::vector<float>& y) {
    unsigned long trips = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int size = T - t0 < 64 ? T - t0 : 64, full = size & ~7;
        for (int h = 0; h * SUB < size; h++) {
            const int lo = h * SUB, hi = lo + SUB < size ? lo + SUB : size, shi = hi < full ? hi : full;
            if (h == 0) g.begin_block(size);
            if (lo < shi) {
                const G snap = g;
                for (int i8 = lo; i8 < shi; i8 += 8) {
                    item_begin(g);
                    for (int i = i8; i < i8 + 8; i += 2) {
                        v2f in{0.0f, 0.0f}, o;
                        g.template step2<PH_SIMD>(&in, &o);
                        y[t0 + i] = o.x;
                        y[t0 + i + 1] = o.y;
                    }
                }
                if (g.tripped()) {
                    trips++;
                    g = snap;
                    for (int i = lo; i < shi; i++) g.template step<PH_SIMD>(nullptr, &y[t0 + i]);
                }
            }
            if (h == (full == 0 ? 0 : (full - 1) / SUB)) g.end_simd();
            for (int i = lo > full ? lo : full; i < hi; i++) g.template step<PH_REM>(nullptr, &y[t0 + i]);
        }
    }
    return trips;
}
template <class G>
static void render_plain(G& g, int T, std::vector<float>& y) {
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int size = T - t0 < 64 ? T - t0 : 64, full = size & ~7;
        g.begin_block(size);
        for (int i = 0; i < full; i++) g.template step<PH_SIMD>(nullptr, &y[t0 + i]);
        g.end_simd();
        for (int i = full; i < size; i++) g.template step<PH_REM>(nullptr, &y[t0 + i]);
    }
}

struct Row {  // one voice: parameters and preset state
    float f, m, fc, q, ph_mod, ph_car, ic1, ic2;
    bool preset;  // the filter state is preset (no oracle comparison: the oracle's filter starts from rest)
};
static FmSvf make_fm(const Row& r, double sr) {
    FmSvf g;
    Ctx ctx{};
    g.init();
    g.x.x.x.x.x.x.value[0] = r.f;
    g.x.x.x.x.scalar = r.f;
    g.x.x.x.scalar = r.m;
    g.x.x.scalar = r.f;
    Sine& mod = g.x.x.x.x.x.y;
    mod.has_phase = 1.0f; mod.initial_phase = r.ph_mod;
    g.x.y.has_phase = 1.0f; g.x.y.initial_phase = r.ph_car;
    g.y.cutoff = r.fc; g.y.q = r.q;
    g.update(sr);
    g.reset();
    g.bind(ctx);
    g.y.c.ic1eq = r.ic1; g.y.c.ic2eq = r.ic2;
    return g;
}
static SineHzLowpass make_shl(const Row& r, double sr) {
    SineHzLowpass g;
    Ctx ctx{};
    g.init();
    g.x.x.value[0] = r.f;
    g.x.y.has_phase = 1.0f; g.x.y.initial_phase = r.ph_car;
    g.y.cutoff = r.fc; g.y.q = r.q;
    g.update(sr);
    g.reset();
    g.bind(ctx);
    g.y.c.ic1eq = r.ic1; g.y.c.ic2eq = r.ic2;
    return g;
}
static void oracle_fm(const Row& r, double sr, int T, std::vector<float>& y) {
    onode* mod = o_sine();
    o_sine_set_phase(mod, r.ph_mod);
    onode* car = o_sine();
    o_sine_set_phase(car, r.ph_car);
    onode* fm = o_unop(O_ADD_SCALAR, o_unop(O_MUL_SCALAR, o_unop(O_MUL_SCALAR, o_pipe(o_constant(1, &r.f), mod), r.f), r.m), r.f);
    onode* n = o_pipe(o_pipe(fm, car), o_fixed_svf(O_SVF_LOWPASS, r.fc, r.q, 1.0f));
    o_set_sample_rate(n, sr);
    o_render_blocks(n, (size_t)T, 64, nullptr, y.data());
    o_free(n);
}
static void oracle_shl(const Row& r, double sr, int T, std::vector<float>& y) {
    onode* car = o_sine();
    o_sine_set_phase(car, r.ph_car);
    onode* n = o_pipe(o_pipe(o_constant(1, &r.f), car), o_fixed_svf(O_SVF_LOWPASS, r.fc, r.q, 1.0f));
    o_set_sample_rate(n, sr);
    o_render_blocks(n, (size_t)T, 64, nullptr, y.data());
    o_free(n);
}

static unsigned long long bad = 0;
static void compare(const char* what, int row, const std::vector<float>& got, const std::vector<float>& want) {
    for (size_t i = 0; i < want.size(); i++)
        if (!same(got[i], want[i])) {
            if (bad < 12) printf("%s: row %d frame %zu got %a want %a\n", what, row, i, got[i], want[i]);
            bad++;
            return;
        }
}
template <class GV, class G>
static unsigned long run_variant(const char* what, int row, const G& g0, int T, int SUB, const std::vector<float>& want, GV* end = nullptr) {
    GV v;
    memcpy((void*)&v, (const void*)&g0, sizeof g0);
    std::vector<float> y(T);
    const unsigned long trips = render_packed(v, T, SUB, y);
    compare(what, row, y, want);
    if (end) *end = v;
    return trips;
}
// every form of one FmSvf voice against the plain rendering (and the oracle); returns the tiles the bounded form re-rendered
static unsigned long check_fm(const Row& r, int row, int T, double sr, FmSvfB* end = nullptr) {
    const FmSvf g0 = make_fm(r, sr);
    std::vector<float> want(T), orc(T);
    FmSvf p = g0;
    render_plain(p, T, want);
    if (!r.preset) { oracle_fm(r, sr, T, orc); compare("fm plain vs oracle", row, want, orc); }
    unsigned long trips = 0;
    for (int SUB : {64, 32, 8}) {
        run_variant<FmSvf>("fm per-frame guards", row, g0, T, SUB, want);
        trips += run_variant<FmSvfB>("fm bounded", row, g0, T, SUB, want, SUB == 64 ? end : nullptr);
        if (lp_ok(g0)) {
            run_variant<LpOf<FmSvf>::type>("fm lowpass per-frame guards", row, g0, T, SUB, want);
            trips += run_variant<FmSvfLB>("fm lowpass bounded", row, g0, T, SUB, want);
        }
    }
    return trips;
}
static unsigned long check_shl(const Row& r, int row, int T, double sr, ShlB* end = nullptr) {
    const SineHzLowpass g0 = make_shl(r, sr);
    std::vector<float> want(T), orc(T);
    SineHzLowpass p = g0;
    render_plain(p, T, want);
    if (!r.preset) { oracle_shl(r, sr, T, orc); compare("shl plain vs oracle", row, want, orc); }
    unsigned long trips = 0;
    for (int SUB : {64, 16}) {
        run_variant<SineHzLowpass>("shl per-frame guards", row, g0, T, SUB, want);
        trips += run_variant<ShlB>("shl bounded", row, g0, T, SUB, want, SUB == 64 ? end : nullptr);
        if (lp_ok(g0)) trips += run_variant<ShlLB>("shl lowpass bounded", row, g0, T, SUB, want);
    }
    return trips;
}

// The edge rows (tests/test_gpu_guard_bounds.py gives the same rows to the voices of its banks: keep the two lists alike).
static std::vector<Row> edge_rows() {
    const float sr = 48000.0f, INF = INFINITY;
    std::vector<Row> rows;
    auto turns = [&](float t) { return t * sr / 64.0f; };  // the frequency whose 64-frame block sweeps t turns of phase
    // block excursion below / at / above the 2047-turn threshold and the 2048-turn end of the packed domain: on the carrier (m = 0: its input is f) ...
    for (float t : {2040.0f, 2046.0f, 2046.9f, 2047.0f, 2047.1f, 2047.9f, 2048.0f, 2048.1f, 2050.0f, -2046.9f, -2047.1f, -2050.0f})
        rows.push_back({turns(t), 0.0f, 1000.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, false});
    // ... and with the modulation adding to it (16 |f m| + |f| straddles the threshold, the true sweep stays inside)
    for (float fm : {turns(2046.0f) / 16.0f, turns(2048.0f) / 16.0f, turns(1000.0f), turns(2040.0f)})
        rows.push_back({1000.0f, fm / 1000.0f, 2000.0f, 0.7f, 0.25f, 0.5f, 0.0f, 0.0f, false});
    rows.push_back({100.0f, 1.0e6f, 500.0f, 2.0f, 0.0f, 0.0f, 0.0f, 0.0f, false});   // a bound far outside, the true sweep outside too
    rows.push_back({1000.0f, 500.0f, 500.0f, 2.0f, 0.0f, 0.0f, 0.0f, 0.0f, false});  // the bound says "might trip", the true phase stays in the domain
    // initial phases: far from zero (the first block only), -0.0 (wide_sin2's one wrong argument), +0.0
    for (float ph : {3000.0f, -0.0f, 0.0f, 2046.5f, -3000.0f})
        for (int which = 0; which < 2; which++)
            rows.push_back({440.0f, 2.0f, 1200.0f, 1.0f, which ? 0.125f : ph, which ? ph : 0.125f, 0.0f, 0.0f, false});
    // negative f, negative m
    rows.push_back({-440.0f, 2.0f, 1200.0f, 1.0f, 0.3f, 0.6f, 0.0f, 0.0f, false});
    rows.push_back({440.0f, -3.0f, 1200.0f, 1.0f, 0.3f, 0.6f, 0.0f, 0.0f, false});
    rows.push_back({-1760.0f, -7.9f, 5000.0f, 3.0f, 0.9f, 0.1f, 0.0f, 0.0f, false});
    // preset filter states around the 2^96 limit, at the top of the range, infinite, NaN; ic2eq = -0.0
    for (float s : {0x1p95f, 0x1p96f, 0x1p97f, 0x1p126f, 0x1p127f, -0x1p95f, -0x1p96f, -0x1p97f, -0x1p126f, -0x1p127f, INF, -INF, NAN, 0x1.fffffep95f, 0x1.fffffep127f})
        for (int which = 0; which < 2; which++)
            rows.push_back({220.0f, 1.5f, 800.0f, 0.8f, 0.2f, 0.4f, which ? 0.0f : s, which ? s : 0.0f, true});
    rows.push_back({220.0f, 1.5f, 800.0f, 0.8f, 0.2f, 0.4f, 0.0f, -0.0f, true});
    rows.push_back({220.0f, 1.5f, 800.0f, 0.8f, 0.2f, 0.4f, 0x1p120f, -0x1p120f, true});
    // cutoffs above Nyquist (g < 0: A > 1) and extreme q, from rest and from large states: A^8 large or overflowing
    for (float fc : {30000.0f, 47000.0f, 23999.0f, 24001.0f, 71000.0f})
        for (float q : {1.0f, 1.0e-30f, 1.0e30f}) {
            rows.push_back({330.0f, 1.0f, fc, q, 0.1f, 0.2f, 0.0f, 0.0f, false});
            rows.push_back({330.0f, 1.0f, fc, q, 0.1f, 0.2f, 0x1p90f, -0x1p60f, true});
        }
    rows.push_back({330.0f, 1.0f, 1000.0f, 1.0e-30f, 0.1f, 0.2f, 0.0f, 0.0f, false});
    rows.push_back({330.0f, 1.0f, 1000.0f, 1.0e30f, 0.1f, 0.2f, 0.0f, 0.0f, false});
    return rows;
}

int main(int argc, char** argv) {
    const double sr = 48000.0;
    const std::vector<Row> rows = edge_rows();
    if (argc > 1 && !strcmp(argv[1], "--rows")) {  // the rows, for the GPU test: f m fc q ph_mod ph_car ic1 ic2 as bit patterns, preset
        for (const Row& r : rows)
            printf("%08x %08x %08x %08x %08x %08x %08x %08x %d\n", f2u(r.f), f2u(r.m), f2u(r.fc), f2u(r.q), f2u(r.ph_mod), f2u(r.ph_car), f2u(r.ic1), f2u(r.ic2), (int)r.preset);
        return 0;
    }
    unsigned long edge_trips = 0;
    for (size_t k = 0; k < rows.size(); k++) {
        edge_trips += check_fm(rows[k], (int)k, 200, sr);
        edge_trips += check_fm(rows[k], (int)k, 192, sr);
        edge_trips += check_shl(rows[k], (int)k, 200, sr);
    }
    // the bounded forms really run unguarded: an ordinary voice never trips, the sines' tmax is never raised (the per-frame
    // guard would have left the largest quadrant argument there) and the filter's vmax holds the seeded bound
    unsigned long long vacuous = 0;
    {
        const Row r{440.0f, 2.0f, 1200.0f, 1.0f, 0.25f, 0.5f, 0.0f, 0.0f, false};
        FmSvfB e;
        if (check_fm(r, -1, 200, sr, &e) != 0) vacuous++;
        if (!(e.x.x.x.x.x.y.tmax == 0.0f && e.x.y.tmax == 0.0f && e.y.vmax >= SINE_OUT_BOUND && e.y.vmax < 64.0f)) vacuous++;
        FmSvf u = make_fm(r, sr);
        std::vector<float> y(200);
        render_packed(u, 200, 64, y);
        if (!(u.x.y.tmax > 0.0f && u.y.vmax > 0.0f && u.y.vmax < SINE_OUT_BOUND)) vacuous++;  // (what the per-frame guards leave behind)
        ShlB s;
        if (check_shl(r, -1, 200, sr, &s) != 0) vacuous++;
        if (!(s.x.y.tmax == 0.0f && s.y.vmax >= SINE_OUT_BOUND)) vacuous++;
        // ... and rows that MUST take the rollback do: a carrier sweep past the domain, a state past the limit
        if (check_fm(Row{2050.0f * 750.0f, 0.0f, 1000.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, false}, -2, 64, sr) == 0) vacuous++;
        if (check_fm(Row{220.0f, 1.5f, 800.0f, 0.8f, 0.2f, 0.4f, 0x1p97f, 0.0f, true}, -3, 64, sr) == 0) vacuous++;
        // ... while one just inside the limits does not: 2046 turns per block from phase 0; a state of 2^95
        if (check_fm(Row{2046.0f * 750.0f, 0.0f, 1000.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, false}, -4, 64, sr) != 0) vacuous++;
        if (check_fm(Row{220.0f, 1.5f, 800.0f, 0.8f, 0.2f, 0.4f, 0x1p95f, 0.0f, true}, -5, 8, sr) != 0) vacuous++;
    }
    // ordinary audio parameters (the sweep of check_svf_paths.hip, plus config 3's f and m ranges): not one tile may trip
    uint64_t st = 7;
    auto rnd = [&]() { st = st * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(st >> 32); };
    auto uni = [&]() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); };
    unsigned long audio_trips = 0;
    for (int trial = 0; trial < 4000; trial++) {
        Row r{55.0f * powf(32.0f, uni()), 0.5f + 7.5f * uni(), 20.0f * powf(1000.0f, uni()), 0.3f + 5.0f * uni(), uni(), uni(), 0.0f, 0.0f, false};
        audio_trips += check_fm(r, 100000 + trial, trial % 2 ? 200 : 192, sr);
        if (trial % 4 == 0) audio_trips += check_shl(r, 100000 + trial, 200, sr);
    }
    printf("edge rows %zu (tiles re-rendered by the bounded forms: %lu), audio trips %lu, vacuous %llu, bad %llu\n", rows.size(), edge_trips, audio_trips, vacuous, bad);
    return (bad != 0 || vacuous != 0 || audio_trips != 0) ? 1 : 0;
}
