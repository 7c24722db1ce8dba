// check_render_plan.cpp -- the launch policy of the voice kernels (fundsp_amd/csrc/fd_plan.hpp) against its decision table.
// Every kernel family renders the same bits, so a wrong choice costs only speed and no GPU test can see it: the expected
// rows below are written out by hand (not a second transcription of the ladder) and sit on every edge of every condition.
// Host only, no HIP: c++ -std=c++17 -I fundsp_amd/csrc tests/host/check_render_plan.cpp.
#include <cstdio>

#include "fd_plan.hpp"

using namespace fd;

namespace {

constexpr size_t C = 256;  // CUs
constexpr int VM = LAYOUT_VOICE_MINOR, PL = LAYOUT_PLANAR, PR = MODE_PROCESS, TK = MODE_TICK;

GraphTraits base(bool heavy, int s0, int s1, int s2, int s3) {
    GraphTraits t{};
    t.nout = 1;
    t.wpb_planar = 4;
    t.pipe_stages[0] = s0, t.pipe_stages[1] = s1, t.pipe_stages[2] = s2, t.pipe_stages[3] = s3;
    t.pipe_min_t = 64;
    t.pipe_threads = 64 * (s0 + 1);
    t.pipe_planar_threads = 256 * 3;
    t.planar_stages = 2;
    t.heavy = heavy;
    t.mix_sum_ok = true;
    return t;
}
// the compiled FM voice (config 3's shape): a three-stage generator chain, light
GraphTraits fm() {
    GraphTraits t = base(false, 2, 1, 2, 3);
    t.ts_ok = t.ts_round2 = t.ts_mix_ok = true;
    return t;
}
// the same graph compiled at run time: one stage plan (none for the loader-only request: no inputs), no "time_split" 2 kernels
GraphTraits fm_rt() {
    GraphTraits t = base(false, 2, 0, 2, 2);
    t.ts_ok = t.ts_mix_ok = true;
    return t;
}
// a compiled heavy voice (config 4's shape): workgroups of 1 / 2 voice groups in every pipeline family
GraphTraits heavy() {
    GraphTraits t = base(true, 3, 1, 2, 3);
    t.small_groups_planar = t.small_groups_mix = true;
    return t;
}
// a heavy graph compiled at run time: those workgroups in the voice-minor pipeline only
GraphTraits heavy_rt(int wide_waves = 0, int nout = 1) {
    GraphTraits t = base(true, 3, 3, 3, 3);
    t.wide_waves = wide_waves;
    t.nout = nout;
    t.mix_sum_ok = nout <= 3;
    return t;
}
GraphTraits with(GraphTraits t, int nout, bool ts_mix_ok, int wpb_planar = 4) {
    t.nout = nout;
    t.ts_mix_ok = ts_mix_ok;
    t.wpb_planar = wpb_planar;
    return t;
}

struct Row {
    const char* what;
    GraphTraits g;
    int pipe_split, time_split;
    size_t V, T;
    int layout, mode;
    size_t fstride;
    bool aligned;
    RenderPlan want;  // family, gpw, grid, vpw, want, ts_round2
};
struct MixRow {
    const char* what;
    GraphTraits g;
    int pipe_split, time_split;
    size_t V, T;
    int mix, mode;
    RenderPlan want;
};

constexpr int SW = LK_SINGLE_WAVE, PP = LK_PIPELINE, PPL = LK_PIPELINE_PLANAR, TS = LK_TIME_SPLIT, WC = LK_WIDE_CHAIN, NO = LK_NONE;

const Row rows[] = {
    // ---- compiled FM voice, voice-minor: the time split on small banks and whole blocks -----------------------------------------------
    {"fm groups = cus", fm(), 1, 1, 64 * C, 64, VM, PR, 0, true, {TS, 1, 256, 64, 0, 0}},
    {"fm groups = cus, last voice", fm(), 1, 1, 64 * C - 63, 64, VM, PR, 0, true, {TS, 1, 256, 64, 0, 0}},
    {"fm groups = cus + 1", fm(), 1, 1, 64 * C + 1, 64, VM, PR, 0, true, {TS, 2, 129, 64, 0, 0}},
    {"fm groups = 2 cus", fm(), 1, 1, 128 * C, 64, VM, PR, 0, true, {TS, 2, 256, 64, 0, 0}},
    {"fm groups = 2 cus + 1", fm(), 1, 1, 128 * C + 1, 64, VM, PR, 0, true, {PP, 4, 129, 64, 0, 0}},
    {"fm T = 128", fm(), 1, 1, 64 * C, 128, VM, PR, 0, true, {TS, 1, 256, 64, 0, 0}},
    {"fm T = 65: not whole blocks", fm(), 1, 1, 64 * C, 65, VM, PR, 0, true, {PP, 4, 64, 64, 0, 0}},
    {"fm T = 63 = pipe_min_t - 1", fm(), 1, 1, 64 * C, 63, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"fm T = 16", fm(), 1, 1, 64 * C, 16, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"fm T = 15", fm(), 1, 1, 64 * C, 15, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"fm T = 63, one wave per SIMD and a voice", fm(), 1, 1, 256 * C + 1, 63, VM, PR, 0, true, {SW, 4, 257, 64, 0, 0}},
    {"fm T = 63, 32 voices per wave", fm(), 1, 1, 128 * C, 63, VM, PR, 0, true, {SW, 4, 256, 32, 0, 0}},
    {"fm time_split 0", fm(), 1, 0, 64 * C, 64, VM, PR, 0, true, {PP, 4, 64, 64, 0, 0}},
    {"fm time_split 2, groups = cus", fm(), 1, 2, 64 * C, 64, VM, PR, 0, true, {TS, 1, 256, 64, 0, 2}},
    {"fm time_split 2, groups = cus + 1", fm(), 1, 2, 64 * C + 1, 64, VM, PR, 0, true, {TS, 1, 257, 64, 0, 1}},
    {"fm time_split 2, groups = 2 cus", fm(), 1, 2, 128 * C, 64, VM, PR, 0, true, {TS, 1, 512, 64, 0, 1}},
    {"fm time_split 2, groups = 2 cus + 1", fm(), 1, 2, 128 * C + 1, 64, VM, PR, 0, true, {PP, 4, 129, 64, 0, 0}},
    {"fm time_split 2, T = 63", fm(), 1, 2, 64 * C, 63, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"fm tick mode", fm(), 1, 1, 64 * C, 64, VM, TK, 0, true, {PP, 4, 64, 64, 0, 0}},
    {"fm pipe_split 0", fm(), 0, 1, 64 * C, 64, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"fm pipe_split 2", fm(), 2, 1, 64 * C, 64, VM, PR, 0, true, {PP, 4, 64, 64, 2, 0}},
    {"fm pipe_split 3", fm(), 3, 1, 64 * C, 64, VM, PR, 0, true, {PP, 4, 64, 64, 3, 0}},
    {"fm pipe_split 4", fm(), 4, 1, 64 * C, 64, VM, PR, 0, true, {PP, 4, 64, 64, 1, 0}},
    {"fm pipe_split 2 forces the pipeline at T = 15", fm(), 2, 1, 200, 15, VM, PR, 0, true, {PP, 4, 1, 64, 2, 0}},
    {"fm pipe_split 4 forces the pipeline at T = 15", fm(), 4, 1, 200, 15, VM, PR, 0, true, {PP, 4, 1, 64, 1, 0}},
    {"fm pipe_split 1 at T = 15", fm(), 1, 1, 200, 15, VM, PR, 0, true, {SW, 4, 4, 16, 0, 0}},
    {"fm as built (no inputs: no loader-only plan), pipe_split 4", base(false, 2, 0, 2, 3), 4, 1, 200, 64, VM, PR, 0, true, {SW, 4, 4, 16, 0, 0}},
    {"fm_rt as built (no loader-only plan either), pipe_split 4", fm_rt(), 4, 1, 200, 64, VM, PR, 0, true, {SW, 4, 4, 16, 0, 0}},
    {"fm_rt as built, pipe_split 4 forces nothing at T = 15", fm_rt(), 4, 1, 200, 15, VM, PR, 0, true, {SW, 4, 4, 16, 0, 0}},
    {"fm without a three-stage plan, pipe_split 3", base(false, 2, 1, 2, 0), 3, 1, 200, 64, VM, PR, 0, true, {SW, 4, 4, 16, 0, 0}},
    // ---- ... planar ------------------------------------------------------------------------------------------------------------------
    {"fm planar T = 16", fm(), 1, 1, 200, 16, PL, PR, 16, true, {PPL, 4, 1, 64, 0, 0}},
    {"fm planar T = 15", fm(), 1, 1, 200, 15, PL, PR, 16, true, {SW, 4, 1, 64, 0, 0}},
    {"fm planar T = 15, pipe_split 2", fm(), 2, 1, 200, 15, PL, PR, 16, true, {PPL, 4, 1, 64, 0, 0}},
    {"fm planar frame stride 18", fm(), 1, 1, 200, 16, PL, PR, 18, true, {SW, 4, 1, 64, 0, 0}},
    {"fm planar unaligned", fm(), 1, 1, 200, 16, PL, PR, 16, false, {SW, 4, 1, 64, 0, 0}},
    {"fm planar pipe_split 0", fm(), 0, 1, 200, 16, PL, PR, 16, true, {SW, 4, 1, 64, 0, 0}},
    {"fm planar tick mode", fm(), 1, 1, 200, 16, PL, TK, 16, true, {PPL, 4, 1, 64, 0, 0}},
    {"fm planar: no time split", fm(), 1, 1, 64 * C, 64, PL, PR, 64, true, {PPL, 4, 64, 64, 0, 0}},
    {"planar single wave, one wave per workgroup", with(fm(), 1, true, 1), 1, 1, 200, 15, PL, PR, 16, true, {SW, 1, 4, 64, 0, 0}},
    {"no planar pipeline kernel", [] { GraphTraits t = fm(); t.planar_stages = 0; return t; }(), 1, 1, 200, 16, PL, PR, 16, true, {SW, 4, 1, 64, 0, 0}},
    // ---- the FM voice compiled at run time: no kernels for "time_split" 2 ------------------------------------------------------------
    {"fm_rt groups = cus", fm_rt(), 1, 1, 64 * C, 64, VM, PR, 0, true, {TS, 1, 256, 64, 0, 0}},
    {"fm_rt groups = 2 cus", fm_rt(), 1, 1, 128 * C, 64, VM, PR, 0, true, {TS, 2, 256, 64, 0, 0}},
    {"fm_rt time_split 2", fm_rt(), 1, 2, 64 * C, 64, VM, PR, 0, true, {PP, 4, 64, 64, 0, 0}},
    {"fm_rt pipe_split 3: its one plan", fm_rt(), 3, 1, 64 * C, 64, VM, PR, 0, true, {PP, 4, 64, 64, 3, 0}},
    // ---- compiled heavy voice: workgroups of 1 / 2 voice groups ------------------------------------------------------------------------
    {"heavy groups = cus", heavy(), 1, 1, 64 * C, 64, VM, PR, 0, true, {PP, 1, 256, 64, 0, 0}},
    {"heavy groups = cus + 1", heavy(), 1, 1, 64 * C + 1, 64, VM, PR, 0, true, {PP, 2, 129, 64, 0, 0}},
    {"heavy groups = 2 cus", heavy(), 1, 1, 128 * C, 64, VM, PR, 0, true, {PP, 2, 256, 64, 0, 0}},
    {"heavy groups = 2 cus + 1", heavy(), 1, 1, 128 * C + 1, 64, VM, PR, 0, true, {PP, 4, 129, 64, 0, 0}},
    {"heavy T = pipe_min_t - 1", heavy(), 1, 1, 64 * C, 63, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"heavy pipe_min_t = 256, T = 255", [] { GraphTraits t = heavy(); t.pipe_min_t = 256; return t; }(), 1, 1, 64 * C, 255, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"heavy pipe_min_t = 256, T = 256", [] { GraphTraits t = heavy(); t.pipe_min_t = 256; return t; }(), 1, 1, 64 * C, 256, VM, PR, 0, true, {PP, 1, 256, 64, 0, 0}},
    {"heavy planar groups = 2 cus - 1", heavy(), 1, 1, 64 * (2 * C - 1), 64, PL, PR, 64, true, {PPL, 1, 511, 64, 0, 0}},
    {"heavy planar groups = 2 cus", heavy(), 1, 1, 64 * (2 * C), 64, PL, PR, 64, true, {PPL, 2, 256, 64, 0, 0}},
    {"heavy planar groups = 4 cus - 1", heavy(), 1, 1, 64 * (4 * C - 1), 64, PL, PR, 64, true, {PPL, 2, 512, 64, 0, 0}},
    {"heavy planar groups = 4 cus", heavy(), 1, 1, 64 * (4 * C), 64, PL, PR, 64, true, {PPL, 4, 256, 64, 0, 0}},
    // ---- heavy graph compiled at run time: those workgroups in the voice-minor pipeline only ---------------------------------------------
    {"heavy_rt groups = cus", heavy_rt(), 1, 1, 64 * C, 64, VM, PR, 0, true, {PP, 1, 256, 64, 0, 0}},
    {"heavy_rt groups = cus + 1", heavy_rt(), 1, 1, 64 * C + 1, 64, VM, PR, 0, true, {PP, 2, 129, 64, 0, 0}},
    {"heavy_rt groups = 2 cus", heavy_rt(), 1, 1, 128 * C, 64, VM, PR, 0, true, {PP, 2, 256, 64, 0, 0}},
    {"heavy_rt groups = 2 cus + 1", heavy_rt(), 1, 1, 128 * C + 1, 64, VM, PR, 0, true, {PP, 4, 129, 64, 0, 0}},
    {"heavy_rt T = 63", heavy_rt(), 1, 1, 64 * C, 63, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"heavy_rt planar groups = 2 cus - 1", heavy_rt(), 1, 1, 64 * (2 * C - 1), 64, PL, PR, 64, true, {PPL, 4, 128, 64, 0, 0}},
    {"heavy_rt planar groups = 4 cus - 1", heavy_rt(), 1, 1, 64 * (4 * C - 1), 64, PL, PR, 64, true, {PPL, 4, 256, 64, 0, 0}},
    // ---- ... with a wide sum of generators at its root: the chain of waves, never a stage pipeline ---------------------------------------
    {"wide T = 65", heavy_rt(8), 1, 1, 64 * C, 65, VM, PR, 0, true, {WC, 1, 256, 64, 0, 0}},
    {"wide T = 128, ragged bank", heavy_rt(8), 1, 1, 64 * C + 1, 128, VM, PR, 0, true, {WC, 1, 257, 64, 0, 0}},
    {"wide T = 64", heavy_rt(8), 1, 1, 64 * C, 64, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"wide T = 64, pipe_split 2", heavy_rt(8), 2, 1, 64 * C, 64, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"wide T = 128, pipe_split 3", heavy_rt(8), 3, 1, 64 * C, 128, VM, PR, 0, true, {WC, 1, 256, 64, 0, 0}},
    {"wide T = 128, pipe_split 0", heavy_rt(8), 0, 1, 64 * C, 128, VM, PR, 0, true, {SW, 4, 256, 16, 0, 0}},
    {"wide planar T = 128, tick mode", heavy_rt(8), 1, 1, 200, 128, PL, TK, 128, true, {WC, 1, 4, 64, 0, 0}},
    {"wide planar T = 64", heavy_rt(8), 1, 1, 200, 64, PL, PR, 64, true, {SW, 4, 1, 64, 0, 0}},
};

const MixRow mix_rows[] = {
    {"fm pan groups = cus", fm(), 1, 1, 64 * C, 64, MIX_PAN, PR, {TS, 1, 256, 64, 0, 0}},
    {"fm pan groups = cus + 1", fm(), 1, 1, 64 * C + 1, 64, MIX_PAN, PR, {TS, 2, 129, 64, 0, 0}},
    {"fm sum groups = 2 cus", fm(), 1, 1, 128 * C, 64, MIX_SUM, PR, {TS, 2, 256, 64, 0, 0}},
    {"fm sum groups = 2 cus + 1", fm(), 1, 1, 128 * C + 1, 64, MIX_SUM, PR, {PP, 4, 129, 64, 0, 0}},
    {"fm pan T = 128", fm(), 1, 1, 64 * C, 128, MIX_PAN, PR, {TS, 1, 256, 64, 0, 0}},
    {"fm pan T = 65", fm(), 1, 1, 64 * C, 65, MIX_PAN, PR, {PP, 4, 64, 64, 0, 0}},
    {"fm pan T = 63: the pipeline at any length", fm(), 1, 1, 64 * C, 63, MIX_PAN, PR, {PP, 4, 64, 64, 0, 0}},
    {"fm pan T = 15", fm(), 1, 1, 64 * C, 15, MIX_PAN, PR, {PP, 4, 64, 64, 0, 0}},
    {"fm pan time_split 0", fm(), 1, 0, 64 * C, 64, MIX_PAN, PR, {PP, 4, 64, 64, 0, 0}},
    {"fm pan time_split 2: no such mix kernels", fm(), 1, 2, 64 * C, 64, MIX_PAN, PR, {PP, 4, 64, 64, 0, 0}},
    {"fm pan pipe_split 0: the pipeline all the same", fm(), 0, 1, 64 * C, 64, MIX_PAN, PR, {PP, 4, 64, 64, 0, 0}},
    {"fm pan pipe_split 2: the best plan", fm(), 2, 1, 64 * C, 64, MIX_PAN, PR, {PP, 4, 64, 64, 0, 0}},
    {"fm pan pipe_split 3", fm(), 3, 1, 64 * C, 64, MIX_PAN, PR, {PP, 4, 64, 64, 0, 0}},
    {"fm pan pipe_split 4", fm(), 4, 1, 64 * C, 64, MIX_PAN, PR, {PP, 4, 64, 64, 0, 0}},
    {"fm pan tick mode", fm(), 1, 1, 64 * C, 64, MIX_PAN, TK, {PP, 4, 64, 64, 0, 0}},
    {"pan on two outputs", with(fm(), 2, true), 1, 1, 64 * C, 64, MIX_PAN, PR, {NO, 0, 0, 0, 0, 0}},
    {"sum on two outputs", with(fm(), 2, true), 1, 1, 64 * C, 64, MIX_SUM, PR, {TS, 1, 256, 64, 0, 0}},
    {"run time, sum on three outputs: no time-split mix", with(fm_rt(), 3, false), 1, 1, 64 * C, 64, MIX_SUM, PR, {PP, 4, 64, 64, 0, 0}},
    {"run time, sum on four outputs", heavy_rt(0, 4), 1, 1, 64 * C, 64, MIX_SUM, PR, {NO, 0, 0, 0, 0, 0}},
    {"run time, pan on four outputs", heavy_rt(0, 4), 1, 1, 64 * C, 64, MIX_PAN, PR, {NO, 0, 0, 0, 0, 0}},
    {"no pipeline plan", base(false, 0, 0, 0, 0), 1, 1, 64 * C, 64, MIX_SUM, PR, {NO, 0, 0, 0, 0, 0}},
    {"heavy sum groups = cus", heavy(), 1, 1, 64 * C, 64, MIX_SUM, PR, {PP, 1, 256, 64, 0, 0}},
    {"heavy sum groups = cus + 1", heavy(), 1, 1, 64 * C + 1, 64, MIX_SUM, PR, {PP, 2, 129, 64, 0, 0}},
    {"heavy sum groups = 2 cus", heavy(), 1, 1, 128 * C, 64, MIX_SUM, PR, {PP, 2, 256, 64, 0, 0}},
    {"heavy sum groups = 2 cus + 1", heavy(), 1, 1, 128 * C + 1, 64, MIX_SUM, PR, {PP, 4, 129, 64, 0, 0}},
    {"heavy_rt sum groups = cus: four groups per workgroup", heavy_rt(), 1, 1, 64 * C, 64, MIX_SUM, PR, {PP, 4, 64, 64, 0, 0}},
    {"heavy_rt sum groups = 2 cus", heavy_rt(), 1, 1, 128 * C, 64, MIX_SUM, PR, {PP, 4, 128, 64, 0, 0}},
};

bool same(const RenderPlan& a, const RenderPlan& b) {
    return a.family == b.family && a.gpw == b.gpw && a.grid == b.grid && a.vpw == b.vpw && a.want == b.want && a.ts_round2 == b.ts_round2;
}
int report(const char* what, const RenderPlan& got, const RenderPlan& want) {
    if (same(got, want)) return 0;
    printf("FAIL %s: family %d gpw %d grid %u vpw %d want %d ts_round2 %d, expected %d %d %u %d %d %d\n", what, got.family, got.gpw, got.grid, got.vpw,
           got.want, got.ts_round2, want.family, want.gpw, want.grid, want.vpw, want.want, want.ts_round2);
    return 1;
}

}  // namespace

int main() {
    int bad = 0, n = 0;
    for (const Row& r : rows) {
        LaunchOpts o;
        o.pipe_split = r.pipe_split;
        o.time_split = r.time_split;
        bad += report(r.what, plan_render(r.g, o, C, r.V, r.T, r.layout, r.mode, r.fstride, r.aligned), r.want);
        n++;
    }
    for (const MixRow& r : mix_rows) {
        LaunchOpts o;
        o.pipe_split = r.pipe_split;
        o.time_split = r.time_split;
        bad += report(r.what, plan_render_mix(r.g, o, C, r.V, r.T, r.mix, r.mode), r.want);
        n++;
    }
    // the second module of a run-time compiled kind is wanted ahead of the first render of a bank of <= 2 voice groups per CU
    const struct { GraphTraits g; size_t voices; bool want; } mods[] = {
        {fm_rt(), 64 * C, true}, {fm_rt(), 128 * C, true}, {fm_rt(), 128 * C + 1, false}, {heavy_rt(), 64 * C, false}};
    for (const auto& m : mods) {
        if (wants_time_split_module(m.g, C, m.voices) != m.want) { printf("FAIL wants_time_split_module(%zu voices)\n", m.voices); bad++; }
        n++;
    }
    static_assert(pipe_want(0) == 0 && pipe_want(1) == 0 && pipe_want(4) == 1 && pipe_want(2) == 2 && pipe_want(3) == 3, "pipe_split -> stage plan");
    printf("%d rows, bad %d\n", n, bad);
    return bad ? 1 : 0;
}
