// check_render_plan_svf.cpp -- the "svf_exec" branch of the launch policy (fundsp_amd/csrc/fd_plan.hpp plan_render) against a decision table
// written out by hand: the time-parallel filter family is chosen only where EVERY condition holds, and everywhere else the plan is the
// one "svf_exec" = 0 gives, field for field.  plan_render_mix never chooses it.  Host only, no HIP (as check_render_plan.cpp).
#include <cstdio>

#include "fd_plan.hpp"

using namespace fd;

namespace {
constexpr size_t C = 256;  // CUs
GraphTraits fm(bool tsp_ok) {  // the compiled FM voice (check_render_plan.cpp fm()); tsp_ok: its tolerance-mode twin
    GraphTraits t{};
    t.nout = 1;
    t.wpb_planar = 4;
    t.pipe_stages[0] = 2, t.pipe_stages[1] = 1, t.pipe_stages[2] = 2, t.pipe_stages[3] = 3;
    t.pipe_min_t = 64;
    t.pipe_threads = 192;
    t.pipe_planar_threads = 768;
    t.planar_stages = 2;
    t.mix_sum_ok = true;
    t.ts_ok = t.ts_round2 = t.ts_mix_ok = true;
    t.tsp_ok = tsp_ok;
    return t;
}
bool same(const RenderPlan& a, const RenderPlan& b) {
    return a.family == b.family && a.gpw == b.gpw && a.grid == b.grid && a.vpw == b.vpw && a.want == b.want && a.ts_round2 == b.ts_round2;
}
struct Row { const char* what; bool tsp_ok; int svf_exec, time_split, pipe_split; size_t V, T; int layout, mode; bool taken; };
}  // namespace

int main() {
    const Row rows[] = {
        {"every condition holds, one group", true, 1, 1, 1, 64, 64, LAYOUT_VOICE_MINOR, MODE_PROCESS, true},
        {"ragged group", true, 1, 1, 1, 65, 128, LAYOUT_VOICE_MINOR, MODE_PROCESS, true},
        {"one group per CU exactly", true, 1, 1, 1, 64 * C, 48000, LAYOUT_VOICE_MINOR, MODE_PROCESS, true},
        {"one group more than CUs", true, 1, 1, 1, 64 * C + 1, 64, LAYOUT_VOICE_MINOR, MODE_PROCESS, false},
        {"svf_exec 0", true, 0, 1, 1, 64, 64, LAYOUT_VOICE_MINOR, MODE_PROCESS, false},
        {"a graph type without the kernel (exact mode, run-time kinds)", false, 1, 1, 1, 64, 64, LAYOUT_VOICE_MINOR, MODE_PROCESS, false},
        {"time_split 0", true, 1, 0, 1, 64, 64, LAYOUT_VOICE_MINOR, MODE_PROCESS, false},
        {"time_split 2", true, 1, 2, 1, 64, 64, LAYOUT_VOICE_MINOR, MODE_PROCESS, false},
        {"pipe_split 0", true, 1, 1, 0, 64, 64, LAYOUT_VOICE_MINOR, MODE_PROCESS, false},
        {"pipe_split 2", true, 1, 1, 2, 64, 64, LAYOUT_VOICE_MINOR, MODE_PROCESS, false},
        {"not whole blocks", true, 1, 1, 1, 64, 100, LAYOUT_VOICE_MINOR, MODE_PROCESS, false},
        {"less than a block", true, 1, 1, 1, 64, 63, LAYOUT_VOICE_MINOR, MODE_PROCESS, false},
        {"planar", true, 1, 1, 1, 64, 64, LAYOUT_PLANAR, MODE_PROCESS, false},
        {"tick mode", true, 1, 1, 1, 64, 64, LAYOUT_VOICE_MINOR, MODE_TICK, false},
    };
    int n = 0, bad = 0;
    for (const Row& r : rows) {
        LaunchOpts o;
        o.svf_exec = r.svf_exec, o.time_split = r.time_split, o.pipe_split = r.pipe_split;
        LaunchOpts o0 = o;
        o0.svf_exec = 0;
        const GraphTraits g = fm(r.tsp_ok);
        const RenderPlan p = plan_render(g, o, C, r.V, r.T, r.layout, r.mode, 64, true), p0 = plan_render(g, o0, C, r.V, r.T, r.layout, r.mode, 64, true);
        const size_t groups = (r.V + 63) / 64;
        const bool ok = r.taken ? same(p, RenderPlan{LK_TIME_SPLIT_SVF, 1, (unsigned)groups, 64, 0, 0}) : same(p, p0) && p.family != LK_TIME_SPLIT_SVF;
        n++;
        if (!ok || p0.family == LK_TIME_SPLIT_SVF) {
            bad++;
            printf("FAILED %s: family %d gpw %d grid %u (svf_exec 0: family %d gpw %d grid %u)\n", r.what, p.family, p.gpw, p.grid, p0.family, p0.gpw, p0.grid);
        }
        const RenderPlan m = plan_render_mix(g, o, C, r.V, r.T, MIX_SUM, r.mode), m0 = plan_render_mix(g, o0, C, r.V, r.T, MIX_SUM, r.mode);
        n++;
        if (!same(m, m0) || m.family == LK_TIME_SPLIT_SVF) {
            bad++;
            printf("FAILED %s: plan_render_mix changed\n", r.what);
        }
    }
    static_assert(LK_TIME_SPLIT_SVF == 11, "the value fdsp_bank_get_option(bank, \"last_kernel\") reports");
    printf("%d rows, bad %d\n", n, bad);
    return bad ? 1 : 0;
}
