// fd_plan.hpp -- the launch plan of a voice-bank render: which kernel family a launch takes, with how many voice groups per
// workgroup and on what grid.  One pure host function per entry point (render, render + mix-down) holds the policy; the launchers
// of the ahead-of-time kinds (fd_engine.hpp) and of the run-time compiled kinds (fd_jit.hip) obey it.  Every family renders the
// same bits, so no bit-exactness test can see a wrong choice here: tests/host/check_render_plan.cpp holds the decision table.
// Plain C++17, no HIP header: a host program can include it alone; hiprtc reads it too, for GraphTraits (no system headers there).
#pragma once

#ifndef __HIPCC_RTC__
#include <stddef.h>
#endif

#include "fd_opts.hpp"

namespace fd {

constexpr int LAYOUT_VOICE_MINOR = 0, LAYOUT_PLANAR = 1;
constexpr int MODE_PROCESS = 0, MODE_TICK = 1;
constexpr int MIX_NONE = 0, MIX_SUM = 1, MIX_PAN = 2;  // sum every output channel over the voices | pan a mono graph to stereo, then sum

// Launch lengths from which a launch leaves the single-wave kernel: PipeMinT<G> (fd_device.hpp) for the stage pipeline, and one whole
// 64-frame block for the time-split kernels of small banks (config 3's shards: 9.2-9.8 us against 13.5-13.9 at T = 64, 12.5-13.4 against
// 22 at 128, 15-16 against 30 at 192; profiles/r04_small_t_kernels.txt).  "pipe_split" 2 / 3 force the pipeline at any length, 0 the
// single-wave kernel.
#ifndef FD_TS_MIN_T
#define FD_TS_MIN_T 64
#endif
// The planar pipeline (loader waves transpose 16-byte runs of the per-voice rows through LDS, a storer wave transposes back) beats the
// single-wave kernel's strided row accesses at every measured length and for every graph -- config 3: 9.8 vs 10.9 us at T = 16, 16.2 vs
// 19.1 at 64; config 4: 18.8 vs 28.0, 30.8 vs 51.9; config 2: 6.5 vs 6.9, 8.5 vs 9.0 (profiles/r04_small_t_kernels.txt, planar table).
#ifndef FD_PLANAR_PIPE_MIN_T
#define FD_PLANAR_PIPE_MIN_T 16
#endif

// What the policy knows about a graph type and about the kernels built for it.  graph_traits<G>() (fd_device.hpp) fills it, on the
// host for the ahead-of-time kinds and on the device (describe_body) for the run-time compiled ones: the same bytes on both.
struct GraphTraits {
    int nin, nout, nrings;
    int wpb_planar;           // waves per workgroup of the planar single-wave kernel (RenderGeom; voice-minor: always 4)
    int pipe_stages[4];       // compute stages of the voice-minor pipeline per pipe_want 0 .. 3, 0 = no such kernel; run-time kinds: the best plan's (graph_traits)
    int pipe_min_t;           // launch length from which the voice-minor pipeline is taken (PipeMinT)
    int pipe_threads;         // threads of a voice-minor pipeline workgroup of four voice groups
    int pipe_planar_threads;  // ... and of a planar one
    int planar_stages;        // compute stages of the planar pipeline, 0 = no such kernel
    int wide_waves;           // a wide sum of generators: waves of the chain kernel; 0 for ahead-of-time kinds (their single-wave entry handles wide sums)
    bool heavy;               // latency-bound waves (Cost >= 150): small banks spread over the CUs, 1 / 2 voice groups per workgroup
    bool small_groups_planar; // ... and the planar pipeline has those workgroups too: ahead-of-time kinds = heavy, run-time kinds never
    bool small_groups_mix;    // ... and so has the pipeline with the fused mix-down: ahead-of-time kinds = heavy, run-time kinds never
    bool ts_ok;               // a three-stage generator chain: small banks take the time-split kernels
    bool ts_round2;           // the kernels of "time_split" 2 exist: ahead-of-time kinds only
    bool ts_mix_ok;           // time-split kernels with the fused mix-down: ahead-of-time kinds = ts_ok, run-time kinds ts_ok && nout <= 2
    bool mix_sum_ok;          // MIX_SUM of nout channels fits beside the pipeline's tiles: run-time kinds jit_mix_channels_ok(nout)
    bool has_fast;            // the graph has a tolerance-mode twin (FastOf<G> is another type)
    bool note_fresh;          // scores may render the notes of a voice independently (no rings, no node marked note_stale); set where the graph is
                              // described (make_kind / describe_body), not by graph_traits: the answer comes from a visit()
    bool tsp_ok;              // the time-split kernel with the time-parallel filter stage exists (fd_tsp.hpp): tolerance-mode twins of some ahead-of-time
                              // kinds; set by their launcher (fd_engine.hpp launch_render), never for run-time kinds
};

struct RenderPlan {
    int family;    // LK_SINGLE_WAVE, LK_PIPELINE, LK_PIPELINE_PLANAR, LK_TIME_SPLIT, LK_TIME_SPLIT_SVF or LK_WIDE_CHAIN; LK_NONE = no fused kernel (plan_render_mix)
    int gpw;       // voice groups per workgroup: 1, 2 or 4 (single wave: waves per workgroup)
    unsigned grid; // workgroups
    int vpw;       // voices per wave (below 64 only in the voice-minor single-wave kernel)
    int want;      // LK_PIPELINE: which stage plan, index into GraphTraits::pipe_stages
    int ts_round2; // LK_TIME_SPLIT: 0 = the three-way split; "time_split" 2: waves of the second oscillator stage, 2 (2 + 2 + 1) or 1 (2 + 1 + 1)
};

// Launch policy for the voice-minor single-wave kernel: voices per wave such that the grid has at least one wave per SIMD.
inline int voices_per_wave(size_t V, int simds) {
    int vpw = 64;
    while (vpw > 16 && (V + vpw - 1) / vpw < (size_t)simds) vpw >>= 1;
    return vpw;
}

// "pipe_split" -> the stage plan pipe_plan<G>(want): 1 = best plan, 4 = loader wave only, 2 / 3 = exactly that many compute stages
constexpr int pipe_want(int pipe_split) { return pipe_split == 4 ? 1 : pipe_split == 2 ? 2 : pipe_split == 3 ? 3 : 0; }

inline unsigned plan_grid(size_t groups, int gpw) { return (unsigned)((groups + gpw - 1) / gpw); }

// stage pipelines: heavy graphs on small banks get one workgroup per CU (1 or 2 groups spend the LDS of 4 on longer tiles); else 4 groups
inline int pipe_gpw(bool small_groups, size_t groups, size_t cus) { return small_groups && groups <= cus ? 1 : small_groups && groups <= 2 * cus ? 2 : 4; }

// banks that leave most SIMDs idle (<= 2 voice groups per CU), whole 64-frame blocks: the oscillator stages are split over time as well
inline bool plan_time_split(const LaunchOpts& o, size_t cus, size_t groups, size_t T, int mode) {
    return o.pipe_split == 1 && mode == MODE_PROCESS && T % 64 == 0 && T >= FD_TS_MIN_T && groups <= 2 * cus;
}

// the second module of a run-time compiled kind (time-split kernels) is compiled ahead of the first render of such a bank
inline bool wants_time_split_module(const GraphTraits& g, size_t cus, size_t voices) { return g.ts_ok && (voices + 63) / 64 <= 2 * cus; }

inline RenderPlan plan_render(const GraphTraits& g, const LaunchOpts& o, size_t cus, size_t V, size_t T, int layout, int mode, size_t fstride,
                              bool io_aligned16) {
    const size_t groups = (V + 63) / 64;
    const bool voice_minor = layout == LAYOUT_VOICE_MINOR;
    if (g.ts_ok && voice_minor && plan_time_split(o, cus, groups, T, mode)) {
        if (o.time_split == 1) {  // both oscillator stages split three ways, the filter wave (nearly) alone on a SIMD
            // "svf_exec" 1, a request: the filter stage split over time too.  tsp_ok is only ever set for a tolerance-mode graph type, so the
            // bank's "math" is FDSP_MATH_FAST here; one voice group per workgroup only (the kernel's LDS tiles)
            if (o.svf_exec == 1 && g.tsp_ok && groups <= cus) return {LK_TIME_SPLIT_SVF, 1, (unsigned)groups, 64, 0, 0};
            const int gpw = groups <= cus ? 1 : 2;
            return {LK_TIME_SPLIT, gpw, plan_grid(groups, gpw), 64, 0, 0};
        }
        if (o.time_split == 2 && g.ts_round2)  // one workgroup per CU: 2 + 2 + 1 waves; two: 2 + 1 + 1 each, roles rotated between neighbours
            return {LK_TIME_SPLIT, 1, (unsigned)groups, 64, 0, groups <= cus ? 2 : 1};
    }
    // a wide sum of generators: the chain of waves for every launch of more than one block, in either layout; never a stage pipeline (fd_jit.hip)
    const bool wide = g.wide_waves > 0;
    if (wide && o.pipe_split && T > 64) return {LK_WIDE_CHAIN, 1, (unsigned)groups, 64, 0, 0};
    // planar rows that allow 16-byte runs go through the planar pipeline
    if (!wide && !voice_minor && o.pipe_split && g.planar_stages >= 1 && (T >= FD_PLANAR_PIPE_MIN_T || o.pipe_split > 1) && fstride % 4 == 0 &&
        io_aligned16) {
        const int gpw = g.small_groups_planar && groups < 2 * cus ? 1 : g.small_groups_planar && groups < 4 * cus ? 2 : 4;
        return {LK_PIPELINE_PLANAR, gpw, plan_grid(groups, gpw), 64, 0, 0};
    }
    // the stage pipeline from pipe_min_t frames on (one 64-frame block for chains worth cutting, four for light graphs)
    const int want = pipe_want(o.pipe_split);
    if (!wide && voice_minor && o.pipe_split && g.pipe_stages[want] >= 1 && (T >= (size_t)g.pipe_min_t || o.pipe_split > 1)) {
        const int gpw = pipe_gpw(g.heavy, groups, cus);
        return {LK_PIPELINE, gpw, plan_grid(groups, gpw), 64, want, 0};
    }
    // 4-wave workgroups unless the per-wave LDS tiles of the planar path would not fit 4x in the CU's LDS
    const int vpw = voice_minor ? voices_per_wave(V, (int)(4 * cus)) : 64, wpb = voice_minor ? 4 : g.wpb_planar;
    return {LK_SINGLE_WAVE, wpb, plan_grid((V + vpw - 1) / vpw, wpb), vpw, 0, 0};
}

// render + mix-down in one launch (voice-minor inputs); family LK_NONE = this graph / launch has no fused kernel
inline RenderPlan plan_render_mix(const GraphTraits& g, const LaunchOpts& o, size_t cus, size_t V, size_t T, int mix, int mode) {
    const size_t groups = (V + 63) / 64;
    if ((mix == MIX_PAN && g.nout != 1) || (mix == MIX_SUM && !g.mix_sum_ok)) return {LK_NONE, 0, 0, 0, 0, 0};
    if (g.ts_mix_ok && o.time_split == 1 && plan_time_split(o, cus, groups, T, mode)) {
        const int gpw = groups <= cus ? 1 : 2;
        return {LK_TIME_SPLIT, gpw, plan_grid(groups, gpw), 64, 0, 0};
    }
    if (g.pipe_stages[0] < 1) return {LK_NONE, 0, 0, 0, 0, 0};
    const int gpw = pipe_gpw(g.small_groups_mix, groups, cus);  // the pipeline's best plan, at any length and any "pipe_split"
    return {LK_PIPELINE, gpw, plan_grid(groups, gpw), 64, 0, 0};
}

}  // namespace fd
