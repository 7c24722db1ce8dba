// fd_engine.hpp -- host side of the bank kernels: per-kind dispatch table for the ahead-of-time compiled voice graphs.
#pragma once

#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "fd_device.hpp"
#include "fd_opts.hpp"

namespace fd {

struct SlotInfo {
    std::string name;
    int kind;
};

struct VDescribe {  // host only
    std::vector<SlotInfo>* out;
    std::vector<int> path;
    std::string prefix() const {
        std::string s;
        for (size_t i = 0; i < path.size(); i++) {
            if (i) s += ".";
            s += std::to_string(path[i]);
        }
        return s;
    }
    void add(const std::string& field, int kind) { out->push_back({prefix() + ":" + field, kind}); }
    void f(float&, FieldKind k, const char* name) { add(name, k); }
    void fi(float&, FieldKind k, const char* name, int index) {
        add(std::string(name) + "[" + std::to_string(index) + "]", k);
    }
    void u32(uint32_t&, FieldKind k, const char* name) { add(name, k); }
    void u64(uint64_t&, FieldKind k, const char* name) {
        add(std::string(name) + ".lo", k);
        add(std::string(name) + ".hi", k);
    }
    void enter(int i) { path.push_back(i); }
    void leave() { path.pop_back(); }
    bool keeps = false;  // a node said that its reset() keeps something of earlier rendering (fd_nodes.hpp note_stale)
    void stale() { keeps = true; }
};

// ---- per-kind dispatch table ---------------------------------------------------------------------------------
struct KindOps {
    std::string name;
    int nin, nout, nrings;
    std::vector<SlotInfo> slots;
    // parameters the graph's Rust TYPE carries (filter modes, shape kinds ...: fdsp_graph_compile_rust): applied to every
    // voice of a new bank right after construction
    std::vector<std::pair<std::string, float>> presets;
    std::function<void(float* slots, size_t stride, size_t first, size_t count, int op, double sr,
                       const uint64_t* d_seeds, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s)>
        lifecycle;
    std::function<void(float* slots, size_t stride, size_t V, const float* in, float* out, size_t T, size_t fstride,
                       int layout, int mode, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s)>
        render;
    // the same launch for the tolerance-mode variant FastOf<G> of the graph (fdsp_set_option("math", 1)); empty when the
    // graph has no node with a tolerance-mode form (then `render` is used)
    std::function<void(float* slots, size_t stride, size_t V, const float* in, float* out, size_t T, size_t fstride,
                       int layout, int mode, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s)>
        render_fast;
    // ... and render_fast has the time-split kernel with the time-parallel filter stage ("svf_exec" 1; fdsp_bank_get_option "has_svf_parallel")
    bool svf_parallel = false;
    // Render + mix-down in one launch (fd_device.hpp "fused mix-down"): part = device [voice groups][mix channels][T] partial
    // mixes, mix = MIX_SUM / MIX_PAN, panw = device [2][stride] pan weights (MIX_PAN).  Voice-minor inputs.  false = this graph /
    // launch has no fused kernel.  Empty for kinds built without one (attach_mix<G>).
    std::function<bool(float* slots, size_t stride, size_t V, const float* in, float* part, size_t T, int mix, int mode,
                       const void* aux, float* ring, uint32_t ring_cap, const float* panw, hipStream_t s)>
        render_mix, render_mix_fast;
    // Whatever the fused mix-down of this kind still has to do before its first launch (run-time compiled graphs: compile and load the
    // mix kernels) -- called by fdsp_bank_mix_reserve AND fdsp_bank_set_pan (either may be the last call a host makes BEFORE its real-time
    // loop or stream capture), and by fdsp_bank_set_option("math") for a bank that already holds a partial-mix buffer; `fast`: the tolerance-mode variant.  Empty for ahead-of-time kinds.
    std::function<void(bool fast)> prepare_mix;
    // ... and the render path of a bank of `voices` voices (run-time compiled three-stage generator chains: the time-split kernels that
    // small banks take live in the kind's second module; `fast`: the tolerance-mode twin FastOf<G>, a module of its own) -- called when a
    // bank is created and when fdsp_bank_set_option switches its arithmetic, so that no render compiles anything.
    std::function<void(size_t voices, bool fast)> prepare_render;
    // ... and the Sequencer's mixed output in one launch (render_sched_body MIXE): part as above, [groups][outputs][T]; graphs of
    // at most two outputs (the block tiles of four waves must fit the CU's LDS)
    std::function<bool(float* slots, size_t stride, size_t V, const float* in, float* part, size_t T, const double* ev,
                       const int* fade, double time0, double sr, int mode, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s)>
        render_events_mix;
    // Sequencer-style rendering (fd_device.hpp render_sched_body with EventNotes): ev = device [4][stride] f64, fade = device [V] or null
    std::function<void(float* slots, size_t stride, size_t V, const float* in, float* out, size_t T, const double* ev,
                       const int* fade, double time0, double sr, int mode, const void* aux, float* ring,
                       uint32_t ring_cap, hipStream_t s)>
        render_events;
    // ... and scores (the same body with ScoreNotes, fdsp_bank_set_score): sc = the score on the device; the mix variant like
    // render_events_mix (false / empty: more than two outputs, or a kind built without the mix kernels)
    std::function<void(float* slots, size_t stride, size_t V, const float* in, float* out, size_t T, const ScoreData& sc, double time0,
                       double sr, int mode, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s)>
        render_score;
    std::function<bool(float* slots, size_t stride, size_t V, const float* in, float* part, size_t T, const ScoreData& sc, double time0,
                       double sr, int mode, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s)>
        render_score_mix;
    // whatever the score kernels of this kind still need before their first launch (run-time compiled graphs: compile and load
    // them) -- called by fdsp_bank_set_score, never by a render; false + *err: they cannot be built.  Empty for ahead-of-time kinds.
    std::function<bool(std::string* err)> prepare_score;
    // ... and scores with one lane per note (fd_device.hpp render_score_notes_body, "score_exec" = FDSP_SCORE_NOTES): voice-out only;
    // the owner of a voice's write-back stores to `stage` [slots][stride] and raises flag[voice], the host commits afterwards.
    // note_fresh: the kind can take that path -- no rings and no node whose reset() keeps earlier state; empty / false otherwise.
    bool note_fresh = false;
    // in: the input rows [channel][in_T][V] from the launch's first frame on (a chunk of a longer launch renders T < in_T frames).
    std::function<void(const float* slots, float* stage, int* flag, size_t stride, size_t V, const float* in, size_t in_T, float* out, size_t T,
                       const ScoreData& sc, double time0, double sr, int mode, const void* aux, hipStream_t s)>
        render_score_notes;
};

template <class G>
void launch_lifecycle(float* slots, size_t stride, size_t first, size_t count, int op, double sr,
                      const uint64_t* d_seeds, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s) {
    if (count == 0) return;
    unsigned grid = (unsigned)((count + 63) / 64);
    hipLaunchKernelGGL((k_lifecycle<G>), dim3(grid), dim3(64), 0, s, slots, stride, first, count, op, sr, d_seeds, aux,
                       ring, ring_cap);
}

// ---- render: the launch plan (fd_plan.hpp) decides, these launch the kernel it names.  Only the kernels a graph can be planned into
// are instantiated: the `if constexpr` guards below say as types what graph_traits<G>() tells the plan as values.
struct RenderArgs {
    float* slots; size_t stride, V; const float* in; float* out; size_t T, fstride; const void* aux; float* ring; uint32_t ring_cap;
    const float* panw;  // fused mix-down (`out` is then the partial-mix buffer)
    hipStream_t s;
};
template <int N> using IntC = std::integral_constant<int, N>;
// f(IntC<GPW>) for the plan's voice groups per workgroup; workgroups of 1 / 2 groups exist for heavy graphs only
template <class G, class F>
void with_gpw(int gpw, F&& f) {
    if constexpr (Cost<G>::v >= 150) {
        if (gpw == 1) return f(IntC<1>{});
        if (gpw == 2) return f(IntC<2>{});
    }
    f(IntC<4>{});
}
// the voice-minor stage pipeline of pipe_plan<G>(WANT); MIX != MIX_NONE: with the fused mix-down
template <class G, int MODE, int WANT, int MIX = MIX_NONE>
void launch_pipe(const RenderPlan& p, const RenderArgs& a) {
    constexpr PipePlan P = pipe_plan<G>(WANT);
    if constexpr (P.S >= 1) {
        constexpr int WAVES = PipeGeom<G::IN, P.S>::WAVES;  // for 4 voice groups
        with_gpw<G>(p.gpw, [&](auto gpw) {
            constexpr int GPW = decltype(gpw)::value;
            if constexpr (MIX == MIX_NONE)
                hipLaunchKernelGGL((k_render_pipe<G, MODE, P.S, P.K1, P.K2, GPW>), dim3(p.grid), dim3(16 * GPW * WAVES), 0, a.s, a.slots, a.stride, a.V,
                                   a.in, a.out, a.T, a.aux, a.ring, a.ring_cap);
            else
                hipLaunchKernelGGL((k_render_pipe_mix<G, MODE, P.S, P.K1, P.K2, GPW, MIX>), dim3(p.grid), dim3(16 * GPW * WAVES), 0, a.s, a.slots,
                                   a.stride, a.V, a.in, a.out, a.T, a.aux, a.ring, a.ring_cap, a.panw);
        });
    }
}
// the time-split kernels of small banks (process mode, voice-minor)
template <class G, int MIX>
void launch_ts(const RenderPlan& p, const RenderArgs& a) {
    auto ts3 = [&](auto gpw) {  // the three-way split, 1 or 2 voice groups per workgroup
        constexpr int GPW = decltype(gpw)::value, THREADS = 64 * Ts3Roles<GPW>::WAVES;
        if constexpr (MIX != MIX_NONE)
            hipLaunchKernelGGL((k_render_ts3_mix<G, GPW, MIX>), dim3(p.grid), dim3(THREADS), 0, a.s, a.slots, a.stride, a.V, a.out, a.T, a.aux, a.panw);
        else
            hipLaunchKernelGGL((k_render_ts3<G, GPW>), dim3(p.grid), dim3(THREADS), 0, a.s, a.slots, a.stride, a.V, a.out, a.T, a.aux);
    };
    if constexpr (MIX == MIX_NONE)
        if (p.ts_round2) {  // "time_split" 2: 2 + 2 + 1 waves, or 2 + 1 + 1
            if (p.ts_round2 == 2) hipLaunchKernelGGL((k_render_ts<G, 2, 2>), dim3(p.grid), dim3(64 * 5), 0, a.s, a.slots, a.stride, a.V, a.out, a.T, a.aux);
            else hipLaunchKernelGGL((k_render_ts<G, 2, 1>), dim3(p.grid), dim3(64 * 4), 0, a.s, a.slots, a.stride, a.V, a.out, a.T, a.aux);
            return;
        }
    if (p.gpw == 1) ts3(IntC<1>{});
    else ts3(IntC<2>{});
}
// the time-split kernel with the time-parallel filter stage ("svf_exec" 1; fd_tsp.hpp): a kind that has it says so by specialising
// TspKernel for its tolerance-mode graph type, and the unit that compiles the kernel defines launch_tsp for that type (fd_kinds_fm_tsp.hip)
template <class G> struct TspKernel { static constexpr bool ok = false; };
template <class G> void launch_tsp(const RenderPlan& p, const RenderArgs& a);
template <class G, int MODE, int LAYOUT>
void launch_single(const RenderPlan& p, const RenderArgs& a) {
    constexpr int WPB = RenderGeom<G, LAYOUT>::WPB;  // = p.gpw
    const size_t fstride = LAYOUT == LAYOUT_VOICE_MINOR ? (size_t)p.vpw : a.fstride;  // see render_body: fstride carries voices-per-wave here
    hipLaunchKernelGGL((k_render<G, MODE, LAYOUT, WPB>), dim3(p.grid), dim3(64 * WPB), 0, a.s, a.slots, a.stride, a.V, a.in, a.out, a.T, fstride, a.aux,
                       a.ring, a.ring_cap);
}
template <class G, int MODE>
void launch_render_mode(const RenderPlan& p, const RenderArgs& a, int layout) {
    if (p.family == LK_PIPELINE_PLANAR) {  // loader / compute stages / storer
        using PP = PlanarPlan<G>;
        if constexpr (PP::S >= 1)
            with_gpw<G>(p.gpw, [&](auto gpw) {
                constexpr int GPW = decltype(gpw)::value;
                hipLaunchKernelGGL((k_render_pipe_planar<G, MODE, PP::S, PP::K1, GPW>), dim3(p.grid), dim3(64 * GPW * PP::T::WAVES), 0, a.s, a.slots,
                                   a.stride, a.V, a.in, a.out, a.T, a.fstride, a.aux, a.ring, a.ring_cap);
            });
    } else if (p.family == LK_PIPELINE) {
        if (p.want == 1) launch_pipe<G, MODE, 1>(p, a);
        else if (p.want == 2) launch_pipe<G, MODE, 2>(p, a);
        else if (p.want == 3) launch_pipe<G, MODE, 3>(p, a);
        else launch_pipe<G, MODE, 0>(p, a);
    } else if (layout == LAYOUT_VOICE_MINOR) {
        launch_single<G, MODE, LAYOUT_VOICE_MINOR>(p, a);
    } else {
        launch_single<G, MODE, LAYOUT_PLANAR>(p, a);
    }
}
template <class G>
void launch_render(float* slots, size_t stride, size_t V, const float* in, float* out, size_t T, size_t fstride,
                   int layout, int mode, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s) {
    if (V == 0 || T == 0) return;
    GraphTraits traits = graph_traits<G>(false);
    traits.tsp_ok = TspKernel<G>::ok;
    const RenderPlan p = plan_render(traits, tl_opts, (size_t)simd_count() / 4, V, T, layout, mode, fstride, (((uintptr_t)in | (uintptr_t)out) & 15) == 0);
    tl_opts.last_kernel = p.family;
    const RenderArgs a{slots, stride, V, in, out, T, fstride, aux, ring, ring_cap, nullptr, s};
    if (p.family == LK_TIME_SPLIT) {
        if constexpr (TsPlan<G>::ok) launch_ts<G, MIX_NONE>(p, a);
    } else if (p.family == LK_TIME_SPLIT_SVF) {
        if constexpr (TspKernel<G>::ok) launch_tsp<G>(p, a);
    } else if (mode == MODE_PROCESS) {
        launch_render_mode<G, MODE_PROCESS>(p, a, layout);
    } else {
        launch_render_mode<G, MODE_TICK>(p, a, layout);
    }
}

// ---- render + mix-down in one launch ------------------------------------------------------------------------------
template <class G>
bool launch_render_mix(float* slots, size_t stride, size_t V, const float* in, float* part, size_t T, int mix, int mode,
                       const void* aux, float* ring, uint32_t ring_cap, const float* panw, hipStream_t s) {
    if (V == 0 || T == 0) return true;
    constexpr GraphTraits traits = graph_traits<G>(false);
    const RenderPlan p = plan_render_mix(traits, tl_opts, (size_t)simd_count() / 4, V, T, mix, mode);
    if (p.family == LK_NONE) return false;
    tl_opts.last_kernel = p.family;
    const RenderArgs a{slots, stride, V, in, part, T, 0, aux, ring, ring_cap, panw, s};
    auto launch = [&](auto mix_c) {
        constexpr int MIX = decltype(mix_c)::value;
        if (p.family == LK_TIME_SPLIT) {
            if constexpr (TsPlan<G>::ok) launch_ts<G, MIX>(p, a);
        } else if (mode == MODE_PROCESS) {
            launch_pipe<G, MODE_PROCESS, 0, MIX>(p, a);
        } else {
            launch_pipe<G, MODE_TICK, 0, MIX>(p, a);
        }
    };
    if (mix != MIX_PAN) launch(IntC<MIX_SUM>{});
    else if constexpr (G::OUT == 1) launch(IntC<MIX_PAN>{});
    return true;
}
template <class G>
bool launch_render_events_mix(float* slots, size_t stride, size_t V, const float* in, float* part, size_t T, const double* ev,
                              const int* fade, double time0, double sr, int mode, const void* aux, float* ring,
                              uint32_t ring_cap, hipStream_t s) {
    if (V == 0 || T == 0) return true;
    if constexpr (G::OUT <= 2) {
        tl_opts.last_kernel = LK_EVENTS;
        const unsigned grid = (unsigned)(((V + 63) / 64 + 3) / 4);
        if (mode == MODE_PROCESS)
            hipLaunchKernelGGL((k_render_events_mix<G, MODE_PROCESS>), dim3(grid), dim3(256), 0, s, slots, stride, V, in, part, T, ev,
                               fade, time0, sr, aux, ring, ring_cap);
        else
            hipLaunchKernelGGL((k_render_events_mix<G, MODE_TICK>), dim3(grid), dim3(256), 0, s, slots, stride, V, in, part, T, ev,
                               fade, time0, sr, aux, ring, ring_cap);
        return true;
    } else {
        return false;
    }
}
template <class G>
bool launch_render_score_mix(float* slots, size_t stride, size_t V, const float* in, float* part, size_t T, const ScoreData& sc, double time0,
                             double sr, int mode, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s) {
    if (V == 0 || T == 0) return true;
    if constexpr (G::OUT <= 2) {
        tl_opts.last_kernel = LK_SCORE;
        const unsigned grid = (unsigned)(((V + 63) / 64 + 3) / 4);
        if (mode == MODE_PROCESS)
            hipLaunchKernelGGL((k_render_score_mix<G, MODE_PROCESS>), dim3(grid), dim3(256), 0, s, slots, stride, V, in, part, T, sc, time0, sr,
                               aux, ring, ring_cap);
        else
            hipLaunchKernelGGL((k_render_score_mix<G, MODE_TICK>), dim3(grid), dim3(256), 0, s, slots, stride, V, in, part, T, sc, time0, sr,
                               aux, ring, ring_cap);
        return true;
    } else {
        return false;
    }
}
// gives a kind its fused mix-down kernels (opt-in per kind: every instantiation is compile time and code size)
template <class G>
void attach_mix(std::vector<KindOps>& kinds, const char* name) {
    for (KindOps& k : kinds)
        if (k.name == name) {
            k.render_mix = &launch_render_mix<G>;
            k.render_events_mix = &launch_render_events_mix<G>;
            k.render_score_mix = &launch_render_score_mix<G>;
            using GF = typename FastOf<G>::type;
            if constexpr (!SameType<GF, G>::v) k.render_mix_fast = &launch_render_mix<GF>;
        }
}

template <class G>
void launch_render_events(float* slots, size_t stride, size_t V, const float* in, float* out, size_t T, const double* ev,
                          const int* fade, double time0, double sr, int mode, const void* aux, float* ring,
                          uint32_t ring_cap, hipStream_t s) {
    if (V == 0 || T == 0) return;
    tl_opts.last_kernel = LK_EVENTS;
    const unsigned grid = (unsigned)(((V + 63) / 64 + 3) / 4);
    if (mode == MODE_PROCESS)
        hipLaunchKernelGGL((k_render_events<G, MODE_PROCESS>), dim3(grid), dim3(256), 0, s, slots, stride, V, in, out, T, ev,
                           fade, time0, sr, aux, ring, ring_cap);
    else
        hipLaunchKernelGGL((k_render_events<G, MODE_TICK>), dim3(grid), dim3(256), 0, s, slots, stride, V, in, out, T, ev,
                           fade, time0, sr, aux, ring, ring_cap);
}

template <class G>
void launch_render_score(float* slots, size_t stride, size_t V, const float* in, float* out, size_t T, const ScoreData& sc, double time0,
                         double sr, int mode, const void* aux, float* ring, uint32_t ring_cap, hipStream_t s) {
    if (V == 0 || T == 0) return;
    tl_opts.last_kernel = LK_SCORE;
    const unsigned grid = (unsigned)(((V + 63) / 64 + 3) / 4);
    if (mode == MODE_PROCESS)
        hipLaunchKernelGGL((k_render_score<G, MODE_PROCESS>), dim3(grid), dim3(256), 0, s, slots, stride, V, in, out, T, sc, time0, sr, aux,
                           ring, ring_cap);
    else
        hipLaunchKernelGGL((k_render_score<G, MODE_TICK>), dim3(grid), dim3(256), 0, s, slots, stride, V, in, out, T, sc, time0, sr, aux,
                           ring, ring_cap);
}

template <class G>
void launch_render_score_notes(const float* slots, float* stage, int* flag, size_t stride, size_t V, const float* in, size_t in_T, float* out, size_t T,
                               const ScoreData& sc, double time0, double sr, int mode, const void* aux, hipStream_t s) {
    if (V == 0 || T == 0 || sc.N == 0) return;
    tl_opts.last_kernel = LK_SCORE_NOTES;
    const unsigned grid = (unsigned)(((size_t)sc.N + 255) / 256);  // lane = note
    if (mode == MODE_PROCESS)
        hipLaunchKernelGGL((k_render_score_notes<G, MODE_PROCESS>), dim3(grid), dim3(256), 0, s, slots, stage, flag, stride, V, in, in_T, out, T, sc,
                           time0, sr, aux);
    else
        hipLaunchKernelGGL((k_render_score_notes<G, MODE_TICK>), dim3(grid), dim3(256), 0, s, slots, stage, flag, stride, V, in, in_T, out, T, sc, time0,
                           sr, aux);
}

template <class G>
KindOps make_kind(const char* name) {
    KindOps k;
    k.name = name;
    k.nin = G::IN;
    k.nout = G::OUT;
    k.nrings = G::RINGS;
    G g{};
    VDescribe d{&k.slots, {}};
    g.visit(d);
    k.lifecycle = &launch_lifecycle<G>;
    k.render = &launch_render<G>;
    using GF = typename FastOf<G>::type;
    if constexpr (!SameType<GF, G>::v) k.render_fast = &launch_render<GF>;
    k.svf_parallel = TspKernel<GF>::ok;
    k.render_events = &launch_render_events<G>;
    k.render_score = &launch_render_score<G>;
    if constexpr (G::RINGS == 0) {  // notes of one voice would share the voice's ring
        k.note_fresh = !d.keeps;
        if (k.note_fresh) k.render_score_notes = &launch_render_score_notes<G>;
    }
    return k;
}

int jit_compile_code(const std::string& type_expr, const std::string& prelude, std::vector<char>* code, std::string* log);
int jit_make_kind(const std::string& name, const std::string& type_expr, const std::string& prelude, KindOps* out,
                  std::string* err);
int rust_translate(const char* rust_type_name, const char* hints, std::string* expr, std::string* presets);  // fd_rust.hip
void register_leaf_kinds(std::vector<KindOps>& out);
void register_graph_kinds(std::vector<KindOps>& out);

}  // namespace fd
