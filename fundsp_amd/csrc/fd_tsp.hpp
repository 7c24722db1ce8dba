// fd_tsp.hpp -- the three-way time-split kernel with a TIME-PARALLEL filter stage ("svf_exec" = FDSP_SVF_PARALLEL, tolerance mode).
//
// k_render_ts3 (fd_device.hpp) is bounded by its one serial FixedSvf wave: ~15 dependent instructions per frame, 64 frames per
// round.  Here that stage is cut over time as well (fd_svf_par.hpp has the algebra and the operation order):
//   stages 0, 1   ts_stage as in k_render_ts3, the same hand-over tiles: the filter's input is the serial kernel's, bit for bit;
//   stage 2       K chunk waves: wave c runs the f32 tick from state (0, 0) over frames [c LC, (c + 1) LC) of hand[1], LC = 64 / K, and
//                 leaves the zero-state outputs and its end state in the yz / z tiles;
//   stage 3       ONE fix-up wave, a round behind: P, r[] and the carried state in registers, 64 independent frames of
//                 yz + r . s, the state carried across the K chunks, the frames stored to `out` (buffer stores, as pipe_stage).
// rounds = nblocks + 3; the ONE __syncthreads() per round is the only synchronisation -- the chunk -> fix-up dependency is carried by
// the extra round and the double-buffered tiles (a tile written in round r is read in round r + 1 and written again in r + 2).
// One voice group per workgroup (banks of <= one group per CU), voice-minor, process mode, T a multiple of 64 (fd_plan.hpp).
// LDS: hand 64 KiB (W = 1) + yz 32 KiB + z 2 x K x 512 B = 98 KiB (K = 2) of the CU's 160.
// With the filter off the critical path the longest waves of a round are those of stage 1 (measured busy 87-95 % of the launch: they
// walk the carrier's phase through all 64 frames whatever their share of the sines), so THEY ask for issue priority here, as the
// filter wave does in k_render_ts3: without it the kernel is no faster than the serial one.
// The chunk and fix-up waves run plain scalar arithmetic: no packed-path guard, no rollback; non-finite samples propagate through
// z and s as they do through the serial state.
#pragma once

#include "fd_engine.hpp"
#include "fd_svf_par.hpp"

namespace fd {

// which graphs: a three-stage generator chain (TsPlan) whose last stage is exactly one FixedSvf -- any mode, the tick does not depend on it
template <class G> struct TspPlan { static constexpr bool ok = false; };
template <class X> struct TspPlan<Pipe<X, FixedSvf>> {
    static constexpr bool ok = TsPlan<Pipe<X, FixedSvf>>::ok && Chain<X>::N == 2 && Seg<Pipe<X, FixedSvf>, 1, 2>::OUT == 1;
};

// wave -> (stage, part); stage 2 = chunk wave `part`, stage 3 = the fix-up wave.  Waves w, w + 4, w + 8 of a workgroup share a SIMD
// (Ts3Roles).  The oscillator cuts are those of Ts3Roles<1> -- stage 0 in thirds (24 + 24 + 16 frames), stage 1 in quarters -- except in
// table 1 of K = 4.  Shipped: K = 2, table 0 (the measured table of all four is in DESIGN.md 6.21).
template <int K, int TABLE> struct Ts3pRoles;
// K = 4, twelve waves, three per SIMD:     SIMD 0: A0 B0 C0   SIMD 1: A1 B1 C1   SIMD 2: A2 B2 C2   SIMD 3: D B3 C3
template <> struct Ts3pRoles<4, 0> {
    static constexpr int WAVES = 12;
    static constexpr int stg[12] = {0, 0, 0, 3, 1, 1, 1, 1, 2, 2, 2, 2};
    static constexpr int prt[12] = {0, 1, 2, 0, 0, 1, 2, 3, 0, 1, 2, 3};
    static constexpr int cut[2][5] = {{0, 24, 48, 64, 64}, {0, 16, 32, 48, 64}};
};
// K = 4, the same places with the second oscillator stage cut 8 + 8 + 24 + 24: oscillator frames per SIMD 32 | 32 | 40 | 24 + D
// instead of 40 | 40 | 32 | 16 + D
template <> struct Ts3pRoles<4, 1> {
    static constexpr int WAVES = 12;
    static constexpr int stg[12] = {0, 0, 0, 3, 1, 1, 1, 1, 2, 2, 2, 2};
    static constexpr int prt[12] = {0, 1, 2, 0, 0, 1, 2, 3, 0, 1, 2, 3};
    static constexpr int cut[2][5] = {{0, 24, 48, 64, 64}, {0, 8, 16, 40, 64}};
};
// K = 2, ten waves: the two chunk waves (32 frames each) behind the lighter oscillator waves
//                                          SIMD 0: A2 B2 C0   SIMD 1: D B3 C1    SIMD 2: A0 B0         SIMD 3: A1 B1
template <> struct Ts3pRoles<2, 0> {
    static constexpr int WAVES = 10;
    static constexpr int stg[10] = {0, 3, 0, 0, 1, 1, 1, 1, 2, 2};
    static constexpr int prt[10] = {2, 0, 0, 1, 2, 3, 0, 1, 0, 1};
    static constexpr int cut[2][5] = {{0, 24, 48, 64, 64}, {0, 16, 32, 48, 64}};
};
// K = 2, the fix-up wave next to the 16-frame oscillator pair and both chunk waves next to B3
//                                          SIMD 0: A2 B2 D    SIMD 1: B3 C0 C1   SIMD 2: A0 B0         SIMD 3: A1 B1
template <> struct Ts3pRoles<2, 1> {
    static constexpr int WAVES = 10;
    static constexpr int stg[10] = {0, 1, 0, 0, 1, 2, 1, 1, 3, 2};
    static constexpr int prt[10] = {2, 3, 0, 1, 2, 0, 0, 1, 0, 1};
    static constexpr int cut[2][5] = {{0, 24, 48, 64, 64}, {0, 16, 32, 48, 64}};
};

#ifndef FD_TSP_PRIO
#define FD_TSP_PRIO 1
#endif

template <class G, int K, int TABLE>
FD_D void render_ts3p_body(float* __restrict__ slots, size_t stride, size_t V, float* __restrict__ out, size_t T, const void* aux) {
    using S0 = Seg<G, 0, 1>;
    using S1 = Seg<G, 1, 2>;
    using S2 = Seg<G, 2, 3>;
    using R = Ts3pRoles<K, TABLE>;
    constexpr int LC = 64 / K;
    constexpr int W = S0::OUT > S1::OUT ? S0::OUT : S1::OUT;
    static_assert(K * LC == 64 && LC % 2 == 0, "chunks of whole frame pairs tile the block");
    static_assert(S2::IN == 1 && S2::OUT == 1 && G::OUT == 1, "one mono filter behind the oscillators");
    static_assert(W * 64 + 32 + K <= 160, "tiles must fit the CU's 160 KiB");
    __shared__ v2f hand[2][2][W][32][64];  // [cut][buffer][channel][frame pair][lane]
    __shared__ v2f yzt[2][32][64];         // [buffer][frame pair][lane]: the chunks' zero-state outputs
    __shared__ v2f zt[2][K][64];           // [buffer][chunk][lane]: their end states
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int stage = R::stg[w], part = R::prt[w];
    const size_t v0 = (size_t)blockIdx.x * 64, v = v0 + lane;
    const bool live = v0 < stride, active = v < V;
    const bool run = live && active;
    const size_t nblocks = T / 64, rounds = nblocks + 3;
    G g{};
    Ctx ctx{static_cast<const Aux*>(aux), nullptr, 0, stride, 0};
    g.bind(ctx);
    if (live) {
        VLoad ld{slots + v, stride, 0};
        VGate::W<VLoad> gate{&ld, true};
        if (stage == 0) S0::visit(g, gate); else if (stage == 1) S1::visit(g, gate); else S2::visit(g, gate);
    }
#ifdef FD_TSP_STAGE_CLOCKS  // a measuring build (tools/svf_par_bench.py --trace): how long every role works per launch, the rest is barrier wait
    unsigned long long busy = 0;
    const unsigned long long clk0 = __builtin_amdgcn_s_memtime();
#endif
    auto loop = [&](size_t first, auto&& block) {
        for (size_t it = 0; it < rounds; it++) {
            if (run && it >= first && it - first < nblocks) {
#ifdef FD_TSP_STAGE_CLOCKS
                const unsigned long long c0 = __builtin_amdgcn_s_memtime();
#endif
                block(it - first);  // the block this stage works on in this round
#ifdef FD_TSP_STAGE_CLOCKS
                busy += __builtin_amdgcn_s_memtime() - c0;
#endif
            }
            __syncthreads();
        }
    };
    const SvfCore& f = g.y.c;
    const SvfpCoefs k{f.a1, f.a2, f.a3, f.m0, f.m1, f.m2};
#if FD_TSP_PRIO
    if (stage == 1) __builtin_amdgcn_s_setprio(1);  // the round's critical path (see the top of the file)
#endif
    if (stage == 0) {
        loop(0, [&](size_t j) { ts_stage<S0, G, true, W>(g, R::cut[0][part], R::cut[0][part + 1], lane, nullptr, hand[0][j & 1]); });
    } else if (stage == 1) {
        loop(1, [&](size_t j) { ts_stage<S1, G, false, W>(g, R::cut[1][part], R::cut[1][part + 1], lane, hand[0][j & 1], hand[1][j & 1]); });
    } else if (stage == 2) {
        loop(2, [&](size_t j) {
            const int b = (int)(j & 1);
            const v2f(*hin)[64] = &hand[1][b][0][part * (LC / 2)];
            v2f(*yz)[64] = &yzt[b][part * (LC / 2)];
            float z1 = 0.0f, z2 = 0.0f;
#pragma unroll
            for (int p = 0; p < LC / 2; p++) {
                const v2f x = hin[p][lane];
                const float ya = svfp_tick(k, z1, z2, x.x);
                const float yb = svfp_tick(k, z1, z2, x.y);
                yz[p][lane] = v2f{ya, yb};
            }
            zt[b][part][lane] = v2f{z1, z2};
        });
    } else {
        SvfpTables<LC> t;
        svfp_tables<LC>(k, t);  // 2 LC ticks in f64, once per launch: no host-side cache to keep in step with set_param / set_state
        float s1 = f.ic1eq, s2 = f.ic2eq;
        const int vrow = (int)(V * sizeof(float));
        loop(3, [&](size_t j) {
            const int b = (int)(j & 1);
            // rows of a block span 64 * V * 4 bytes < 2^32: the frame's row offset travels in the store's scalar offset (pipe_stage)
            const __amdgpu_buffer_rsrc_t orow = __builtin_amdgcn_make_buffer_rsrc(out + v0 + (j * 64) * V, 0, (int)0xffffffffu, 0x00020000);
#pragma unroll
            for (int c = 0; c < K; c++) {
#pragma unroll
                for (int p = 0; p < LC / 2; p++) {
                    const v2f yz = yzt[b][c * (LC / 2) + p][lane];
                    const float ya = svfp_fix(yz.x, t.rx[2 * p], t.ry[2 * p], s1, s2);
                    const float yb = svfp_fix(yz.y, t.rx[2 * p + 1], t.ry[2 * p + 1], s1, s2);
                    __builtin_amdgcn_raw_buffer_store_b32(f2u(ya), orow, lane * 4, (c * LC + 2 * p) * vrow, FD_PIPE_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b32(f2u(yb), orow, lane * 4, (c * LC + 2 * p + 1) * vrow, FD_PIPE_STORE_AUX);
                }
                const v2f z = zt[b][c][lane];
                svfp_carry<LC>(t, s1, s2, z.x, z.y);
            }
        });
        g.y.c.ic1eq = s1;
        g.y.c.ic2eq = s2;
    }
    if (run && part == 0 && stage != 2) {  // the waves of a split stage end with identical state: one of them stores it; the chunk waves have none
        VStore<false> st{slots + v, stride, 0};
        VGate::W<VStore<false>> gate{&st, true};
        if (stage == 0) S0::visit(g, gate); else if (stage == 1) S1::visit(g, gate); else S2::visit(g, gate);
    }
#ifdef FD_TSP_STAGE_CLOCKS
    if (blockIdx.x == 0 && lane == 0)
        printf("tsp_clocks wave %d stage %d part %d busy %llu of %llu\n", w, stage, part, busy, (unsigned long long)(__builtin_amdgcn_s_memtime() - clk0));
#endif
}

template <class G, int K, int TABLE>
__global__ __launch_bounds__((64 * Ts3pRoles<K, TABLE>::WAVES)) void k_render_ts3p(float* __restrict__ slots, size_t stride, size_t V,
                                                                                 float* __restrict__ out, size_t T, const void* aux) {
    if constexpr (TspPlan<G>::ok) render_ts3p_body<G, K, TABLE>(slots, stride, V, out, T, aux);
}

// the shipped shape (DESIGN.md 6.21 has what was measured); a build may override them to measure another
#ifndef FD_TSP_K
#define FD_TSP_K 2
#endif
#ifndef FD_TSP_ROLES
#define FD_TSP_ROLES 0
#endif

template <class G>
void launch_tsp(const RenderPlan& p, const RenderArgs& a) {
    static_assert(TspPlan<G>::ok, "k_render_ts3p: oscillator | oscillator | FixedSvf chains only");
    hipLaunchKernelGGL((k_render_ts3p<G, FD_TSP_K, FD_TSP_ROLES>), dim3(p.grid), dim3(64 * Ts3pRoles<FD_TSP_K, FD_TSP_ROLES>::WAVES), 0, a.s, a.slots,
                       a.stride, a.V, a.out, a.T, a.aux);
}

}  // namespace fd
