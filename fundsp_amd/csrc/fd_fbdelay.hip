// fd_fbdelay.hip -- feedback delay banks (echo, comb, ping-pong), lane = frame (see fd_fbdelay.hpp).  Compiled with
// -fgpu-flush-denormals-to-zero like fd_fdnx.hip: Feedback::new and Feedback2::new call prevent_denormals() (feedback.rs:96, :220).
#include <cmath>

#include "fd_fbdelay.hpp"
#include "fd_fdn_frames.hpp"
#include "fd_line_table.hpp"   // (fd_nodes.hpp: SvfCore, host + device)
#include "fd_opts.hpp"

namespace fd {

int fb_make_table(const FdnxDesc& d, size_t instances, double sample_rate, std::vector<FbInst>& tab, FbConst* c) {
    const LineSpan span = line_table_fill(d, instances, sample_rate, tab);
    if (span.shortest < 0) return -1;
    const int N = d.lines, cap = line_ring_cap(span.longest);
    for (size_t p = 0; p < tab.size(); p++) {
        if (N == 1) tab[p].len[1] = tab[p].len[0];
        tab[p].outer = d.has_outer ? d.outer[p] : 1.0f;
    }
    *c = FbConst{};
    c->lines = N;
    c->taps = d.taps;
    c->filter = d.filter;
    c->place = d.place;
    c->has_gain = d.has_gain;
    c->has_outer = d.has_outer;
    c->reverse = N == 2 ? d.reverse : 0;
    c->cap = cap;
    c->ring_stride = (size_t)N * ((size_t)cap + 64);
    c->tab_stride = d.per_instance ? 1 : 0;
    c->tab = nullptr;
    return span.shortest - 1;
}

// the lines' parameters of this kernel: a row of the device table (wave-uniform: scalar loads)
struct FbLines {
    const FbInst* __restrict__ tp;
    __device__ __forceinline__ int len(int k) const { return tp->len[k]; }
    __device__ __forceinline__ float w(int j, int k) const { return tp->w[j][k]; }
};

// One wave per instance, lane = frame; NL channels (1 | 2), K FIR taps (0 = no Fir node).  The steps of fd_fdn_frames.hpp; where the Hadamard
// networks have their butterflies and the scale, the permutation and the outer gain -- the result goes into the feedback row as it is.  The
// filter kind, its place, the gains and the permutation are wave-uniform run-time values: one branch per block each.
template <int NL, int K>
__global__ __launch_bounds__(256) void k_fb_frames(FbConst c, FdnxState s, size_t V, const float* __restrict__ in, float* __restrict__ out, size_t T,
                                                   size_t fstride, int layout, FdnBus bus) {
    static_assert(K >= 0 && K <= 3 && (NL == 1 || NL == 2), "feedback delay: 1 or 2 channels, FIR order 0..3");
    __shared__ float hist_all[4][NL * HS];  // per channel: the K - 1 carried delay outputs | d[0..63]
    __shared__ float fbr_all[4][NL * HS];   // per channel: fb[-1] | fb[0..63]; before that, [4..67] carries the filter's 64 frames
    const int lane = threadIdx.x & 63, wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* hist = hist_all[wib];
    float* fbr = fbr_all[wib];
    const size_t inst = (size_t)blockIdx.x * 4 + wib;
    if (inst >= V) return;
    const FbInst* __restrict__ tp = c.tab + inst * c.tab_stride;
    const FbLines p{tp};
    const FdnOut io{out, V, T, fstride, inst, layout, lane};
    const int filter = c.filter;
    const bool loop = c.place == FDNX_IN_LOOP, gained = c.has_gain != 0, outer = c.has_outer != 0, rev = NL == 2 && c.reverse != 0;
    const int CMASK = c.cap - 1;
    const __amdgpu_buffer_rsrc_t rings = fdn_rings(s, inst, c.ring_stride);
    const int lane4 = lane * 4;
    int wp = __builtin_amdgcn_readfirstlane(s.wpos[inst]);
    // the serial lanes (lane = channel): this channel's filter coefficients and state
    const bool serial = lane < NL;
    const int sl = serial ? lane : 0;
    SvfCore svf;
    svf.a1 = tp->co[0][sl]; svf.a2 = tp->co[1][sl]; svf.a3 = tp->co[2][sl];
    svf.m0 = tp->co[3][sl]; svf.m1 = tp->co[4][sl]; svf.m2 = tp->co[5][sl];
    svf.ic1eq = serial ? s.s1[inst * 32 + sl] : 0.0f;
    svf.ic2eq = serial ? s.s2[inst * 32 + sl] : 0.0f;
    const float pc = svf.a1, pomc = svf.a2;   // Lowpole: coeff, 1 - coeff
    if (serial) fdn_state_load<K>(s, inst, lane, hist, fbr);
    float dn[NL], xin[2];
    auto fetch = [&](size_t t0n, int wpn) {
        fdn_ring_fetch(dn, rings, lane4, c.cap, wpn, p);
        // the block's input frames, channel = line (zeros past a ragged end)
        const int sizen = fdn_block_size(T, t0n);
#pragma unroll
        for (int ch = 0; ch < 2; ch++)
            xin[ch] = (ch < NL && lane < sizen) ? (layout == 0 ? in[((size_t)ch * T + t0n + lane) * V + inst] : in[(inst * NL + ch) * fstride + t0n + lane]) : 0.0f;
    };
    // p_c = o_perm(c), then the outer gain (Unop<.., FrameMulScalar> around the body or around reverse(): x * scalar)
    auto permute = [&](float (&f)[NL]) {
        if (NL == 2 && rev) { const float a = f[0]; f[0] = f[NL - 1]; f[NL - 1] = a; }
        if (outer) {
#pragma unroll
            for (int k = 0; k < NL; k++) f[k] = f[k] * tp->outer;
        }
    };
    fetch(0, wp);
    for (size_t t0 = 0; t0 < T; t0 += 64) {
        const int size = fdn_block_size(T, t0);
        float d[NL];
        const float x0 = xin[0], x1 = xin[1];   // this block's input frames, by channel
#pragma unroll
        for (int k = 0; k < NL; k++) d[k] = dn[k];
        if (t0 + 64 < T) fetch(t0 + 64, (wp + 64) & CMASK);
        float o[NL], f[NL];
        fdn_fir_lines<NL, K>(f, d, hist, lane, p);
        if (loop) {   // Feedback2: the output is x's, the line [reversed]; y filters what goes back
            permute(f);
#pragma unroll
            for (int k = 0; k < NL; k++) o[k] = f[k];
        }
        if (filter != FDNX_NONE) {
            // lane = frame -> lane = channel: each of lanes 0 .. NL-1 runs its channel's 64-step recurrence in registers
#pragma unroll
            for (int k = 0; k < NL; k++) fbr[k * HS + 4 + lane] = f[k];
            fdn_wave_sync();
            if (serial) fdn_filter_walk(fbr + lane * HS + 4, filter == FDNX_SVF, svf, pc, pomc, size);
            fdn_wave_sync();
#pragma unroll
            for (int k = 0; k < NL; k++) f[k] = fbr[k * HS + 4 + lane];
            fdn_wave_sync();   // (the feedback rows below overwrite [1..64])
        }
        if (gained) {
#pragma unroll
            for (int k = 0; k < NL; k++) f[k] = f[k] * tp->g[k];   // Unop<F, FrameMulScalar>: x * scalar (audionode.rs:1190-1228)
        }
        if (!loop) {   // Feedback: the output and the feedback are the body's output
            permute(f);
#pragma unroll
            for (int k = 0; k < NL; k++) o[k] = f[k];
        }
        // FrameId::frame multiplies by nothing: the feedback of frame n goes to row slot n + 1 as it is
#pragma unroll
        for (int k = 0; k < NL; k++) fbr[k * HS + 1 + lane] = f[k];
        fdn_wave_sync();
        float xw[NL];
        fdn_ring_input<0, NL>(xw, fbr, lane, x0, x1);
        fdn_ring_store(xw, rings, lane, lane4, c.cap, wp, size);
        fdn_output_store(io, NL, t0, size, bus, o[0], o[NL - 1], x0, x1);
        fdn_block_carry<NL, K>(hist, fbr, lane, size);
        wp = (wp + size) & CMASK;
    }
    if (lane == 0) s.wpos[inst] = wp;
    if (serial) {
        fdn_state_store<K>(s, inst, lane, hist, fbr);
        if (filter != FDNX_NONE) {
            s.s1[inst * 32 + lane] = svf.ic1eq;
            s.s2[inst * 32 + lane] = svf.ic2eq;
        }
    }
}

void fb_launch_render(const FbConst& c, const FdnxState& s, size_t instances, const float* in, float* out, size_t T, size_t fstride, int layout,
                      hipStream_t stream, const FdnBus& bus) {
    if (instances == 0 || T == 0) return;
    tl_opts.last_kernel = LK_FDN_FRAMES;
    if (c.lines == 1) FD_FDN_FRAMES_TAPS(k_fb_frames, 1, 0, c.taps, instances, stream, c, s, instances, in, out, T, fstride, layout, bus);
    else FD_FDN_FRAMES_TAPS(k_fb_frames, 2, 0, c.taps, instances, stream, c, s, instances, in, out, T, fstride, layout, bus);
}

}  // namespace fd
