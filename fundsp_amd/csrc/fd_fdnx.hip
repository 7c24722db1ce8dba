// fd_fdnx.hip -- filtered / per-instance Hadamard feedback delay networks, lane = frame (see fd_fdnx.hpp).  Compiled with
// -fgpu-flush-denormals-to-zero like fd_fdn.hip: Feedback::new and Feedback2::new call prevent_denormals() (feedback.rs:96, :220).
#include <cmath>

#include "fd_fdnx.hpp"
#include "fd_fdn_frames.hpp"
#include "fd_line_table.hpp"   // (fd_nodes.hpp: SvfCore, host + device)
#include "fd_opts.hpp"

namespace fd {

int fdnx_make_table(const FdnxDesc& d, size_t instances, double sample_rate, std::vector<FdnxInst>& tab, FdnxConst* c) {
    const LineSpan span = line_table_fill(d, instances, sample_rate, tab);
    if (span.shortest < 0) return -1;
    const int N = d.lines, cap = line_ring_cap(span.longest);
    *c = FdnxConst{};
    c->lines = N;
    c->taps = d.taps;
    c->nin = d.nin;
    c->nout = d.nout;
    c->filter = d.filter;
    c->place = d.place;
    c->has_gain = d.has_gain;
    c->cap = cap;
    c->had_scale = (float)(1.0 / std::sqrt((double)N));
    c->ring_stride = (size_t)N * ((size_t)cap + 64);
    c->tab_stride = d.per_instance ? 1 : 0;
    c->tab = nullptr;
    return span.shortest - 1;
}

// the lines' parameters of this kernel: a row of the device table (wave-uniform: scalar loads)
struct FdnxLines {
    const FdnxInst* __restrict__ tp;
    __device__ __forceinline__ int len(int k) const { return tp->len[k]; }
    __device__ __forceinline__ float w(int j, int k) const { return tp->w[j][k]; }
};

// One wave per instance, lane = frame; NL lines (2 .. 32), K FIR taps (0 = no Fir node).  The steps of fd_fdn_frames.hpp with per-line
// weights, and between the FIR and the Hadamard the filter, the gain and the place.  The filter kind, its place and the gain are
// wave-uniform run-time values (c.filter, c.place, c.has_gain): one branch per block each.
template <int NL, int K>
__global__ __launch_bounds__(256) void k_fdn_frames_filtered(FdnxConst c, FdnxState s, size_t V, const float* __restrict__ in,
                                                             float* __restrict__ out, size_t T, size_t fstride, int layout, int tick_mode, FdnBus bus) {
    static_assert(K >= 0 && K <= 3 && NL >= 2 && NL <= 32 && (NL & (NL - 1)) == 0, "filtered FDN: 2..32 lines (a power of two), FIR order 0..3");
    __shared__ float hist_all[4][NL * HS];  // per line: the K - 1 carried delay outputs | d[0..63]
    __shared__ float fbr_all[4][NL * HS];   // per line: fb[-1] | fb[0..63]; before the Hadamard, [4..67] carries the filter's 64 frames
    const int lane = threadIdx.x & 63, wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* hist = hist_all[wib];
    float* fbr = fbr_all[wib];
    const size_t inst = (size_t)blockIdx.x * 4 + wib;
    if (inst >= V) return;
    const FdnxInst* __restrict__ tp = c.tab + inst * c.tab_stride;
    const FdnxLines p{tp};
    const FdnOut io{out, V, T, fstride, inst, layout, lane};
    const int nin = c.nin, nout = c.nout, filter = c.filter;
    const bool loop = c.place == FDNX_IN_LOOP, gained = c.has_gain != 0;
    const int CMASK = c.cap - 1;
    const __amdgpu_buffer_rsrc_t rings = fdn_rings(s, inst, c.ring_stride);
    const int lane4 = lane * 4;
    int wp = __builtin_amdgcn_readfirstlane(s.wpos[inst]);
    // the serial lanes (lane = line): this line's filter coefficients and state
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
        // The block's input frames (zeros past a ragged end).  The same four lines stand in k_fdn_frames_generic (fd_fdn.hip): a fix to one
        // is a fix to both.  Not a shared step: as a function it compiled to another shape (profiles/fdn_frames_shared_isa.txt).
        const int sizen = fdn_block_size(T, t0n);
#pragma unroll
        for (int ch = 0; ch < 2; ch++)
            xin[ch] = (ch < nin && lane < sizen) ? (layout == 0 ? in[((size_t)ch * T + t0n + lane) * V + inst] : in[(inst * nin + ch) * fstride + t0n + lane]) : 0.0f;
    };
    fetch(0, wp);
    for (size_t t0 = 0; t0 < T; t0 += 64) {
        const int size = fdn_block_size(T, t0);
        float d[NL];
        const float x0 = xin[0], x1 = xin[1];   // this block's input frames, by channel
        const float xi1 = nin == 2 ? x1 : x0;   // line k takes input channel k % nin
#pragma unroll
        for (int k = 0; k < NL; k++) d[k] = dn[k];
        if (t0 + 64 < T) fetch(t0 + 64, (wp + 64) & CMASK);
        float o[NL], f[NL];
        // fdn_fir_lines and (below) fdn_feedback_put with their LDS row stores in place: inside the shared functions those two store loops
        // cost <16, 3> and <32, 3> of THIS kernel one and two VGPRs (profiles/fdn_frames_shared_isa.txt).  Fir::tick itself is the shared one.
        if (K > 1) {   // lane n writes slot n + K - 1, then reads the K - 1 slots before its own
#pragma unroll
            for (int k = 0; k < NL; k++) hist[k * HS + K - 1 + lane] = d[k];
            fdn_wave_sync();
        }
#pragma unroll
        for (int k = 0; k < NL; k++) o[k] = fdn_fir<K>(hist + k * HS + lane, d[k], p.w(0, k), p.w(1, k), p.w(2, k));
#pragma unroll
        for (int k = 0; k < NL; k++) f[k] = o[k];
        if (filter != FDNX_NONE) {
            // lane = frame -> lane = line: each of lanes 0 .. NL-1 runs its line's 64-step recurrence in registers
#pragma unroll
            for (int k = 0; k < NL; k++) fbr[k * HS + 4 + lane] = o[k];
            fdn_wave_sync();
            // (in place in the LDS row: the lane = frame part keeps 4 x NL values live across this)
            if (serial) fdn_filter_walk(fbr + lane * HS + 4, filter == FDNX_SVF, svf, pc, pomc, size);
            fdn_wave_sync();
#pragma unroll
            for (int k = 0; k < NL; k++) f[k] = fbr[k * HS + 4 + lane];
            fdn_wave_sync();   // (the Hadamard rows below overwrite [1..64])
        }
        if (gained) {
#pragma unroll
            for (int k = 0; k < NL; k++) f[k] = f[k] * tp->g[k];   // Unop<F, FrameMulScalar>: x * scalar (audionode.rs:1190-1228)
        }
        if (!loop) {   // Feedback: the output is the filtered line.  Feedback2: the line before y
#pragma unroll
            for (int k = 0; k < NL; k++) o[k] = f[k];
        }
        fdn_hadamard<NL>(f);
#pragma unroll
        for (int k = 0; k < NL; k++) fbr[k * HS + 1 + lane] = f[k] * c.had_scale;   // the feedback of frame n -> row slot n + 1
        fdn_wave_sync();
        float xw[NL];
        fdn_ring_input<0, NL>(xw, fbr, lane, x0, xi1);
        fdn_ring_store(xw, rings, lane, lane4, c.cap, wp, size);
        float y0, y1;
        fdn_join<NL>(o, nout, tick_mode, y0, y1);
        fdn_output_store(io, nout, t0, size, bus, y0, y1, x0, x1);
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

void fdnx_launch_render(const FdnxConst& c, const FdnxState& s, size_t instances, const float* in, float* out, size_t T, size_t fstride,
                        int layout, int tick_mode, hipStream_t stream, const FdnBus& bus) {
    if (instances == 0 || T == 0) return;
    tl_opts.last_kernel = LK_FDN_FRAMES;
    FD_FDN_FRAMES_LAUNCH(k_fdn_frames_filtered, 0, c.lines, c.taps, instances, stream, c, s, instances, in, out, T, fstride, layout, tick_mode, bus);
}

}  // namespace fd
