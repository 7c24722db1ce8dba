// fd_fbdelay.hip -- feedback delay banks (echo, comb, ping-pong), lane = frame (see fd_fbdelay.hpp).  Compiled with
// -fgpu-flush-denormals-to-zero like fd_fdnx.hip: Feedback::new and Feedback2::new call prevent_denormals() (feedback.rs:96, :220).
#include <cmath>

#include "fd_fbdelay.hpp"
#include "fd_fdn_frames.hpp"
#include "fd_opts.hpp"
#include "fd_math.hpp"
#include "fd_nodes.hpp"   // svf_coefs, SvfCore (host + device)

namespace fd {

int fb_make_table(const FbDesc& d, size_t instances, double sample_rate, std::vector<FbInst>& tab, FbConst* c) {
    const size_t P = d.per_instance ? instances : 1;
    const int N = d.lines;
    tab.assign(P, FbInst{});
    const float sr = (float)sample_rate;   // the filters' coefficients are computed in F = f32 (filter.rs:35-38, svf.rs:236-239)
    int maxlen = 0, shortest = 1 << 30;
    for (size_t p = 0; p < P; p++) {
        FbInst& e = tab[p];
        for (int k = 0; k < N; k++) {
            const size_t i = p * N + k;
            const double samples = std::round(d.delay[i] * sample_rate);   // Delay::new / set_sample_rate (delay.rs:104-112)
            if (samples + 1.0 > (double)(1 << 18)) return -1;
            e.len[k] = (int)samples + 1;
            maxlen = e.len[k] > maxlen ? e.len[k] : maxlen;
            shortest = e.len[k] - 1 < shortest ? e.len[k] - 1 : shortest;
            for (int j = 0; j < d.taps; j++) e.w[j][k] = d.w[i * d.taps + j];
            if (d.filter == FDNX_LOWPOLE) {
                e.co[0][k] = expf_musl(-F32_TAU * d.cutoff[i] / sr);   // Lowpole::set_cutoff (filter.rs:35-38)
                e.co[1][k] = 1.0f - e.co[0][k];                         // (1 - coeff) as tick computes it (:65)
            } else if (d.filter == FDNX_SVF) {
                const SvfCoefs s = svf_coefs(d.svf_mode, sr, d.cutoff[i], d.q[i], d.gain.empty() ? 1.0f : d.gain[i]);
                e.co[0][k] = s.a1; e.co[1][k] = s.a2; e.co[2][k] = s.a3; e.co[3][k] = s.m0; e.co[4][k] = s.m1; e.co[5][k] = s.m2;
            }
            e.g[k] = d.has_gain ? d.line_gain[i] : 1.0f;
        }
        if (N == 1) e.len[1] = e.len[0];
        e.outer = d.has_outer ? d.outer[p] : 1.0f;
    }
    int cap = 256;
    while (cap < maxlen) cap <<= 1;
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
    return shortest;
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
            // lane = frame -> lane = channel: each of lanes 0 .. NL-1 runs its channel's 64-step recurrence in registers.  The same walk stands
            // in k_fdn_frames_filtered (fd_fdnx.hip): a fix to one is a fix to both.  Not a shared step: that kernel's code object stays as it is.
#pragma unroll
            for (int k = 0; k < NL; k++) fbr[k * HS + 4 + lane] = f[k];
            fdn_wave_sync();
            if (serial) {
                float* row = fbr + lane * HS + 4;
                if (filter == FDNX_SVF) {   // FixedSvf::tick, the reference's operations in the reference's order (svf.rs:995-1006)
#pragma unroll 8
                    for (int n = 0; n < 64; n++) {
                        const float i1 = svf.ic1eq, i2 = svf.ic2eq;
                        row[n] = svf.tick(row[n]);
                        if (n >= size) { svf.ic1eq = i1; svf.ic2eq = i2; }   // a ragged last block: the filter stops where the launch does
                    }
                } else {                    // Lowpole::tick: value = (1 - coeff) * x + coeff * value (filter.rs:64-66)
                    float v = svf.ic1eq;
#pragma unroll 8
                    for (int n = 0; n < 64; n++) {
                        const float a = pomc * row[n];
                        const float b = pc * v;
                        const float nv = a + b;
                        v = n < size ? nv : v;
                        row[n] = nv;
                    }
                    svf.ic1eq = v;
                }
            }
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
