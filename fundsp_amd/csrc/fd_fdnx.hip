// fd_fdnx.hip -- filtered / per-instance Hadamard feedback delay networks, lane = frame (see fd_fdnx.hpp).  Compiled with
// -fgpu-flush-denormals-to-zero like fd_fdn.hip: Feedback::new and Feedback2::new call prevent_denormals() (feedback.rs:96, :220).
#include <cmath>

#include "fd_fdnx.hpp"
#include "fd_opts.hpp"
#include "fd_math.hpp"
#include "fd_nodes.hpp"   // svf_coefs, SvfCore (host + device)

namespace fd {

int fdnx_make_table(const FdnxDesc& d, size_t instances, double sample_rate, std::vector<FdnxInst>& tab, FdnxConst* c) {
    const size_t P = d.per_instance ? instances : 1;
    const int N = d.lines;
    tab.assign(P, FdnxInst{});
    const float sr = (float)sample_rate;   // the filters' coefficients are computed in F = f32 (filter.rs:35-38, svf.rs:236-239)
    int maxlen = 0, shortest = 1 << 30;
    for (size_t p = 0; p < P; p++) {
        FdnxInst& e = tab[p];
        for (int k = 0; k < N; k++) {
            const size_t i = p * N + k;
            e.len[k] = (int)std::round(d.delay[i] * sample_rate) + 1;   // Delay::new / set_sample_rate (delay.rs:104-112)
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
    }
    int cap = 256;
    while (cap < maxlen) cap <<= 1;
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
    return cap > (1 << 18) ? -1 : shortest;
}

constexpr int XS = 68;  // floats per LDS row: [0] carry-in | [1..64] this block (fb rows) | [4..67] the filter hand-over (16-byte aligned)

__global__ __launch_bounds__(256) void k_fdnx_reset(FdnxConst c, FdnxState s, size_t instances) {
    // Feedback(2)::reset (feedback.rs:123-126, 248-252): the rings, the Fir carry, the filters and the feedback value
    const size_t total = instances * c.ring_stride;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) s.rings[i] = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < instances * 32; i += (size_t)gridDim.x * 256) {
        if (i < instances) s.wpos[i] = 0;
        s.v1[i] = 0.0f;
        s.v2[i] = 0.0f;
        s.fb[i] = 0.0f;
        s.s1[i] = 0.0f;
        s.s2[i] = 0.0f;
    }
}

__device__ __forceinline__ void fdnx_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave per instance, lane = frame; NL lines (2 .. 32), K FIR taps (0 = no Fir node).  The filter kind, its place and the gain are
// wave-uniform run-time values (c.filter, c.place, c.has_gain): one branch per block each.
template <int NL, int K>
__global__ __launch_bounds__(256) void k_fdn_frames_filtered(FdnxConst c, FdnxState s, size_t V, const float* __restrict__ in,
                                                             float* __restrict__ out, size_t T, size_t fstride, int layout, int tick_mode, FdnBus bus) {
    static_assert(K >= 0 && K <= 3 && NL >= 2 && NL <= 32 && (NL & (NL - 1)) == 0, "filtered FDN: 2..32 lines (a power of two), FIR order 0..3");
    constexpr int H0 = K >= 2 ? K - 1 : 0;  // carried delay outputs per line: Fir::v[1 .. K-1]
    __shared__ float hist_all[4][NL * XS];  // per line: the H0 carried delay outputs | d[0..63]
    __shared__ float fbr_all[4][NL * XS];   // per line: fb[-1] | fb[0..63]; before the Hadamard, [4..67] carries the filter's 64 frames
    const int lane = threadIdx.x & 63, wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* hist = hist_all[wib];
    float* fbr = fbr_all[wib];
    const size_t inst = (size_t)blockIdx.x * 4 + wib;
    if (inst >= V) return;
    const FdnxInst* __restrict__ tp = c.tab + inst * c.tab_stride;
    const float scale = c.had_scale;
    const int nin = c.nin, nout = c.nout, filter = c.filter;
    const bool loop = c.place == FDNX_IN_LOOP, gained = c.has_gain != 0;
    const int CMASK = c.cap - 1, CP = c.cap + 64;
    const __amdgpu_buffer_rsrc_t rings = __builtin_amdgcn_make_buffer_rsrc(s.rings + inst * c.ring_stride, 0, (int)(c.ring_stride * sizeof(float)), 0x00020000);
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
    if (serial) {  // carry-in: Fir::v[1..K-1] (v1 = the older, v2 = the newer), Feedback::value
        if (K == 3) hist[lane * XS + 0] = s.v1[inst * 32 + lane];
        if (K >= 2) hist[lane * XS + H0 - 1] = s.v2[inst * 32 + lane];
        fbr[lane * XS + 0] = s.fb[inst * 32 + lane];
    }
    float dn[NL], xin[2];
    auto fetch = [&](size_t t0n, int wpn) {
        const int sizen = (int)((T - t0n) < 64 ? (T - t0n) : 64);
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int r = (wpn - (tp->len[k] - 1)) & CMASK;   // frame 0 reads the slot written len - 1 frames ago; 64 contiguous slots (mirror zone)
            dn[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rings, lane4, (k * CP + r) * 4, 0));
        }
#pragma unroll
        for (int ch = 0; ch < 2; ch++)
            xin[ch] = (ch < nin && lane < sizen) ? (layout == 0 ? in[((size_t)ch * T + t0n + lane) * V + inst] : in[(inst * nin + ch) * fstride + t0n + lane]) : 0.0f;
    };
    fetch(0, wp);
    for (size_t t0 = 0; t0 < T; t0 += 64) {
        const int size = (int)((T - t0) < 64 ? (T - t0) : 64);
        float d[NL];
        const float xi0 = xin[0], xi1 = nin == 2 ? xin[1] : xin[0];
        const float xin_now[2] = {xin[0], xin[1]};
#pragma unroll
        for (int k = 0; k < NL; k++) d[k] = dn[k];
        if (t0 + 64 < T) fetch(t0 + 64, (wp + 64) & CMASK);
        if (K > 1) {
#pragma unroll
            for (int k = 0; k < NL; k++) hist[k * XS + H0 + lane] = d[k];
            fdnx_wave_sync();
        }
        float o[NL], f[NL];
#pragma unroll
        for (int k = 0; k < NL; k++) {  // Fir::tick fir.rs:57-70: the sum starts at 0.0 and takes the taps oldest first, per-line weights
            float acc = 0.0f;
            if (K == 3) {
                acc += tp->w[0][k] * hist[k * XS + lane];
                acc += tp->w[1][k] * hist[k * XS + lane + 1];
                acc += tp->w[2][k] * d[k];
            } else if (K == 2) {
                acc += tp->w[0][k] * hist[k * XS + lane];
                acc += tp->w[1][k] * d[k];
            } else if (K == 1) {
                acc += tp->w[0][k] * d[k];
            } else {
                acc = d[k];   // no Fir node
            }
            o[k] = acc;
            f[k] = acc;
        }
        if (filter != FDNX_NONE) {
            // lane = frame -> lane = line: each of lanes 0 .. NL-1 runs its line's 64-step recurrence in registers
#pragma unroll
            for (int k = 0; k < NL; k++) fbr[k * XS + 4 + lane] = o[k];
            fdnx_wave_sync();
            if (serial) {
                // in place in the LDS row, eight frames at a time: the loads do not depend on the recurrence and run ahead of it, and the
                // 64 frames never sit in registers at once (the lane = frame part keeps 4 x NL values live across this)
                float* row = fbr + lane * XS + 4;
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
            fdnx_wave_sync();
#pragma unroll
            for (int k = 0; k < NL; k++) f[k] = fbr[k * XS + 4 + lane];
            fdnx_wave_sync();   // (the Hadamard rows below overwrite [1..64])
        }
        if (gained) {
#pragma unroll
            for (int k = 0; k < NL; k++) f[k] = f[k] * tp->g[k];   // Unop<F, FrameMulScalar>: x * scalar (audionode.rs:1190-1228)
        }
        if (!loop) {   // Feedback: the output is the filtered line.  Feedback2: the line before y
#pragma unroll
            for (int k = 0; k < NL; k++) o[k] = f[k];
        }
#pragma unroll
        for (int st = 1; st < NL; st <<= 1)  // FrameHadamard feedback.rs:35-57
#pragma unroll
            for (int i = 0; i < NL; i++)
                if ((i & st) == 0) {
                    const float x = f[i], y = f[i + st];
                    f[i] = x + y;
                    f[i + st] = x - y;
                }
#pragma unroll
        for (int k = 0; k < NL; k++) fbr[k * XS + 1 + lane] = f[k] * scale;
        fdnx_wave_sync();
        float xw[NL];  // Feedback::tick: input + value (feedback.rs:130-134, 260-261)
#pragma unroll
        for (int k = 0; k < NL; k++) xw[k] = ((k & 1) ? xi1 : xi0) + fbr[k * XS + lane];
        if (size == 64 && wp >= 64 && wp + 64 <= c.cap) {
#pragma unroll
            for (int k = 0; k < NL; k++)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, xw[k]), rings, lane4, (k * CP + wp) * 4, 0);
        } else if (lane < size) {  // wrap, mirror zone or ragged tail
            const int pos = (wp + lane) & CMASK;
#pragma unroll
            for (int k = 0; k < NL; k++) {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, xw[k]), rings, pos * 4, k * CP * 4, 0);
                if (pos < 64) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, xw[k]), rings, (c.cap + pos) * 4, k * CP * 4, 0);
            }
        }
        // Join<N> / MultiJoin<M, N/M>: channel j over lines j, j + nout, ..
        float y0, y1 = 0.0f;
        if (nout == 1) {
            if (tick_mode) {
                y0 = o[0];
#pragma unroll
                for (int i = 1; i < NL; i++) y0 += o[i];
                y0 = y0 / (float)NL;
            } else {
                const float z = 1.0f / (float)NL;
                y0 = o[0] * z;
#pragma unroll
                for (int i = 1; i < NL; i++) y0 += o[i] * z;
            }
        } else {
            if (tick_mode) {
                y0 = o[0]; y1 = o[1];
#pragma unroll
                for (int i = 1; i < NL / 2; i++) { y0 += o[2 * i]; y1 += o[2 * i + 1]; }
                y0 = y0 / (float)(NL / 2); y1 = y1 / (float)(NL / 2);
            } else {
                const float z = 1.0f / (float)(NL / 2);
                y0 = o[0] * z; y1 = o[1] * z;
#pragma unroll
                for (int i = 1; i < NL / 2; i++) { y0 += o[2 * i] * z; y1 += o[2 * i + 1] * z; }
            }
        }
        if (bus.mode) {  // wet * network [& dry * multipass()] (fd_fdn.hpp FdnBus; mode 2: nin == nout)
            y0 = fdn_bus(bus, y0, xin_now[0]);
            y1 = fdn_bus(bus, y1, xin_now[1]);
        }
        if (lane < size) {
            if (layout == 0) {
                out[((size_t)0 * T + t0 + lane) * V + inst] = y0;
                if (nout == 2) out[((size_t)1 * T + t0 + lane) * V + inst] = y1;
            } else {
                out[(inst * nout + 0) * fstride + t0 + lane] = y0;
                if (nout == 2) out[(inst * nout + 1) * fstride + t0 + lane] = y1;
            }
        }
        fdnx_wave_sync();
        if (serial) {  // the block's last delay outputs and feedback value become the next block's carry-in
            float a = 0.0f, b = 0.0f;
            if (K == 3) { a = hist[lane * XS + size]; b = hist[lane * XS + size + 1]; }
            if (K == 2) b = hist[lane * XS + size];
            const float fv = fbr[lane * XS + size];
            if (K == 3) hist[lane * XS + 0] = a;
            if (K >= 2) hist[lane * XS + H0 - 1] = b;
            fbr[lane * XS + 0] = fv;
        }
        wp = (wp + size) & CMASK;
        fdnx_wave_sync();
    }
    if (lane == 0) s.wpos[inst] = wp;
    if (serial) {
        if (K == 3) s.v1[inst * 32 + lane] = hist[lane * XS + 0];
        if (K >= 2) s.v2[inst * 32 + lane] = hist[lane * XS + H0 - 1];
        s.fb[inst * 32 + lane] = fbr[lane * XS + 0];
        if (filter != FDNX_NONE) {
            s.s1[inst * 32 + lane] = svf.ic1eq;
            s.s2[inst * 32 + lane] = svf.ic2eq;
        }
    }
}

template <int NL>
static void fdnx_launch(const FdnxConst& c, const FdnxState& s, size_t instances, const float* in, float* out, size_t T, size_t fstride, int layout,
                        int tick_mode, hipStream_t stream, const FdnBus& bus) {
    const dim3 grid((unsigned)((instances + 3) / 4)), block(256);
    switch (c.taps) {
    case 3: hipLaunchKernelGGL((k_fdn_frames_filtered<NL, 3>), grid, block, 0, stream, c, s, instances, in, out, T, fstride, layout, tick_mode, bus); break;
    case 2: hipLaunchKernelGGL((k_fdn_frames_filtered<NL, 2>), grid, block, 0, stream, c, s, instances, in, out, T, fstride, layout, tick_mode, bus); break;
    case 1: hipLaunchKernelGGL((k_fdn_frames_filtered<NL, 1>), grid, block, 0, stream, c, s, instances, in, out, T, fstride, layout, tick_mode, bus); break;
    default: hipLaunchKernelGGL((k_fdn_frames_filtered<NL, 0>), grid, block, 0, stream, c, s, instances, in, out, T, fstride, layout, tick_mode, bus); break;
    }
}

void fdnx_launch_reset(const FdnxConst& c, const FdnxState& s, size_t instances, hipStream_t stream) {
    hipLaunchKernelGGL(k_fdnx_reset, dim3(2048), dim3(256), 0, stream, c, s, instances);
}

void fdnx_launch_render(const FdnxConst& c, const FdnxState& s, size_t instances, const float* in, float* out, size_t T, size_t fstride,
                        int layout, int tick_mode, hipStream_t stream, const FdnBus& bus) {
    if (instances == 0 || T == 0) return;
    tl_opts.last_kernel = LK_FDN_FRAMES;
    switch (c.lines) {
    case 2: return fdnx_launch<2>(c, s, instances, in, out, T, fstride, layout, tick_mode, stream, bus);
    case 4: return fdnx_launch<4>(c, s, instances, in, out, T, fstride, layout, tick_mode, stream, bus);
    case 8: return fdnx_launch<8>(c, s, instances, in, out, T, fstride, layout, tick_mode, stream, bus);
    case 16: return fdnx_launch<16>(c, s, instances, in, out, T, fstride, layout, tick_mode, stream, bus);
    default: return fdnx_launch<32>(c, s, instances, in, out, T, fstride, layout, tick_mode, stream, bus);
    }
}

}  // namespace fd
