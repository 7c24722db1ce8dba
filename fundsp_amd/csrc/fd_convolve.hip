// fd_convolve.hip -- convolver banks (fd_convolve.hpp): uniformly partitioned FFT convolution, complete blocks only, direct head.
// Built twice: fd_convolve.o with IEEE denormals (namespace cv_ieee, plus the host's block-length rule) and fd_convolve_ftz.o with
// -fgpu-flush-denormals-to-zero -DFD_FTZ=1 (namespace cv_ftz).
#include "fd_convolve.hpp"
#include "fd_fft.hpp"
#include "../../include/fundsp_hip.h"

#if FD_FTZ
#define FD_CV_NS cv_ftz
#else
#define FD_CV_NS cv_ieee
#endif

namespace fd {

#if !FD_FTZ
int cv_block_length(size_t max_len) {
    int B = 1 << CV_MIN_LOGB;
    while (B < (1 << CV_MAX_LOGB) && (size_t)B * B < 8 * max_len) B <<= 1;
    return B;
}
#endif

namespace FD_CV_NS {
namespace {

typedef unsigned long long u64;

// chunk input -> input ring
__global__ void k_cv_input(CvConst c, CvState st, size_t V, const float* __restrict__ in, size_t T, size_t t0, int L, size_t fs, int layout) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = V * (size_t)c.C * L;
    if (idx >= n) return;
    const u64 S = *st.samples;
    size_t v, t, ch;
    float x;
    if (layout == FDSP_LAYOUT_PLANAR) {   // [v][c][fs]: t fastest
        t = idx % L;
        const size_t r = idx / L;
        ch = r % c.C;
        v = r / c.C;
        x = in[(v * c.C + ch) * fs + t0 + t];
    } else {                              // [c][T][V]: v fastest
        v = idx % V;
        const size_t r = idx / V;
        t = r % L;
        ch = r / L;
        x = in[(ch * T + t0 + t) * V + v];
    }
    st.xin[(v * c.C + ch) * (size_t)c.Rx + ((S + t) & (u64)(c.Rx - 1))] = x;
}

// rfft_N of N = 2B real values, B-point working set in LDS; P lanes per unit, G units per 256-lane workgroup.
// RESP = false: unit (f, instance, channel) -- the block that completes f-th in the chunk, followed by B zeros -> spectrum ring.
// RESP = true:  unit (p, row * C + channel) of rows [row0, ..) -- g_p of the stored taps -> response spectra.
template <int LOGB, bool RESP>
__global__ __launch_bounds__(256) void k_cv_forward(CvConst c, CvState st, size_t units, size_t inner, int L, size_t row0) {
    constexpr int B = 1 << LOGB, N = 2 * B, P = B < 256 ? B : 256, G = 256 / P, NB = (B + P) / P;
    __shared__ Cf lds[G * B];
    const int lane = threadIdx.x % P, g = threadIdx.x / P;
    const size_t unit = (size_t)blockIdx.x * G + g;
    const bool in_range = unit < units;
    const size_t vc = in_range ? unit % inner : 0;   // instance * C + channel, or (row - row0) * C + channel
    const size_t f = in_range ? unit / inner : 0;
    Cf* buf = lds + g * B;
    bool live = in_range;
    float2* dst;
    if (RESP) {
        const float* __restrict__ hr = c.h + (row0 * c.C + vc) * c.Hcap + f * B;   // h[pB ..]: g_p[i] = hr[B + i] (i < B), hr[i - B] (i > B)
        for (int m = lane; m < B; m += P) {
            const int i = 2 * m;
            const int o = i < B ? B + i : i - B;
            buf[bitrev(m, LOGB)] = Cf{i == B ? 0.0f : hr[o], hr[o + 1]};   // g_p[B] = 0: no output of the first B reads it
        }
        dst = (float2*)c.G + ((row0 * c.C + vc) * c.Pcap + f) * (size_t)(B + 1);
    } else {
        const u64 S = *st.samples;
        const u64 jb = S / B + f;
        live = live && (jb + 1) * B <= S + (u64)L;
        const float* __restrict__ xr = st.xin + vc * (size_t)c.Rx;
        const u64 x0 = jb * B, xm = (u64)(c.Rx - 1);
        for (int m = lane; m < B; m += P) {
            Cf z{0.0f, 0.0f};
            if (m < B / 2) z = Cf{xr[(x0 + 2 * m) & xm], xr[(x0 + 2 * m + 1) & xm]};
            buf[bitrev(m, LOGB)] = z;
        }
        dst = st.spec + (vc * c.R + (size_t)(jb % (u64)c.R)) * (size_t)(B + 1);
    }
    __syncthreads();
    for (int ls = 1; ls <= LOGB; ls++) {
        stage<P>(buf, B, ls, N, LOGB + 1, c.tw, lane);
        __syncthreads();
    }
    if (!live) return;
#pragma unroll
    for (int r = 0; r < NB; r++) {
        const int b = lane + r * P;
        if (b > B) break;
        const Cf X = rfft_bin(buf, b, B, c.tw);
        dst[b] = make_float2(X.re, X.im);
    }
}

// The hot kernel: Z_j'[k] = sum over p (increasing from zero) of X_{j'-1-p}[k] * G_p[k] for the boundaries j' reached in the chunk.
// A lane owns bin k of one (instance, channel) for CV_J consecutive boundaries (blockIdx.y picks the group).  Step s loads block
// btop - s once and G_s once; sum jj takes it as its term p = s - (CV_J - 1 - jj), so every sum sees p = 0, 1, 2, .. in order.  The
// conditions depend on the group and the step only: they are uniform over the workgroup.
__global__ __launch_bounds__(256) void k_cv_tail(CvConst c, CvState st, size_t V, int L) {
    constexpr int J = CV_J;
    const int B1 = c.B + 1;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= V * (size_t)c.C * B1) return;
    const int k = (int)(idx % B1);
    const size_t vc = idx / B1;
    const u64 S = *st.samples;
    const int P = st.dims[1];
    const long long j0 = (long long)(S / (u64)c.B);
    const int nb = (int)((long long)((S + (u64)L) / (u64)c.B) - j0);   // boundaries j0 + 1 .. j0 + nb
    const int bi0 = (int)blockIdx.y * J;
    if (bi0 >= nb) return;
    const long long jbase = j0 + 1 + bi0;
    const long long btop = jbase + J - 2;
    const size_t row = c.rows == 1 ? 0 : vc / c.C;
    const float2* __restrict__ Gr = c.G + ((row * c.C + vc % c.C) * c.Pcap) * (size_t)B1 + k;
    const float2* __restrict__ Xr = st.spec + vc * c.R * (size_t)B1 + k;
    Cf acc[J], gw[J];
#pragma unroll
    for (int jj = 0; jj < J; jj++) acc[jj] = Cf{0.0f, 0.0f}, gw[jj] = Cf{0.0f, 0.0f};
    for (int s0 = 0; s0 < P + J - 1; s0 += J) {
#pragma unroll
        for (int u = 0; u < J; u++) {
            const int s = s0 + u;
            if (s < P) {
                const float2 gv = Gr[(size_t)s * B1];
                gw[u] = Cf{gv.x, gv.y};
            }
            const long long b = btop - s;
            Cf X{0.0f, 0.0f};
            if (b >= 0 && b < j0 + nb) {
                const float2 xv = Xr[(size_t)((u64)b % (u64)c.R) * B1];
                X = Cf{xv.x, xv.y};
            }
#pragma unroll
            for (int jj = 0; jj < J; jj++) {
                const int q = J - 1 - jj;
                const int p = s - q;
                if (bi0 + jj < nb && p >= 0 && p < P && b >= 0) {
                    const Cf g = gw[(u - q + J) % J];
                    const float pr = X.re * g.re - X.im * g.im, pi = X.re * g.im + X.im * g.re;
                    acc[jj] = Cf{acc[jj].re + pr, acc[jj].im + pi};
                }
            }
        }
    }
    float2* __restrict__ Z = st.zbuf + (vc * c.KB + bi0) * (size_t)B1 + k;
#pragma unroll
    for (int jj = 0; jj < J; jj++)
        if (bi0 + jj < nb) Z[(size_t)jj * B1] = make_float2(acc[jj].re, acc[jj].im);
}

// irfft_N of Z, one unit per (boundary of the chunk, instance, channel), N complex values in LDS; the first B real values -> pend ring
template <int LOGB>
__global__ __launch_bounds__(256) void k_cv_inverse(CvConst c, CvState st, size_t V, int L, int Fmax) {
    constexpr int B = 1 << LOGB, N = 2 * B, LOGN = LOGB + 1, P = B < 256 ? B : 256, G = 256 / P, NB = (B + P) / P;
    __shared__ Cf lds[G * N];
    const int lane = threadIdx.x % P, g = threadIdx.x / P;
    const size_t unit = (size_t)blockIdx.x * G + g;
    const size_t VC = V * (size_t)c.C;
    const bool in_range = unit < VC * Fmax;
    const size_t vc = in_range ? unit % VC : 0;
    const int bi = in_range ? (int)(unit / VC) : 0;   // < Fmax <= KB
    const u64 S = *st.samples;
    const u64 j0 = S / B;
    const int nb = (int)((S + (u64)L) / B - j0);
    const bool live = in_range && bi < nb;
    Cf* buf = lds + g * N;
    const float2* __restrict__ Z = st.zbuf + (vc * c.KB + bi) * (size_t)(B + 1);
#pragma unroll
    for (int r = 0; r < NB; r++) {
        const int b = lane + r * P;
        if (b > B) break;
        const float2 z = Z[b];
        ifft_store_bin(buf, b, Cf{z.x, z.y}, LOGN);
    }
    __syncthreads();
    for (int ls = 1; ls <= LOGN; ls++) {
        stage<P>(buf, N, ls, N, LOGN, c.tw, lane);
        __syncthreads();
    }
    if (!live) return;
    const u64 j = j0 + 1 + bi;
    float* __restrict__ dst = st.pend + (vc * (c.KB + 1) + (size_t)(j % (u64)(c.KB + 1))) * (size_t)B;
    for (int r = lane; r < B; r += P) dst[r] = buf[r].re * c.invN;
}

// y[n] = pend_j[r] + head[n]: one workgroup per (instance, channel, tile of blockDim.x = min(B, 256) samples aligned to the absolute count,
// so a tile lies inside one block); the block's inputs up to the tile's end and as many taps are staged in LDS (2 * B floats at most)
__global__ void k_cv_output(CvConst c, CvState st, size_t V, int L, int ntiles, float* __restrict__ out, size_t T, size_t t0, size_t fs, int layout) {
    extern __shared__ float cv_lds[];
    const int TS = blockDim.x, B = c.B;
    const size_t vc = blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles;
    const u64 S = *st.samples;
    const int M = st.dims[0];
    const u64 n0 = (S / TS + tile) * TS;
    const u64 j = n0 / B;
    const int r0 = (int)(n0 % B);
    const int cnt = r0 + TS;   // <= B
    float* xs = cv_lds;
    float* hs = cv_lds + B;
    const size_t ch = vc % c.C, v = vc / c.C;
    const float* __restrict__ xr = st.xin + vc * (size_t)c.Rx;
    const float* __restrict__ hr = c.h + ((c.rows == 1 ? 0 : v) * c.C + ch) * c.Hcap;
    const u64 xm = (u64)(c.Rx - 1);
    for (int i = threadIdx.x; i < cnt; i += TS) {
        xs[i] = xr[(j * B + i) & xm];
        hs[i] = hr[i];
    }
    __syncthreads();
    const u64 n = n0 + threadIdx.x;
    if (n < S || n >= S + (u64)L) return;
    const int r = r0 + threadIdx.x;
    const int imax = r < M - 1 ? r : M - 1;
    float a = hs[0] * xs[r];
    for (int i = 1; i <= imax; i++) a = a + hs[i] * xs[r - i];
    const float pend = j == 0 ? 0.0f : st.pend[(vc * (c.KB + 1) + (size_t)(j % (u64)(c.KB + 1))) * (size_t)B + r];
    const float y = pend + a;
    const size_t t = (size_t)(n - S);
    if (layout == FDSP_LAYOUT_PLANAR) out[vc * fs + t0 + t] = y;
    else out[(ch * T + t0 + t) * V + v] = y;
}

__global__ void k_cv_advance(CvState st, int L) { *st.samples += (u64)L; }

template <int LOGB, bool RESP>
void launch_forward(const CvConst& c, const CvState& st, size_t outer, size_t inner, int L, size_t row0, hipStream_t s) {
    constexpr int B = 1 << LOGB, P = B < 256 ? B : 256, G = 256 / P;
    const size_t units = outer * inner;
    if (units == 0) return;
    hipLaunchKernelGGL((k_cv_forward<LOGB, RESP>), dim3((unsigned)((units + G - 1) / G)), dim3(256), 0, s, c, st, units, inner, L, row0);
}
template <bool RESP>
void forward(const CvConst& c, const CvState& st, size_t outer, size_t inner, int L, size_t row0, hipStream_t s) {
    switch (c.logB) {
        case 6: launch_forward<6, RESP>(c, st, outer, inner, L, row0, s); break;
        case 7: launch_forward<7, RESP>(c, st, outer, inner, L, row0, s); break;
        case 8: launch_forward<8, RESP>(c, st, outer, inner, L, row0, s); break;
        case 9: launch_forward<9, RESP>(c, st, outer, inner, L, row0, s); break;
        case 10: launch_forward<10, RESP>(c, st, outer, inner, L, row0, s); break;
        case 11: launch_forward<11, RESP>(c, st, outer, inner, L, row0, s); break;
        default: launch_forward<12, RESP>(c, st, outer, inner, L, row0, s); break;
    }
}
template <int LOGB>
void launch_inverse(const CvConst& c, const CvState& st, size_t V, int L, int Fmax, hipStream_t s) {
    constexpr int B = 1 << LOGB, P = B < 256 ? B : 256, G = 256 / P;
    const size_t units = V * (size_t)c.C * Fmax;
    hipLaunchKernelGGL(k_cv_inverse<LOGB>, dim3((unsigned)((units + G - 1) / G)), dim3(256), 0, s, c, st, V, L, Fmax);
}

}  // namespace

void cv_launch_render(const CvConst& c, const CvState& st, size_t V, const float* in, float* out, size_t T, size_t fs, int layout, hipStream_t s) {
    const size_t Lmax = (size_t)c.KB * c.B, VC = V * (size_t)c.C;
    const int TS = c.B < 256 ? c.B : 256;
    for (size_t t0 = 0; t0 < T; t0 += Lmax) {
        const int L = (int)(T - t0 < Lmax ? T - t0 : Lmax);
        const int Fmax = L / c.B + 1 < c.KB ? L / c.B + 1 : c.KB;   // blocks that can complete in (S, S + L]
        const size_t ni = VC * L;
        hipLaunchKernelGGL(k_cv_input, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, s, c, st, V, in, T, t0, L, fs, layout);
        forward<false>(c, st, (size_t)Fmax, VC, L, 0, s);
        const size_t nz = VC * (size_t)(c.B + 1);
        hipLaunchKernelGGL(k_cv_tail, dim3((unsigned)((nz + 255) / 256), (unsigned)((Fmax + CV_J - 1) / CV_J)), dim3(256), 0, s, c, st, V, L);
        switch (c.logB) {
            case 6: launch_inverse<6>(c, st, V, L, Fmax, s); break;
            case 7: launch_inverse<7>(c, st, V, L, Fmax, s); break;
            case 8: launch_inverse<8>(c, st, V, L, Fmax, s); break;
            case 9: launch_inverse<9>(c, st, V, L, Fmax, s); break;
            case 10: launch_inverse<10>(c, st, V, L, Fmax, s); break;
            case 11: launch_inverse<11>(c, st, V, L, Fmax, s); break;
            default: launch_inverse<12>(c, st, V, L, Fmax, s); break;
        }
        const int ntiles = L / TS + 2;   // tiles of TS samples that (S, S + L] can touch
        hipLaunchKernelGGL(k_cv_output, dim3((unsigned)(VC * ntiles)), dim3(TS), 2 * c.B * sizeof(float), s, c, st, V, L, ntiles, out, T, t0, fs, layout);
        hipLaunchKernelGGL(k_cv_advance, dim3(1), dim3(1), 0, s, st, L);
    }
}

void cv_launch_response(const CvConst& c, size_t row0, size_t nrows, hipStream_t s) {
    forward<true>(c, CvState{}, (size_t)c.Pcap, nrows * c.C, 0, row0, s);
}

}  // namespace FD_CV_NS
}  // namespace fd
