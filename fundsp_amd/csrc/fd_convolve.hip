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

void cv_set_routing(CvConst& c, int inputs, const int* source, bool fan) {
    c.I = inputs;
    for (int o = 0; o < CV_MAX_CH; o++) c.source[o] = o < c.C ? (source ? source[o] : o) : 0;
    c.NG = c.NG2 = 0;
    if (!fan) return;
    // the outputs of an input, in increasing order, in groups of CV_FAN; the full groups first, so that a launch sees one group size
    int full[CV_MAX_CH][CV_FAN], one[CV_MAX_CH], nfull = 0, none = 0;
    for (int i = 0; i < inputs; i++) {
        int n = 0, g[CV_FAN];
        for (int o = 0; o < c.C; o++) {
            if (c.source[o] != i) continue;
            g[n++] = o;
            if (n == CV_FAN) {
                for (int f = 0; f < CV_FAN; f++) full[nfull][f] = g[f];
                nfull++;
                n = 0;
            }
        }
        for (int f = 0; f < n; f++) one[none++] = g[f];   // (CV_FAN = 2: a remainder is one output)
    }
    c.NG2 = nfull;
    c.NG = nfull + none;
    for (int g = 0; g < c.NG; g++) {
        for (int f = 0; f < CV_FAN; f++) c.gout[g][f] = g < nfull ? full[g][f] : one[g - nfull];
        c.gsrc[g] = c.source[c.gout[g][0]];
    }
}
#endif

namespace FD_CV_NS {
namespace {

typedef unsigned long long u64;

// chunk input -> input ring, one row per (instance, input) (a plain bank has I = C)
__global__ void k_cv_input(CvConst c, CvState st, size_t V, const float* __restrict__ in, size_t T, size_t t0, int L, size_t fs, int layout) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = V * (size_t)c.I * L;
    if (idx >= n) return;
    const u64 S = *st.samples;
    size_t v, t, ch;
    float x;
    if (layout == FDSP_LAYOUT_PLANAR) {   // [v][i][fs]: t fastest
        t = idx % L;
        const size_t r = idx / L;
        ch = r % c.I;
        v = r / c.I;
        x = in[(v * c.I + ch) * fs + t0 + t];
    } else {                              // [i][T][V]: v fastest
        v = idx % V;
        const size_t r = idx / V;
        t = r % L;
        ch = r / L;
        x = in[(ch * T + t0 + t) * V + v];
    }
    st.xin[(v * c.I + ch) * (size_t)c.Rx + ((S + t) & (u64)(c.Rx - 1))] = x;
}

// rfft_N of N = 2B real values, B-point working set in LDS; P lanes per unit, G units per 256-lane workgroup.
// RESP = false: unit (f, instance, input) -- the block that completes f-th in the chunk, followed by B zeros -> spectrum ring.
// RESP = true:  unit (p, row * NT + response row) of rows [row0, ..) -- g_p of the stored taps -> response spectra.
template <int LOGB, bool RESP>
__global__ __launch_bounds__(256) void k_cv_forward(CvConst c, CvState st, size_t units, size_t inner, int L, size_t row0) {
    constexpr int B = 1 << LOGB, N = 2 * B, P = B < 256 ? B : 256, G = 256 / P, NB = (B + P) / P;
    __shared__ Cf lds[G * B];
    const int lane = threadIdx.x % P, g = threadIdx.x / P;
    const size_t unit = (size_t)blockIdx.x * G + g;
    const bool in_range = unit < units;
    const size_t vc = in_range ? unit % inner : 0;   // instance * I + input, or (row - row0) * NT + response row
    const size_t f = in_range ? unit / inner : 0;
    Cf* buf = lds + g * B;
    bool live = in_range;
    float2* dst;
    if (RESP) {
        const float* __restrict__ hr = c.h + (row0 * c.NT + vc) * c.Hcap + f * B;   // h[pB ..]: g_p[i] = hr[B + i] (i < B), hr[i - B] (i > B)
        for (int m = lane; m < B; m += P) {
            const int i = 2 * m;
            const int o = i < B ? B + i : i - B;
            buf[bitrev(m, LOGB)] = Cf{i == B ? 0.0f : hr[o], hr[o + 1]};   // g_p[B] = 0: no output of the first B reads it
        }
        dst = (float2*)c.G + ((row0 * c.NT + vc) * c.Pcap + f) * (size_t)(B + 1);
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
    const float2* __restrict__ Gr = c.G + ((row * c.NT + vc % c.C) * c.Pcap) * (size_t)B1 + k;
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

// The tail of a routed bank: k_cv_tail for the F outputs of a fan group at once.  A lane owns bin k of one (instance, group) -- blockIdx.z
// picks the group g0 + z, blockIdx.y the CV_J boundaries -- loads every X of the group's input ONCE and keeps F x CV_J sums and F windows of
// response bins in registers; output f's sums take exactly the terms, in exactly the order, that k_cv_tail gives them.  The conditions
// depend on the block indices and the step only: they are uniform over the workgroup, and the group's entries of `c` are scalar.
template <int F>
__global__ __launch_bounds__(256) void k_cv_tail_fan(CvConst c, CvState st, size_t V, int L, int g0) {
    constexpr int J = CV_J;
    const int B1 = c.B + 1;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= V * (size_t)B1) return;
    const int k = (int)(idx % B1);
    const size_t v = idx / B1;
    const int g = g0 + (int)blockIdx.z;
    const u64 S = *st.samples;
    const int P = st.dims[1];
    const long long j0 = (long long)(S / (u64)c.B);
    const int nb = (int)((long long)((S + (u64)L) / (u64)c.B) - j0);   // boundaries j0 + 1 .. j0 + nb
    const int bi0 = (int)blockIdx.y * J;
    if (bi0 >= nb) return;
    const long long jbase = j0 + 1 + bi0;
    const long long btop = jbase + J - 2;
    const size_t row = c.rows == 1 ? 0 : v;
    const float2* __restrict__ Xr = st.spec + (v * c.I + c.gsrc[g]) * c.R * (size_t)B1 + k;
    const float2* __restrict__ Gr[F];
    Cf acc[F][J], gw[F][J];
#pragma unroll
    for (int f = 0; f < F; f++) {
        Gr[f] = c.G + ((row * c.NT + c.gout[g][f]) * c.Pcap) * (size_t)B1 + k;
#pragma unroll
        for (int jj = 0; jj < J; jj++) acc[f][jj] = Cf{0.0f, 0.0f}, gw[f][jj] = Cf{0.0f, 0.0f};
    }
    for (int s0 = 0; s0 < P + J - 1; s0 += J) {
#pragma unroll
        for (int u = 0; u < J; u++) {
            const int s = s0 + u;
            if (s < P) {
#pragma unroll
                for (int f = 0; f < F; f++) {
                    const float2 gv = Gr[f][(size_t)s * B1];
                    gw[f][u] = Cf{gv.x, gv.y};
                }
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
#pragma unroll
                    for (int f = 0; f < F; f++) {
                        const Cf gg = gw[f][(u - q + J) % J];
                        const float pr = X.re * gg.re - X.im * gg.im, pi = X.re * gg.im + X.im * gg.re;
                        acc[f][jj] = Cf{acc[f][jj].re + pr, acc[f][jj].im + pi};
                    }
                }
            }
        }
    }
#pragma unroll
    for (int f = 0; f < F; f++) {
        float2* __restrict__ Z = st.zbuf + ((v * c.C + c.gout[g][f]) * c.KB + bi0) * (size_t)B1 + k;
#pragma unroll
        for (int jj = 0; jj < J; jj++)
            if (bi0 + jj < nb) Z[(size_t)jj * B1] = make_float2(acc[f][jj].re, acc[f][jj].im);
    }
}

// The tail of a summing bank: one Z per (instance, output), ONE running sum across the output's terms.  A lane owns bin k of one (instance,
// output) -- blockIdx.z picks the output, blockIdx.y the CV_J boundaries -- and keeps the CV_J sums in registers over all the terms; each
// term runs k_cv_tail's whole step loop with its own response spectra, its own input's spectrum ring and its own window of response bins,
// so sum jj takes term t's partitions p = 0, 1, 2, .. in order after every partition of the terms before it.  The conditions depend on
// the block indices, the term and the step only: they are uniform over the workgroup, and the term tables of `c` are scalar.
__global__ __launch_bounds__(256) void k_cv_tail_sum(CvConst c, CvState st, size_t V, int L) {
    constexpr int J = CV_J;
    const int B1 = c.B + 1;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= V * (size_t)B1) return;
    const int k = (int)(idx % B1);
    const size_t v = idx / B1;
    const int o = (int)blockIdx.z;
    const u64 S = *st.samples;
    const int P = st.dims[1];
    const long long j0 = (long long)(S / (u64)c.B);
    const int nb = (int)((long long)((S + (u64)L) / (u64)c.B) - j0);   // boundaries j0 + 1 .. j0 + nb
    const int bi0 = (int)blockIdx.y * J;
    if (bi0 >= nb) return;
    const long long jbase = j0 + 1 + bi0;
    const long long btop = jbase + J - 2;
    const size_t row = c.rows == 1 ? 0 : v;
    Cf acc[J];
#pragma unroll
    for (int jj = 0; jj < J; jj++) acc[jj] = Cf{0.0f, 0.0f};
    for (int t = c.tfirst[o]; t < c.tfirst[o + 1]; t++) {
        const float2* __restrict__ Gr = c.G + ((row * c.NT + t) * c.Pcap) * (size_t)B1 + k;
        const float2* __restrict__ Xr = st.spec + (v * c.I + c.tin[t]) * c.R * (size_t)B1 + k;
        Cf gw[J];
#pragma unroll
        for (int jj = 0; jj < J; jj++) gw[jj] = Cf{0.0f, 0.0f};
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
    }
    float2* __restrict__ Z = st.zbuf + ((v * c.C + o) * c.KB + bi0) * (size_t)B1 + k;
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
    const float* __restrict__ hr = c.h + ((c.rows == 1 ? 0 : v) * c.NT + ch) * c.Hcap;
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

// The head of a routed bank: k_cv_output for the F outputs of a fan group at once.  One workgroup per (instance, group g0 + blockIdx.y,
// tile); the block's input samples are staged once (xs, B floats) and the taps of the F outputs behind them (hs, F * B floats).  A lane
// computes the F heads of its sample, each in k_cv_output's order, from one read of every xs[r - i] (consecutive lanes, consecutive
// words) and F broadcast reads of the taps: F + 1 LDS reads per F multiply-adds.
template <int F>
__global__ void k_cv_output_fan(CvConst c, CvState st, size_t V, int L, int ntiles, int g0, float* __restrict__ out, size_t T, size_t t0, size_t fs,
                                int layout) {
    extern __shared__ float cv_lds[];
    const int TS = blockDim.x, B = c.B;
    const size_t v = blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles;
    const int g = g0 + (int)blockIdx.y;
    const u64 S = *st.samples;
    const int M = st.dims[0];
    const u64 n0 = (S / TS + tile) * TS;
    const u64 j = n0 / B;
    const int r0 = (int)(n0 % B);
    const int cnt = r0 + TS;   // <= B
    float* xs = cv_lds;
    float* hs = cv_lds + B;
    const float* __restrict__ xr = st.xin + (v * c.I + c.gsrc[g]) * (size_t)c.Rx;
    const u64 xm = (u64)(c.Rx - 1);
    size_t vc[F];
#pragma unroll
    for (int f = 0; f < F; f++) vc[f] = v * c.C + c.gout[g][f];
    for (int i = threadIdx.x; i < cnt; i += TS) xs[i] = xr[(j * B + i) & xm];
#pragma unroll
    for (int f = 0; f < F; f++) {
        const float* __restrict__ hr = c.h + ((c.rows == 1 ? 0 : v) * c.NT + c.gout[g][f]) * c.Hcap;
        for (int i = threadIdx.x; i < cnt; i += TS) hs[f * B + i] = hr[i];
    }
    __syncthreads();
    const u64 n = n0 + threadIdx.x;
    if (n < S || n >= S + (u64)L) return;
    const int r = r0 + threadIdx.x;
    const int imax = r < M - 1 ? r : M - 1;
    float a[F];
    const float x0 = xs[r];
#pragma unroll
    for (int f = 0; f < F; f++) a[f] = hs[f * B] * x0;
    for (int i = 1; i <= imax; i++) {
        const float xv = xs[r - i];
#pragma unroll
        for (int f = 0; f < F; f++) a[f] = a[f] + hs[f * B + i] * xv;
    }
    const size_t t = (size_t)(n - S);
#pragma unroll
    for (int f = 0; f < F; f++) {
        const float pend = j == 0 ? 0.0f : st.pend[(vc[f] * (c.KB + 1) + (size_t)(j % (u64)(c.KB + 1))) * (size_t)B + r];
        const float y = pend + a[f];
        if (layout == FDSP_LAYOUT_PLANAR) out[vc[f] * fs + t0 + t] = y;
        else out[((size_t)c.gout[g][f] * T + t0 + t) * V + v] = y;
    }
}

// The head of a summing bank: one workgroup per (instance, output blockIdx.y, tile).  LDS stays at 2 * B floats, so the workgroup walks the
// output's terms: stage the term's input samples and taps, barrier, every lane whose sample lies in [S, S + L) goes on with its ONE sum a in the
// contract's order, barrier before the next term overwrites the staging.  No lane leaves before the last barrier: the lanes outside the
// launch's samples stage and wait with the others and only skip the arithmetic and the store.  Consecutive terms of one input keep xs.
__global__ void k_cv_output_sum(CvConst c, CvState st, size_t V, int L, int ntiles, float* __restrict__ out, size_t T, size_t t0, size_t fs, int layout) {
    extern __shared__ float cv_lds[];
    const int TS = blockDim.x, B = c.B;
    const size_t v = blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles;
    const int o = (int)blockIdx.y;
    const u64 S = *st.samples;
    const int M = st.dims[0];
    const u64 n0 = (S / TS + tile) * TS;
    const u64 j = n0 / B;
    const int r0 = (int)(n0 % B);
    const int cnt = r0 + TS;   // <= B
    float* xs = cv_lds;
    float* hs = cv_lds + B;
    const u64 xm = (u64)(c.Rx - 1);
    const u64 n = n0 + threadIdx.x;
    const bool live = n >= S && n < S + (u64)L;
    const int r = r0 + threadIdx.x;
    const int imax = r < M - 1 ? r : M - 1;
    const int tA = c.tfirst[o], tB = c.tfirst[o + 1];
    float a = 0.0f;
    for (int t = tA; t < tB; t++) {
        const float* __restrict__ hr = c.h + ((c.rows == 1 ? 0 : v) * c.NT + t) * c.Hcap;
        if (t == tA || c.tin[t] != c.tin[t - 1]) {
            const float* __restrict__ xr = st.xin + (v * c.I + c.tin[t]) * (size_t)c.Rx;
            for (int i = threadIdx.x; i < cnt; i += TS) xs[i] = xr[(j * B + i) & xm];
        }
        for (int i = threadIdx.x; i < cnt; i += TS) hs[i] = hr[i];
        __syncthreads();
        if (live) {
            const float p0 = hs[0] * xs[r];
            a = t == tA ? p0 : a + p0;
            for (int i = 1; i <= imax; i++) a = a + hs[i] * xs[r - i];
        }
        __syncthreads();
    }
    if (!live) return;
    const size_t vo = v * c.C + o;
    const float pend = j == 0 ? 0.0f : st.pend[(vo * (c.KB + 1) + (size_t)(j % (u64)(c.KB + 1))) * (size_t)B + r];
    const float y = pend + a;
    const size_t t = (size_t)(n - S);
    if (layout == FDSP_LAYOUT_PLANAR) out[vo * fs + t0 + t] = y;
    else out[((size_t)o * T + t0 + t) * V + v] = y;
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
    const size_t Lmax = (size_t)c.KB * c.B, VC = V * (size_t)c.C, VI = V * (size_t)c.I;
    const int TS = c.B < 256 ? c.B : 256;
    const int n2 = c.NG2, n1 = c.NG - c.NG2;   // routed banks: the fan groups of CV_FAN outputs and of one (a summing bank: c.sum, per output)
    for (size_t t0 = 0; t0 < T; t0 += Lmax) {
        const int L = (int)(T - t0 < Lmax ? T - t0 : Lmax);
        const int Fmax = L / c.B + 1 < c.KB ? L / c.B + 1 : c.KB;   // blocks that can complete in (S, S + L]
        const size_t ni = VI * L;
        hipLaunchKernelGGL(k_cv_input, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, s, c, st, V, in, T, t0, L, fs, layout);
        forward<false>(c, st, (size_t)Fmax, VI, L, 0, s);
        const unsigned jg = (unsigned)((Fmax + CV_J - 1) / CV_J);
        if (c.sum) {
            const unsigned nx = (unsigned)((V * (size_t)(c.B + 1) + 255) / 256);
            hipLaunchKernelGGL(k_cv_tail_sum, dim3(nx, jg, (unsigned)c.C), dim3(256), 0, s, c, st, V, L);
        } else if (c.NG == 0) {
            const size_t nz = VC * (size_t)(c.B + 1);
            hipLaunchKernelGGL(k_cv_tail, dim3((unsigned)((nz + 255) / 256), jg), dim3(256), 0, s, c, st, V, L);
        } else {
            const unsigned nx = (unsigned)((V * (size_t)(c.B + 1) + 255) / 256);
            if (n2) hipLaunchKernelGGL(k_cv_tail_fan<CV_FAN>, dim3(nx, jg, (unsigned)n2), dim3(256), 0, s, c, st, V, L, 0);
            if (n1) hipLaunchKernelGGL(k_cv_tail_fan<1>, dim3(nx, jg, (unsigned)n1), dim3(256), 0, s, c, st, V, L, n2);
        }
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
        if (c.sum) {
            hipLaunchKernelGGL(k_cv_output_sum, dim3((unsigned)(V * ntiles), (unsigned)c.C), dim3(TS), 2 * c.B * sizeof(float), s, c, st, V, L, ntiles, out, T, t0, fs, layout);
        } else if (c.NG == 0) {
            hipLaunchKernelGGL(k_cv_output, dim3((unsigned)(VC * ntiles)), dim3(TS), 2 * c.B * sizeof(float), s, c, st, V, L, ntiles, out, T, t0, fs, layout);
        } else {
            const unsigned nx = (unsigned)(V * ntiles);
            if (n2)
                hipLaunchKernelGGL(k_cv_output_fan<CV_FAN>, dim3(nx, (unsigned)n2), dim3(TS), (1 + CV_FAN) * c.B * sizeof(float), s, c, st, V, L, ntiles, 0, out, T,
                                   t0, fs, layout);
            if (n1) hipLaunchKernelGGL(k_cv_output_fan<1>, dim3(nx, (unsigned)n1), dim3(TS), 2 * c.B * sizeof(float), s, c, st, V, L, ntiles, n2, out, T, t0, fs, layout);
        }
        hipLaunchKernelGGL(k_cv_advance, dim3(1), dim3(1), 0, s, st, L);
    }
}

void cv_launch_response(const CvConst& c, size_t row0, size_t nrows, hipStream_t s) {
    forward<true>(c, CvState{}, (size_t)c.Pcap, nrows * c.NT, 0, row0, s);
}

}  // namespace FD_CV_NS
}  // namespace fd
