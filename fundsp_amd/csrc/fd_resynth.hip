// fd_resynth.hip -- resynthesizer banks (fd_resynth.hpp): batched FFT frames + window-ordered overlap-add.
// Built twice: fd_resynth.o with IEEE denormals (namespace rs_ieee, plus the host tables) and fd_resynth_ftz.o with
// -fgpu-flush-denormals-to-zero -DFD_FTZ=1 (namespace rs_ftz).
#include <cmath>

#include "fd_fft.hpp"
#include "fd_math.hpp"
#include "fd_resynth.hpp"
#include "../../include/fundsp_hip.h"

#if FD_FTZ
#define FD_RS_NS rs_ftz
#else
#define FD_RS_NS rs_ieee
#endif

namespace fd {

#if !FD_FTZ
void rs_tables(int N, float* hann, float* hz, float* tw) {
    const float z = 2.0f / 3.0f;   // resynth.rs:310
    for (int i = 0; i < N; i++) {
        const float h = 0.5f + 0.5f * cosf_musl((float)(i - (N >> 1)) * F32_TAU / (float)N);
        if (hann) hann[i] = h;
        if (hz) hz[i] = h * z;
    }
    if (tw)
        for (int j = 0; j < N / 2; j++) {   // the expression of cfft_inplace (fd_capi.hip) at span N, k = j
            const double ang = 6.283185307179586476925286766559 * (double)j / (double)N;
            tw[2 * j] = (float)std::cos(ang);
            tw[2 * j + 1] = (float)-std::sin(ang);
        }
}
#endif

namespace FD_RS_NS {
namespace {

// chunk input -> input ring (raw samples)
__global__ void k_rs_input(RsConst c, RsState st, size_t V, const float* __restrict__ in, size_t T, size_t t0, int L, size_t fs, int layout) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = V * (size_t)c.I * L;
    if (idx >= n) return;
    const unsigned long long S = *st.samples;
    size_t v, t, ch;
    float x;
    if (layout == FDSP_LAYOUT_PLANAR) {   // [v][c][fs]: t fastest
        t = idx % L;
        const size_t r = idx / L;
        ch = r % c.I;
        v = r / c.I;
        x = in[(v * c.I + ch) * fs + t0 + t];
    } else {                              // [c][T][V]: v fastest
        v = idx % V;
        const size_t r = idx / V;
        t = r % L;
        ch = r / L;
        x = in[(ch * T + t0 + t) * V + v];
    }
    st.xin[(v * c.I + ch) * (size_t)c.Rx + ((S + t) & (unsigned long long)(c.Rx - 1))] = x;
}

// one unit per (new frame f, instance v, output o); P lanes per unit, G units per 256-lane workgroup
template <int LOGN>
__global__ __launch_bounds__(256) void k_rs_frames(RsConst c, RsState st, size_t V, int L, int Fmax) {
    constexpr int N = 1 << LOGN, NH = N / 2, P = NH < 256 ? NH : 256, G = 256 / P, NB = (NH + P) / P;
    __shared__ Cf lds[G * N];
    const int lane = threadIdx.x % P, g = threadIdx.x / P;
    const size_t unit = (size_t)blockIdx.x * G + g;
    const int O = c.O;
    const int o = (int)(unit % O);
    const size_t v = (unit / O) % V;
    const size_t f = unit / ((size_t)O * V);
    const unsigned long long S = *st.samples;
    constexpr int H = N / 4;
    const unsigned long long k = S / H + 1 + f;
    const bool live = f < (size_t)Fmax && k * H <= S + (unsigned long long)L && k >= 4;
    const int src = c.src[o];
    const int ch = src < 0 ? 0 : src;
    const size_t row = c.rows == 1 ? 0 : v;
    Cf* buf = lds + g * N;
    const float* __restrict__ xr = st.xin + (v * c.I + ch) * (size_t)c.Rx;
    const unsigned long long x0 = k * H - N;
    const unsigned long long xm = (unsigned long long)(c.Rx - 1);
    // windowed input packed as z[m] = x[2m] + i x[2m+1], bit-reversed for the N/2-point transform
    for (int m = lane; m < NH; m += P) {
        const int p = 2 * m;
        const float a = xr[(x0 + p) & xm] * c.hann[p];
        const float b = xr[(x0 + p + 1) & xm] * c.hann[p + 1];
        buf[bitrev(m, LOGN - 1)] = Cf{a, b};
    }
    __syncthreads();
    for (int ls = 1; ls <= LOGN - 1; ls++) {
        stage<P>(buf, NH, ls, N, LOGN, c.tw, lane);
        __syncthreads();
    }
    // split into bins 0 .. N/2, then the processor
    Cf y[NB];
#pragma unroll
    for (int r = 0; r < NB; r++) {
        const int b = lane + r * P;
        if (b > NH) break;
        const Cf X = rfft_bin(buf, b, NH, c.tw);
        Cf Y{0.0f, 0.0f};
        if (src >= 0) {
            if (c.proc == RS_PASS) {
                Y = X;
            } else if (c.proc == RS_BAND) {
                const float fr = *st.fstep * (float)b;
                const float2 lh = c.band[row * O + o];
                if (lh.x <= fr && fr <= lh.y) Y = X;
            } else {
                const float gv = c.gain[(row * O + o) * (size_t)(NH + 1) + b];
                Y = Cf{X.re * gv, X.im * gv};
            }
        }
        y[r] = Y;
    }
    __syncthreads();
    // fix_negative + the inverse's reversal of elements 1 .. N-1, written bit-reversed for the N-point transform
#pragma unroll
    for (int r = 0; r < NB; r++) {
        const int b = lane + r * P;
        if (b > NH) break;
        ifft_store_bin(buf, b, y[r], LOGN);
    }
    __syncthreads();
    for (int ls = 1; ls <= LOGN; ls++) {
        stage<P>(buf, N, ls, N, LOGN, c.tw, lane);
        __syncthreads();
    }
    if (live) {
        float* __restrict__ dst = st.frames + ((v * c.R + (size_t)(k % (unsigned long long)c.R)) * O + o) * (size_t)N;
        for (int p = lane; p < N; p += P) dst[p] = buf[p].re * c.invN;
    }
}

// The closure path (fd_resynth_fn.hpp) cuts k_rs_frames at the spectra, with the same device functions in the same order.
// one unit per (new frame f, instance v, INPUT ch): the forward half -> X [v][f][ch][bin]
template <int LOGN>
__global__ __launch_bounds__(256) void k_rs_forward(RsConst c, RsState st, float2* __restrict__ X, int Fc, size_t V, int L, int Fmax) {
    constexpr int N = 1 << LOGN, NH = N / 2, P = NH < 256 ? NH : 256, G = 256 / P, NB = (NH + P) / P;
    __shared__ Cf lds[G * NH];
    const int lane = threadIdx.x % P, g = threadIdx.x / P;
    const size_t unit = (size_t)blockIdx.x * G + g;
    const int I = c.I;
    const int ch = (int)(unit % I);
    const size_t v = (unit / I) % V;
    const size_t f = unit / ((size_t)I * V);
    const unsigned long long S = *st.samples;
    constexpr int H = N / 4;
    const unsigned long long k = S / H + 1 + f;
    const bool live = f < (size_t)Fmax && k * H <= S + (unsigned long long)L && k >= 4;
    Cf* buf = lds + g * NH;
    const float* __restrict__ xr = st.xin + (v * I + ch) * (size_t)c.Rx;
    const unsigned long long x0 = k * H - N;
    const unsigned long long xm = (unsigned long long)(c.Rx - 1);
    for (int m = lane; m < NH; m += P) {
        const int p = 2 * m;
        const float a = xr[(x0 + p) & xm] * c.hann[p];
        const float b = xr[(x0 + p + 1) & xm] * c.hann[p + 1];
        buf[bitrev(m, LOGN - 1)] = Cf{a, b};
    }
    __syncthreads();
    for (int ls = 1; ls <= LOGN - 1; ls++) {
        stage<P>(buf, NH, ls, N, LOGN, c.tw, lane);
        __syncthreads();
    }
    if (!live) return;   // (no barrier follows)
    float2* __restrict__ dst = X + ((v * Fc + f) * I + ch) * (size_t)(NH + 1);
#pragma unroll
    for (int r = 0; r < NB; r++) {
        const int b = lane + r * P;
        if (b > NH) break;
        const Cf Xb = rfft_bin(buf, b, NH, c.tw);
        dst[b] = float2{Xb.re, Xb.im};
    }
}

// one unit per (new frame f, instance v, OUTPUT o): Y [v][f][o][bin] -> the inverse half -> the frame ring
template <int LOGN>
__global__ __launch_bounds__(256) void k_rs_inverse(RsConst c, RsState st, const float2* __restrict__ Y, int Fc, size_t V, int L, int Fmax) {
    constexpr int N = 1 << LOGN, NH = N / 2, P = NH < 256 ? NH : 256, G = 256 / P, NB = (NH + P) / P;
    __shared__ Cf lds[G * N];
    const int lane = threadIdx.x % P, g = threadIdx.x / P;
    const size_t unit = (size_t)blockIdx.x * G + g;
    const int O = c.O;
    const int o = (int)(unit % O);
    const size_t v = (unit / O) % V;
    const size_t f = unit / ((size_t)O * V);
    const unsigned long long S = *st.samples;
    constexpr int H = N / 4;
    const unsigned long long k = S / H + 1 + f;
    const bool live = f < (size_t)Fmax && k * H <= S + (unsigned long long)L && k >= 4;
    Cf* buf = lds + g * N;
    const float2* __restrict__ src = Y + ((v * Fc + (live ? f : 0)) * O + o) * (size_t)(NH + 1);   // (a unit without a frame reads frame 0: in bounds, unused)
#pragma unroll
    for (int r = 0; r < NB; r++) {
        const int b = lane + r * P;
        if (b > NH) break;
        const float2 y = src[b];
        ifft_store_bin(buf, b, Cf{y.x, y.y}, LOGN);
    }
    __syncthreads();
    for (int ls = 1; ls <= LOGN; ls++) {
        stage<P>(buf, N, ls, N, LOGN, c.tw, lane);
        __syncthreads();
    }
    if (live) {
        float* __restrict__ dst = st.frames + ((v * c.R + (size_t)(k % (unsigned long long)c.R)) * O + o) * (size_t)N;
        for (int p = lane; p < N; p += P) dst[p] = buf[p].re * c.invN;
    }
}

// one lane per (instance, output, sample): ((((0 + f_w0) + f_w1) + f_w2) + f_w3), frame k in window (-k) mod 4
__global__ void k_rs_ola(RsConst c, RsState st, size_t V, int L, float* __restrict__ out, size_t T, size_t t0, size_t fs, int layout) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int O = c.O;
    const size_t n = V * (size_t)O * L;
    if (idx >= n) return;
    size_t v, t, o;
    if (layout == FDSP_LAYOUT_PLANAR) {
        t = idx % L;
        const size_t r = idx / L;
        o = r % O;
        v = r / O;
    } else {
        v = idx % V;
        const size_t r = idx / V;
        t = r % L;
        o = r / L;
    }
    const unsigned long long S = *st.samples;
    const unsigned long long tg = S + t;
    const int logH = c.logN - 2;
    const unsigned long long m = tg >> logH;
    float acc = 0.0f;
    for (int w = 0; w < 4; w++) {
        const long long k = (long long)m - (long long)((m + w) & 3ull);
        if (k < 4) continue;   // the window is still empty: out_w[idx].re * hz = 0 * hz adds +0.0 to a sum that is never -0.0
        const unsigned p = (unsigned)(tg - ((unsigned long long)k << logH));
        acc = acc + st.frames[((v * c.R + (size_t)(k % (unsigned long long)c.R)) * O + o) * (size_t)c.N + p] * c.hz[p];
    }
    if (layout == FDSP_LAYOUT_PLANAR) out[(v * O + o) * fs + t0 + t] = acc;
    else out[(o * T + t0 + t) * V + v] = acc;
}

__global__ void k_rs_advance(RsState st, int L) { *st.samples += (unsigned long long)L; }

template <int LOGN>
void launch_frames(const RsConst& c, const RsState& st, size_t V, int L, int Fmax, hipStream_t s) {
    constexpr int N = 1 << LOGN, NH = N / 2, P = NH < 256 ? NH : 256, G = 256 / P;
    const size_t units = (size_t)Fmax * V * c.O;
    hipLaunchKernelGGL(k_rs_frames<LOGN>, dim3((unsigned)((units + G - 1) / G)), dim3(256), 0, s, c, st, V, L, Fmax);
}

template <int LOGN>
void launch_forward(const RsConst& c, const RsState& st, const RsFn& fn, size_t V, int L, int Fmax, hipStream_t s) {
    constexpr int N = 1 << LOGN, NH = N / 2, P = NH < 256 ? NH : 256, G = 256 / P;
    const size_t units = (size_t)Fmax * V * c.I;
    hipLaunchKernelGGL(k_rs_forward<LOGN>, dim3((unsigned)((units + G - 1) / G)), dim3(256), 0, s, c, st, fn.x, fn.Fc, V, L, Fmax);
}
template <int LOGN>
void launch_inverse(const RsConst& c, const RsState& st, const RsFn& fn, size_t V, int L, int Fmax, hipStream_t s) {
    constexpr int N = 1 << LOGN, NH = N / 2, P = NH < 256 ? NH : 256, G = 256 / P;
    const size_t units = (size_t)Fmax * V * c.O;
    hipLaunchKernelGGL(k_rs_inverse<LOGN>, dim3((unsigned)((units + G - 1) / G)), dim3(256), 0, s, c, st, (const float2*)fn.y, fn.Fc, V, L, Fmax);
}

#define FD_RS_BY_LOGN(call)                   \
    switch (c.logN) {                         \
        case 2: call<2>(c, st, fn, V, L, Fmax, s); break;   \
        case 3: call<3>(c, st, fn, V, L, Fmax, s); break;   \
        case 4: call<4>(c, st, fn, V, L, Fmax, s); break;   \
        case 5: call<5>(c, st, fn, V, L, Fmax, s); break;   \
        case 6: call<6>(c, st, fn, V, L, Fmax, s); break;   \
        case 7: call<7>(c, st, fn, V, L, Fmax, s); break;   \
        case 8: call<8>(c, st, fn, V, L, Fmax, s); break;   \
        case 9: call<9>(c, st, fn, V, L, Fmax, s); break;   \
        case 10: call<10>(c, st, fn, V, L, Fmax, s); break; \
        case 11: call<11>(c, st, fn, V, L, Fmax, s); break; \
        case 12: call<12>(c, st, fn, V, L, Fmax, s); break; \
        default: call<13>(c, st, fn, V, L, Fmax, s); break; \
    }

}  // namespace

// a closure bank's launch: k_rs_frames' place is taken by forward -> the module's rs_process -> inverse (c.Lmax = (fn.Fc - 1) * H)
void rs_launch_render_fn(const RsConst& c, const RsState& st, const RsFn& fn, size_t V, const float* in, float* out, size_t T, size_t fs, int layout, hipStream_t s) {
    const int H = c.N / 4, NB = c.N / 2 + 1;
    for (size_t t0 = 0; t0 < T; t0 += (size_t)c.Lmax) {
        const int L = (int)(T - t0 < (size_t)c.Lmax ? T - t0 : (size_t)c.Lmax);
        const int Fmax = L / H + 1;   // frames completing in (S, S + L]: at most fn.Fc
        const size_t ni = V * (size_t)c.I * L, no = V * (size_t)c.O * L;
        hipLaunchKernelGGL(k_rs_input, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, s, c, st, V, in, T, t0, L, fs, layout);
        FD_RS_BY_LOGN(launch_forward)
        RsFnArgs a{fn.x, fn.y, fn.params, fn.state, st.samples, st.fstep, fn.srf, (unsigned long long)V, c.N, c.I, c.O, fn.P, fn.Fc, L, Fmax};
        const size_t lanes = V * (size_t)NB * (fn.S > 0 ? 1 : Fmax);
        void* args[] = {&a};
        hipModuleLaunchKernel(fn.process, (unsigned)((lanes + 255) / 256), 1, 1, 256, 1, 1, 0, s, args, nullptr);
        FD_RS_BY_LOGN(launch_inverse)
        hipLaunchKernelGGL(k_rs_ola, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, s, c, st, V, L, out, T, t0, fs, layout);
        hipLaunchKernelGGL(k_rs_advance, dim3(1), dim3(1), 0, s, st, L);
    }
}
#undef FD_RS_BY_LOGN

void rs_launch_render(const RsConst& c, const RsState& st, size_t V, const float* in, float* out, size_t T, size_t fs, int layout, hipStream_t s) {
    const int H = c.N / 4;
    for (size_t t0 = 0; t0 < T; t0 += (size_t)c.Lmax) {
        const int L = (int)(T - t0 < (size_t)c.Lmax ? T - t0 : (size_t)c.Lmax);
        const int Fmax = L / H + 1;   // frames completing in (S, S + L]
        const size_t ni = V * (size_t)c.I * L, no = V * (size_t)c.O * L;
        hipLaunchKernelGGL(k_rs_input, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, s, c, st, V, in, T, t0, L, fs, layout);
        switch (c.logN) {
            case 2: launch_frames<2>(c, st, V, L, Fmax, s); break;
            case 3: launch_frames<3>(c, st, V, L, Fmax, s); break;
            case 4: launch_frames<4>(c, st, V, L, Fmax, s); break;
            case 5: launch_frames<5>(c, st, V, L, Fmax, s); break;
            case 6: launch_frames<6>(c, st, V, L, Fmax, s); break;
            case 7: launch_frames<7>(c, st, V, L, Fmax, s); break;
            case 8: launch_frames<8>(c, st, V, L, Fmax, s); break;
            case 9: launch_frames<9>(c, st, V, L, Fmax, s); break;
            case 10: launch_frames<10>(c, st, V, L, Fmax, s); break;
            case 11: launch_frames<11>(c, st, V, L, Fmax, s); break;
            case 12: launch_frames<12>(c, st, V, L, Fmax, s); break;
            default: launch_frames<13>(c, st, V, L, Fmax, s); break;
        }
        hipLaunchKernelGGL(k_rs_ola, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, s, c, st, V, L, out, T, t0, fs, layout);
        hipLaunchKernelGGL(k_rs_advance, dim3(1), dim3(1), 0, s, st, L);
    }
}

}  // namespace FD_RS_NS
}  // namespace fd
