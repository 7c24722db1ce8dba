// fd_fitness.hip -- reverb_fitness per instance on the device (see fd_fitness.hpp).  Built with the default IEEE flags: the score is
// evaluated on the rendered response like the reference's, outside any Feedback node's thread.
#include <vector>

#include "fd_fitness.hpp"
#include "fd_fft.hpp"
#include "fd_resynth.hpp"   // rs_tables

namespace fd {

void fit_make_tables(float* tables) { rs_tables(FIT_N, tables + FIT_N, nullptr, tables); }

namespace {

constexpr int FIT_P = 1024;   // lanes per row

__global__ __launch_bounds__(256) void k_fit_impulse(float* __restrict__ in, size_t rows) {
    const size_t total = rows * FIT_N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) in[i] = (i & (FIT_N - 1)) == 0 ? 1.0f : 0.0f;
}

// the 1 024 partial sums of the lanes -> red[0], by the tree of fd_fitness.hpp
__device__ __forceinline__ float fit_fold(float* red, int t, float v) {
    red[t] = v;
    __syncthreads();
    for (int s = FIT_P / 2; s >= 1; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// Complex32::norm (hypot), through f64: no overflow or underflow of the squares, one rounding to f32 at the end
__device__ __forceinline__ float fit_norm(float re, float im) {
    const double a = (double)re, b = (double)im;
    return (float)sqrt(a * a + b * b);
}

__global__ __launch_bounds__(FIT_P) void k_fit_terms(const float* __restrict__ response, const float2* __restrict__ tw, const float* __restrict__ hann,
                                                     float* __restrict__ terms) {
    constexpr int N = FIT_N, NH = FIT_NH, P = FIT_P;
    __shared__ Cf buf[NH];      // 128 KiB: the packed row, its transform, then the norms
    __shared__ float red[P];
    const int t = threadIdx.x;
    const float2* __restrict__ x = reinterpret_cast<const float2*>(response + (size_t)blockIdx.x * N);
    // echo density (reverb.rs:45-53), and the windowed row packed as z[m] = r[2m] + i r[2m+1], bit-reversed for the N/2-point transform
    float echo = 0.0f;
    for (int m = t; m < NH; m += P) {
        const float2 r = x[m];
        const int i0 = 2 * m, i1 = 2 * m + 1;
        if (i0 >= 1 && fabsf(r.x) >= 1.0e-9f) echo += 1.0f / (float)i0;
        if (fabsf(r.y) >= 1.0e-9f) echo += 1.0f / (float)i1;
        buf[bitrev(m, FIT_LOGN - 1)] = Cf{r.x * hann[i0], r.y * hann[i1]};
    }
    echo = fit_fold(red, t, echo);   // (its barriers also close the packing)
    for (int ls = 1; ls <= FIT_LOGN - 1; ls++) {
        stage<P>(buf, NH, ls, N, FIT_LOGN, tw, t);
        __syncthreads();
    }
    // real_fft's bins k and N/2 - k from one lane, which then owns both entries: their norms go to .re in place
    for (int u = t; u < NH / 2; u += P) {
        if (u == 0) {
            const Cf z0 = buf[0];   // bin 0 packs (DC, Nyquist): the norm of the pair (never read below: the sums start at bin 1)
            const Cf mid = rfft_bin(buf, NH / 2, NH, tw);
            buf[0].re = fit_norm(z0.re + z0.im, z0.re - z0.im);
            buf[NH / 2].re = fit_norm(mid.re, mid.im);
        } else {
            const Cf a = rfft_bin(buf, u, NH, tw), b = rfft_bin(buf, NH - u, NH, tw);
            buf[u].re = fit_norm(a.re, a.im);
            buf[NH - u].re = fit_norm(b.re, b.im);
        }
    }
    __syncthreads();
    float nr[NH / P];
#pragma unroll
    for (int r = 0; r < NH / P; r++) nr[r] = buf[t + r * P].re;
    __syncthreads();
    float* norm = reinterpret_cast<float*>(buf);
#pragma unroll
    for (int r = 0; r < NH / P; r++) norm[t + r * P] = nr[r];
    __syncthreads();
    // outliers above the mean of the 50 bins before (reverb.rs:98-115)
    float pen = 0.0f;
    for (int k = FIT_WINDOW + 1 + t; k < NH; k += P) {
        float sum = 0.0f;
        for (int j = k - FIT_WINDOW; j < k; j++) sum += norm[j];
        const float mean = sum / (float)FIT_WINDOW;
        const float n1 = norm[k];
        if (n1 > mean) {
            const float d = n1 - mean;
            pen += d * d;
        }
    }
    pen = fit_fold(red, t, pen);
    if (t == 0) {
        terms[(size_t)blockIdx.x * 2 + 0] = echo;
        terms[(size_t)blockIdx.x * 2 + 1] = pen * 0.1f;
    }
}

__global__ __launch_bounds__(256) void k_fit_combine(const float* __restrict__ terms, float* __restrict__ fitness, size_t instances) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= instances) return;
    const float* q = terms + i * 4;
    fitness[i] = ((q[0] - q[1]) + q[2]) - q[3];
}

}  // namespace

void fit_launch_impulse(float* in, size_t rows, hipStream_t stream) {
    if (rows == 0) return;
    const size_t blocks = (rows * FIT_N + 255) / 256;
    hipLaunchKernelGGL(k_fit_impulse, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, in, rows);
}

void fit_launch_score(const float* response, const float* d_tables, size_t instances, float* terms, float* fitness, hipStream_t stream) {
    if (instances == 0) return;
    hipLaunchKernelGGL(k_fit_terms, dim3((unsigned)(instances * 2)), dim3(FIT_P), 0, stream, response, reinterpret_cast<const float2*>(d_tables),
                       d_tables + FIT_N, terms);
    hipLaunchKernelGGL(k_fit_combine, dim3((unsigned)((instances + 255) / 256)), dim3(256), 0, stream, (const float*)terms, fitness, instances);
}

}  // namespace fd
