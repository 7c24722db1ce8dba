// fd_fxmix.hip -- the fused mix-down of the lane-per-frame effect banks (fd_fxbank.hpp, fdsp_bank_process_mix on reverb / network banks):
// the kernels between a planar render in the bank's mix scratch and the groups' partial mixes.  Built with the default flags (IEEE
// denormals), like fd_capi.hip's k_group_partials / k_mix_tree: the additions below are the only arithmetic here, and they are the
// additions of fdsp_sum_voices.
#include "fd_fxbank.hpp"

namespace fd {
namespace {

// four frames of one row: a 16-byte load where the row allows it, else dwords (a ragged end, an odd stride); frames past `n` read as +0.0
__device__ __forceinline__ float4 ld_frames(const float* __restrict__ row, size_t t, size_t n, bool v4) {
    if (v4) return *reinterpret_cast<const float4*>(row + t);
    float4 r = {0.0f, 0.0f, 0.0f, 0.0f};
    if (t < n) r.x = row[t];
    if (t + 1 < n) r.y = row[t + 1];
    if (t + 2 < n) r.z = row[t + 2];
    if (t + 3 < n) r.w = row[t + 3];
    return r;
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
__device__ __forceinline__ float4 mul4(float4 a, float w) { return float4{a.x * w, a.y * w, a.z * w, a.w * w}; }

// x: planar [V][C][xstride], frames 0 .. n-1 of it -> part[group][mix channel][T], columns t0 .. t0+n-1: the group's partial in the
// mix-down's summation order (include/fundsp_hip.h "SUMMATION ORDER"): (S0 + S1) + (S2 + S3), Sq = the quarter's 16 instances added one
// after the other, instances past the end +0.0.  PAN (C == 1): every sample times its instance's two weights first, two mix channels.
// Lane = frame (four frames per lane).  One workgroup = one group x one channel x 256 frames; wave q adds up quarter q -- its sixteen
// loads are independent of the running sum and go out ahead of the adds -- and the four quarters meet in LDS.
// vec: bit 0 = the input rows take 16-byte loads, bit 1 = the partial rows take 16-byte stores.
template <bool PAN>
__global__ __launch_bounds__(256) void k_fx_mix_groups(const float* __restrict__ x, const float* __restrict__ panw, size_t pstride,
                                                       float* __restrict__ part, size_t V, int C, size_t xstride, size_t n, size_t T, size_t t0,
                                                       int vec) {
    constexpr int NM = PAN ? 2 : 1;
    __shared__ float4 sq[NM][4][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const size_t g = blockIdx.x, t = ((size_t)blockIdx.z * 64 + lane) * 4;
    const int c = blockIdx.y;
    const size_t v0 = g * 64 + (size_t)q * 16;
    const bool whole = t + 4 <= n;
    float4 xs[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const size_t v = v0 + j;
        xs[j] = v < V ? ld_frames(x + (v * C + c) * xstride, t, n, (vec & 1) && whole) : float4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    if constexpr (PAN) {
        float4 sl = {0.0f, 0.0f, 0.0f, 0.0f}, sr = sl;
        if (v0 < V) {
            sl = mul4(xs[0], panw[v0]);
            sr = mul4(xs[0], panw[pstride + v0]);
        }
#pragma unroll
        for (int j = 1; j < 16; j++) {
            const size_t v = v0 + j;
            const float4 z = {0.0f, 0.0f, 0.0f, 0.0f};
            sl = add4(sl, v < V ? mul4(xs[j], panw[v]) : z);
            sr = add4(sr, v < V ? mul4(xs[j], panw[pstride + v]) : z);
        }
        sq[0][q][lane] = sl;
        sq[1][q][lane] = sr;
    } else {
        float4 s = xs[0];
#pragma unroll
        for (int j = 1; j < 16; j++) s = add4(s, xs[j]);
        sq[0][q][lane] = s;
    }
    __syncthreads();
    if (q != 0 || t >= n) return;
#pragma unroll
    for (int m = 0; m < NM; m++) {
        const float4 r = add4(add4(sq[m][0][lane], sq[m][1][lane]), add4(sq[m][2][lane], sq[m][3][lane]));
        float* dst = part + (g * (size_t)(PAN ? 2 : C) + (size_t)(PAN ? m : c)) * T + t0 + t;
        if ((vec & 2) && whole) *reinterpret_cast<float4*>(dst) = r;
        else {
            dst[0] = r.x;
            if (t + 1 < n) dst[1] = r.y;
            if (t + 2 < n) dst[2] = r.z;
            if (t + 3 < n) dst[3] = r.w;
        }
    }
}

// frames t0 .. t0+n-1 of a voice-minor buffer [C][T][V] -> planar [V][C][dstride], frames 0 .. n-1: one 64 x 64 tile per workgroup
__global__ __launch_bounds__(256) void k_fx_stage_in(const float* __restrict__ src, float* __restrict__ dst, size_t V, size_t T, int C, size_t t0,
                                                     size_t n, size_t dstride) {
    __shared__ float tile[64][65];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t v0 = (size_t)blockIdx.x * 64, f0 = (size_t)blockIdx.y * 64;
    const int c = blockIdx.z;
#pragma unroll 4
    for (int r = w; r < 64; r += 4)
        tile[r][lane] = (f0 + r < n && v0 + lane < V) ? src[((size_t)c * T + t0 + f0 + r) * V + v0 + lane] : 0.0f;
    __syncthreads();
#pragma unroll 4
    for (int r = w; r < 64; r += 4)
        if (v0 + r < V && f0 + lane < n) dst[((v0 + r) * C + c) * dstride + f0 + lane] = tile[lane][r];
}

// frames 0 .. n-1 of `rows` rows: src (row stride sstride) -> dst (row stride dstride)
__global__ __launch_bounds__(256) void k_fx_copy_rows(const float* __restrict__ src, size_t sstride, float* __restrict__ dst, size_t dstride, size_t n) {
    const size_t row = blockIdx.x;
    for (size_t t = (size_t)blockIdx.y * 256 + threadIdx.x; t < n; t += (size_t)gridDim.y * 256) dst[row * dstride + t] = src[row * sstride + t];
}

}  // namespace

void fx_launch_mix_groups(const float* x, size_t V, int C, size_t xstride, size_t n, float* part, size_t T, size_t t0, const float* panw,
                          size_t pstride, hipStream_t s) {
    if (V == 0 || n == 0 || C == 0) return;
    const int vec = ((xstride % 4 == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0) | ((T % 4 == 0 && t0 % 4 == 0 && ((uintptr_t)part & 15) == 0) ? 2 : 0);
    const dim3 grid((unsigned)((V + 63) / 64), (unsigned)(panw ? 1 : C), (unsigned)((n + 255) / 256));
    if (panw) hipLaunchKernelGGL(k_fx_mix_groups<true>, grid, dim3(256), 0, s, x, panw, pstride, part, V, 1, xstride, n, T, t0, vec);
    else hipLaunchKernelGGL(k_fx_mix_groups<false>, grid, dim3(256), 0, s, x, panw, pstride, part, V, C, xstride, n, T, t0, vec);
}

void fx_launch_stage_in(const float* src, float* dst, size_t V, size_t T, int channels, size_t t0, size_t n, size_t dstride, hipStream_t s) {
    if (V == 0 || n == 0 || channels == 0) return;
    hipLaunchKernelGGL(k_fx_stage_in, dim3((unsigned)((V + 63) / 64), (unsigned)((n + 63) / 64), (unsigned)channels), dim3(256), 0, s, src, dst, V, T,
                       channels, t0, n, dstride);
}

void fx_launch_copy_rows(const float* src, size_t sstride, float* dst, size_t dstride, size_t rows, size_t n, hipStream_t s) {
    if (rows == 0 || n == 0) return;
    const size_t by = (n + 255) / 256;
    hipLaunchKernelGGL(k_fx_copy_rows, dim3((unsigned)rows, (unsigned)(by < 64 ? by : 64)), dim3(256), 0, s, src, sstride, dst, dstride, n);
}

}  // namespace fd
