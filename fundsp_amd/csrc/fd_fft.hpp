// fd_fft.hpp -- the radix-2 FFT the frequency-domain banks share (fd_resynth.hip, fd_convolve.hip), as device code over a buffer in LDS.
// It is cfft_inplace of fd_capi.hip restated per lane (fd_resynth.hpp states every operation): bit-reversed input, stages of span 2, 4, .. n,
// twiddle k * (N / span) of ONE table (cos, -sin)(2 pi j / N), j < N/2, computed in double and rounded to f32 (rs_tables).  Every operation is
// one f32 rounding in the order written, no FMA (the translation units build with -ffp-contract=off).  The functions are static to the
// translation unit that includes them: each unit builds twice (IEEE denormals / flushed) and must not share an instantiation.
#pragma once

#include <hip/hip_runtime.h>

namespace fd {
namespace {

struct Cf {
    float re, im;
};

__device__ __forceinline__ unsigned bitrev(unsigned x, int bits) { return __brev(x) >> (32 - bits); }

// one radix-2 stage of cfft_inplace over `n` points at buf: butterflies j = lane, lane + P, ..; twiddle k * (N / span) of the N table
template <int P>
__device__ __forceinline__ void stage(Cf* buf, int n, int lspan, int N, int logN, const float2* __restrict__ tw, int lane) {
    const int half = 1 << (lspan - 1);
    const int tstep = logN - lspan;   // N / span = 2^tstep
    for (int j = lane; j < n / 2; j += P) {
        const int k = j & (half - 1);
        const int i = ((j >> (lspan - 1)) << lspan) + k;
        const float2 w = tw[k << tstep];
        Cf p = buf[i], q = buf[i + half];
        const float yr = w.x * q.re - w.y * q.im, yi = w.x * q.im + w.y * q.re;
        buf[i + half] = Cf{p.re - yr, p.im - yi};
        buf[i] = Cf{p.re + yr, p.im + yi};
    }
}

// real_fft + fix_nyquist: bin b (0 .. NH) of the N = 2 NH point real transform from the NH-point complex transform of the packed input at buf
__device__ __forceinline__ Cf rfft_bin(const Cf* buf, int b, int NH, const float2* __restrict__ tw) {
    if (b == 0 || b == NH) {
        const Cf z0 = buf[0];
        return Cf{b == 0 ? z0.re + z0.im : z0.re - z0.im, 0.0f};
    }
    const Cf A = buf[b], Bc = buf[NH - b];
    const Cf B{Bc.re, -Bc.im};
    const Cf E{0.5f * (A.re + B.re), 0.5f * (A.im + B.im)};
    const Cf D{0.5f * (A.re - B.re), 0.5f * (A.im - B.im)};
    const float2 w = tw[b];
    const float qr = D.im, qi = -D.re;
    const float wr = w.x * qr - w.y * qi, wi = w.x * qi + w.y * qr;
    return Cf{E.re + wr, E.im + wi};
}

// fix_negative + the inverse's reversal of elements 1 .. N-1: output bin b (0 .. N/2) stored bit-reversed for the N-point transform
__device__ __forceinline__ void ifft_store_bin(Cf* buf, int b, Cf Y, int logN) {
    const int N = 1 << logN;
    if (b == 0 || b == N / 2) {
        buf[bitrev(b, logN)] = Y;
    } else {
        buf[bitrev(b, logN)] = Cf{Y.re, -Y.im};
        buf[bitrev(N - b, logN)] = Y;
    }
}

}  // namespace
}  // namespace fd
