// fd_resynth.hpp -- banks of the reference's frequency-domain resynthesizer Resynth<I, O, F> (resynth.rs:216-372) with a stock processing
// closure, rendered as batched FFTs.
//
// The contract (N = window length, H = N / 4 the hop, z = 2/3 as f32):
//   * hann[i] = 0.5 + 0.5 * cosf(((i - N/2) as f32 * TAU) / N as f32) (resynth.rs:277-291, cosf = musl's, fd_math.hpp cosf_musl).
//   * The frame that completes at sample count k*H (k >= 4) holds x[kH-N .. kH-1] * hann; its inverse transform, divided by N, is read
//     at positions 0 .. N-1 over ticks kH .. kH+N-1 and multiplied by (hann[p] * z).  Output y[t] starts at 0.0 and adds the (up to four)
//     live frames in WINDOW order w = 0..3 (frame k belongs to window (-k) mod 4), not in frame order.
//   * Forward (real_fft + fix_nyquist, fft.rs:10-38), the project's restatement of microfft's rfft_N (whose source is absent, so its exact
//     butterflies are unpinned): pack z[m] = x[2m] + i x[2m+1], take the N/2-point complex FFT cfft (below), then
//         X[0] = (Z[0].re + Z[0].im, 0),  X[N/2] = (Z[0].re - Z[0].im, 0),
//         for k = 1 .. N/2-1:  A = Z[k], B = conj(Z[N/2-k]), E = 0.5*(A+B), D = 0.5*(A-B), X[k] = E + W_N^k * (D.im, -D.re),
//     each operation one f32 rounding in the order written (Complex32 * Complex32 = (a.re*b.re - a.im*b.im, a.re*b.im + a.im*b.re), no FMA).
//   * The processor writes output bins 0 .. N/2 (the rest start at zero, resynth.rs:190-194); fix_negative (fft.rs:40-47) sets
//     Y[i] = conj(Y[N-i]) for i in N/2+1 .. N-1; inverse_fft reverses elements 1 .. N-1, runs cfft and divides by N (fd_capi.hip
//     ifft_inplace).  Only .re is used.
//   * cfft is fd_capi.hip's cfft_inplace: radix-2 decimation in time, bit-reversed input, stages of span 2, 4, .. n, twiddle
//     (cos, -sin)(2 pi k / span) computed in double and rounded to f32.  Since N / span is a power of two, that value equals entry
//     k * N / span of ONE table (cos, -sin)(2 pi j / N), j < N/2, so the N/2-point forward and the N-point inverse share it.
//
// Stock processors (o and i in increasing order): PASS Y_o[i] = X_src[o][i]; BAND the same where lo_o <= frequency(i) <= hi_o
// (frequency(i) = (sr as f32 / N as f32) * i as f32, resynth.rs:128-131); GAIN Y_o[i] = X_src[o][i] * g_o[i] (Complex32 * f32).
// source[o] = -1 leaves output o silent (its spectrum stays zero).
//
// Device layout.  Frames are independent given the input, so a launch is split into chunks and each chunk runs three kernels:
//   k_rs_input   the chunk's input samples -> a per-instance input ring xin [V][I][Rx] (raw x; the window is applied on reading),
//   k_rs_frames  one unit per (new frame, instance, output): the source channel's forward transform and the output's inverse, the whole
//                working set in LDS (N complex f32: 64 KiB at N = 8192), the N real outputs / N written to a per-instance frame ring
//                frames [V][R][O][N] in HBM (slot k mod R),
//   k_rs_ola     one lane per (instance, output, sample): the window-ordered sum of the four frames that cover the sample,
// and a one-lane kernel advances the device-side sample counter.  The counter and the bin spacing of frequency() live on the device, so a
// captured launch replays with the state moving on and with the sample rate of the moment.  The chunk length L is at most (R - 5) * H, so
// the frames a chunk reads (the four before it and the ones it makes) never share a ring slot, and Rx >= L + N, so the chunk's input never
// overwrites history a frame still needs.  Every size takes the HBM frame ring: the overlap-add needs frames made by other workgroups (and
// earlier launches), which LDS cannot hold across workgroups.  R = clamp(256 MiB / (V * O * N * 4 B), 8, 5 + 65536 / H), so the frame ring
// is at most max(256 MiB, 8 * V * O * N * 4 B), and the input ring V * I * Rx * 4 B.  The split into chunks depends on R only, and any split
// of a launch gives the same bits as one launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "fd_resynth_fn.hpp"   // RsFnArgs: the argument block of a closure bank's run-time compiled process kernel

namespace fd {

constexpr int RS_PASS = 0, RS_BAND = 1, RS_GAIN = 2;
constexpr int RS_FN = 3;   // a caller's closure (fd_resynth_fn.hpp): the host's mark only, k_rs_frames never sees it
constexpr int RS_MAX_CH = 8;
constexpr int RS_MIN_LOGN = 2, RS_MAX_LOGN = 13;   // N = 4 .. 8192

struct RsConst {
    int N, logN, I, O;
    int proc;                 // RS_PASS | RS_BAND | RS_GAIN
    int src[RS_MAX_CH];       // input channel of each output, -1 = silent
    int rows;                 // 1: shared band / gain tables, V: per instance
    float invN;               // 1 / N (exact): x * invN == x / N bit for bit
    int R;                    // frame ring slots per instance (>= 8)
    int Rx;                   // input ring length per channel (power of two >= Lmax + N)
    int Lmax;                 // longest chunk: (R - 5) * H
    const float2* tw;         // [N/2] (cos, -sin)(2 pi j / N) as f32
    const float* hann;        // [N]
    const float* hz;          // [N] hann[p] * z (rounded once)
    const float2* band;       // [rows][O] (lo, hi) in Hz
    const float* gain;        // [rows][O][N/2 + 1]
};

struct RsState {
    float* frames;            // [V][R][O][N] inverse-transformed real outputs / N
    float* xin;               // [V][I][Rx] input history
    unsigned long long* samples;   // [1] samples processed since reset (all instances run in lock-step)
    float* fstep;                  // [1] (sample_rate as f32) / (N as f32): frequency(i) = fstep * i (device memory, so a replayed capture follows set_sample_rate)
};

// a closure bank's part (fd_resynth_fn.hpp): the spectrum workspace, parameters, per-bin state and the process kernel of its module
struct RsFn {
    int P, S, Fc;             // parameters per instance, state values per (instance, bin), frames per chunk (RsConst::Lmax = (Fc - 1) * H)
    float2* x;                // [V][Fc][I][N/2 + 1] input spectra of the chunk
    float2* y;                // [V][Fc][O][N/2 + 1] output spectra
    float* params;            // [V][P]
    float* state;             // [V][N/2 + 1][S]
    float* srf;               // [1] sample rate as f32 (the time() family; device memory like fstep)
    hipFunction_t process;    // rs_process of the bank's module
};

// host: the window and twiddle tables of N (fdsp_resynth_tables); hz = hann * (2/3 as f32)
void rs_tables(int N, float* hann, float* hz, float* tw);
// fd_jit.hip: the process module of a functor -- fd_resynth_fn.hpp + `source` in namespace fd + rs_process around `functor`, with
// static_asserts that its PARAMS / STATE equal `params` / `state`.  No device needed.  Equal requests share one code object.  0 or -1 + log
int jit_compile_resynth_fn(const std::string& functor, const std::string& source, int params, int state, bool ftz,
                           std::shared_ptr<const std::vector<char>>* code, std::string* log);

namespace rs_ieee {
void rs_launch_render(const RsConst& c, const RsState& st, size_t V, const float* in, float* out, size_t T, size_t fstride, int layout,
                      hipStream_t stream);
void rs_launch_render_fn(const RsConst& c, const RsState& st, const RsFn& fn, size_t V, const float* in, float* out, size_t T, size_t fstride,
                         int layout, hipStream_t stream);
}
namespace rs_ftz {   // the same kernels compiled with f32 denormals flushed (a Feedback node in front of the resynthesizer)
void rs_launch_render(const RsConst& c, const RsState& st, size_t V, const float* in, float* out, size_t T, size_t fstride, int layout,
                      hipStream_t stream);
void rs_launch_render_fn(const RsConst& c, const RsState& st, const RsFn& fn, size_t V, const float* in, float* out, size_t T, size_t fstride,
                         int layout, hipStream_t stream);
}

}  // namespace fd
