// fd_fitness.hpp -- reverb_fitness (reverb.rs:31-139) per instance of a stereo effect bank, on the device: the score examples/optimize.rs
// maximises over populations of reverb4_stereo_delays candidates (reverb.rs:17-28).
//
// The reference renders `Impulse::<U2> >> reverb` for N = 32 768 samples at 44.1 kHz (reverb.rs:32-36) and then, per channel c in {0, 1}
// (the `channel == 0 || channel == 1` arm; the stereo arm :67-73 is unreachable in `0..=1`):
//   echo_c = sum_{i=1}^{N-1} (|r[i]| >= 1e-9 ? 1 / (i as f32) : 0)                              :45-53  (echo_weight = 1)
//   r[i] *= 0.5 + 0.5 * cos((i - N/2) as f32 * TAU / N as f32)                                  :56-64  (the Hann window of resynth.rs, rs_tables)
//   S = real_fft(r): N/2 complex bins, Nyquist packed into bin 0's imaginary part               :75, fft.rs:6-29
//   norm_k = |S_k|, k < N/2 (Complex32::norm = hypot; bin 0: the norm of the packed pair)      :103-108
//   pen_c = sum_{k=51}^{N/2-1} max(0, norm_k - mean_k)^2 * 0.1, mean_k = (sum_{j=k-50}^{k-1} norm_j) / 50     :98-115
// and fitness = echo_0 - pen_0 + echo_1 - pen_1 (:38, :51, :111, :138).  The commented-out flatness and autocorrelation terms (:76-96,
// :116-135) are not restated.
//
// Here: one workgroup of 1 024 lanes per (instance, channel) row of the rendered response [instances][2][N] (k_fit_terms), then one lane
// per instance for the total (k_fit_combine).  A row is windowed and packed into a 16 384-point complex buffer in LDS (128 KiB), transformed
// by fd_fft.hpp's stage<1024> over 14 stages with the 32 768-point twiddle table of rs_tables, split by rfft_bin -- the pair (k, N/2 - k) in
// one lane, which overwrites both entries with their norms -- and the norms are compacted to the front of the buffer.
//
// ORDER OF THE SUMS (fixed, no atomics: the same bits run to run, whatever the bank size):
//   echo_c:  lane t adds its terms in ascending i over i = 2m, 2m + 1 for m = t, t + 1024, ..; the 1 024 partial sums are folded by the
//            tree red[t] += red[t + s], s = 512, 256, .. 1.
//   mean_k:  the 50 norms j = k - 50 .. k - 1 added in ascending j from 0.0, then / 50.0 -- for k = 51 the reference's own first sum
//            (:102-104).  DEVIATION: the reference slides one running `sum -= norm0; sum += norm1` (:113-114) across all bins; summing
//            each window afresh carries no error from bin to bin (and needs no prefix sums, whose differences would cancel).
//   pen_c:   lane t adds (norm_k - mean_k)^2 over k = 51 + t, 51 + t + 1024, .. ascending where norm_k > mean_k; the same tree; the 0.1
//            multiplies the sum, not every term.
//   fitness: ((echo_0 - pen_0) + echo_1) - pen_1.
// The norm is sqrt(re^2 + im^2) evaluated in f64 and rounded to f32 (hypot's result but for double rounding).  The FFT is the project's
// radix-2 one in f32, not microfft's: the spectrum differs from the reference's by f32 rounding of the same size.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

namespace fd {

constexpr int FIT_LOGN = 15, FIT_N = 1 << FIT_LOGN, FIT_NH = FIT_N / 2;   // reverb.rs:34: 32768.0 / 44100.0 seconds at 44 100 Hz
constexpr int FIT_WINDOW = 50;                                            // outlier_samples :99
constexpr size_t FIT_TABLE_FLOATS = (size_t)FIT_N + FIT_N;                // twiddles [N/2] (cos, -sin) | Hann [N]

// host: the two tables (rs_tables(32768, ..)) in the order above
void fit_make_tables(float* tables);
// in = [rows][N]: 1.0 at frame 0, zeros after (Impulse::<U2>, rows = instances * 2)
void fit_launch_impulse(float* in, size_t rows, hipStream_t stream);
// response = [instances][2][N] planar; terms = [instances][4] (echo_0, pen_0, echo_1, pen_1); fitness = [instances]
void fit_launch_score(const float* response, const float* d_tables, size_t instances, float* terms, float* fitness, hipStream_t stream);

}  // namespace fd
