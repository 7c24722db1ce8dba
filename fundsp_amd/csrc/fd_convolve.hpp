// fd_convolve.hpp -- banks of the reference's Convolver (convolve.rs, prelude.rs:3154-3160: `convolve(&wave, channel)`, 1 -> 1, ID = 100),
// rendered as uniformly partitioned FFT convolution.
//
// What the reference pins: y[n] = sum over k < M of h[k] * x[n - k], x[n < 0] = 0, NO latency (test_basic.rs:698-711), tick and process
// within 1e-4 (test_basic.rs:329-330), reset() clears the history, set_response re-initialises the node, no set_sample_rate override.  It
// wraps fft_convolver::FFTConvolver<f32>, whose source is not in the reference tree: that crate's butterflies, its partition scheme and any
// trimming of trailing near-zero taps are NOT pinned.  The algorithm below is this project's own statement, and the kernels, the numpy
// restatement (tests/convolve_ref.py) and every split of an input into launches give its bits exactly.
//
// The contract (B = block length, a power of two; N = 2B; M = response length; P = ceil(M / B); n = samples since reset; every operation
// one f32 rounding in the order written, no FMA; Complex32 a * b = (a.re*b.re - a.im*b.im, a.re*b.im + a.im*b.re)):
//   * B is chosen at creation from the response CAPACITY max_len: the power of two at or above sqrt(8 * max_len), clamped to 64 .. 4096
//     (cv_block_length; tail about 8 M / B and head about B operations per output sample).
//   * rfft_N(g) of N real values is fd_resynth.hpp's forward: z[m] = g[2m] + i g[2m+1], the B-point cfft, then the split into bins 0 .. B
//     (bins 0 and B have .im = +0.0).  irfft_N(Z) of bins 0 .. B is its inverse: fix_negative, the reversal of elements 1 .. N-1, the N-point
//     cfft, .re * (1/N).  One twiddle table (cos, -sin)(2 pi j / N), j < B, computed in double and rounded to f32.
//   * Response spectra, p = 0 .. P-1:  G_p = rfft_N(g_p),  g_p[i] = h[(p+1)B + i] for i < B,  g_p[B] = 0,  g_p[i] = h[pB + i - B] for i > B
//     (h[k] = 0 for k >= M; the first B values of the product never read g_p[B], so it carries no tap and adds no rounding noise).  The
//     circular convolution of a zero-padded block with g_p has, in its first B values, exactly the block's contribution to the B outputs
//     that start (p + 1) blocks later: taps pB + 1 .. (p + 2)B - 1, no aliasing.
//   * Block spectra: when the count reaches (j + 1)B, X_j = rfft_N(x[jB .. jB + B - 1] followed by B zeros).  Only complete blocks are ever
//     transformed, so no rounding depends on where a launch ended.
//   * Tail: at the same moment, with j' = j + 1:  Z = (0, 0);  for p = 0, 1, .. min(P, j') - 1 in this order:  Z[k] = Z[k] + X_{j'-1-p}[k] *
//     G_p[k]  (k = 0 .. B; terms of blocks before the reset are skipped, not added as zeros);  pend_{j'}[r] = irfft_N(Z)[r], r = 0 .. B-1.
//     pend_0[r] = +0.0.  One forward and ONE inverse transform per block: folding the overlap-add's two halves into g_p is what overlap-save
//     does, with the zero-padded window the head makes possible.
//   * Head and output, n = jB + r:  a = h[0] * x[n];  for i = 1 .. min(r, M - 1):  a = a + h[i] * x[n - i];  y[n] = pend_j[r] + a.
//   * reset(): n = 0 (nothing before it is read again).  set_response: new h, M, P and G, then reset.  Channel c of a bank is its own 1 -> 1
//     convolver with response row c; instances run in lock-step (one sample counter).
//   * Routing: a bank has I inputs and C outputs, 1 <= I <= C <= 8, and a source map source[c] in [0, I) under which every input feeds at
//     least one output.  Output c is the 1 -> 1 convolver above with response row c, reading input source[c]: block spectra X_j and the
//     input samples are per (instance, input); G, h, Z, pend and y are per (instance, output).  No operation and no order changes, so a
//     routed bank gives the bits of the C-channel bank fed copies of the input rows (tests/convolve_ref.py: render(x[:, source, :], h)),
//     and the identity map (I = C, fdsp_convolve_create) is the bank of the bullets above.
//   * Summing: a bank has I inputs, O outputs and NT terms, 1 <= I <= 8, 1 <= O <= 8, 1 <= NT <= 16.  Term t convolves input tin[t] with
//     response row t and belongs to output tout[t]; tout is non-decreasing, every output has at least one term, every input feeds at
//     least one term; one response length M for the whole bank (shorter rows zero-padded).  X_j and the input ring are per (instance,
//     input), G and h per (row, term), Z, pend and y per (instance, output).
//     Tail of output o at boundary j':  Z = (0, 0);  for each term t of o in increasing t:  for p = 0 .. min(P, j') - 1 in this order:
//     Z[k] = Z[k] + X^{tin[t]}_{j'-1-p}[k] * G_{t,p}[k];  pend_{j'} = irfft_N(Z)[0 .. B-1].  ONE running sum across the terms, not one sum
//     per term added afterwards; terms of blocks before the reset are skipped, as above.
//     Head at n = jB + r:  for the first term t of o:  a = h_t[0] * x_t[n];  a = a + h_t[i] * x_t[n - i] for i = 1 .. min(r, M - 1)  (x_t
//     the input tin[t]);  for every later term of o, in order:  a = a + h_t[0] * x_t[n], then the same i loop;  y[n] = pend_j[r] + a.
//     An output with a single term has exactly the routed bank's bits, and a summing bank in which every output has one term IS the
//     routed bank; every split into launches gives the same bits; FDSP_MODE_TICK == FDSP_MODE_PROCESS.
//     This is the project's statement of Binop<FrameAdd> over convolvers (src/audionode.rs:903-955, `convolve(&w, 0) + convolve(&w, 1)`):
//     the reference adds the two nodes' rounded outputs, this bank adds before the inverse transform, and the association of a `+` tree
//     is flattened to term order.  Both stay inside the float64 bound below; the fft_convolver crate's bits are not pinned either way.
//
// Device layout.  Nothing is allocated after creation.  A launch is cut into chunks of at most Lmax = KB * B samples, and a chunk runs, on
// the bank's stream (S = the count at its start, read from device memory, so a captured launch replays with the state moving on):
//   k_cv_input    the chunk's samples -> input ring xin [V][C][Rx], Rx a power of two >= Lmax + B,
//   k_cv_forward  one unit per (block completing in the chunk, instance, channel): X_j in LDS -> spectrum ring spec [V][C][R][B + 1] (re, im),
//                 slot j mod R, R = Pcap + KB (Pcap = ceil(max_len / B)): the frequency-domain delay line,
//   k_cv_tail     the hot kernel.  Per bin the tail is a 1-D convolution along the block index, so a lane owns one bin of one (instance,
//                 channel) for CV_J consecutive block boundaries: it walks the blocks from the newest down ONCE, keeps the CV_J sums in
//                 registers and a window of the last CV_J response bins in registers, and uses each X loaded for up to CV_J sums (p still
//                 increases from zero in every sum).  Z -> zbuf [V][C][KB][B + 1],
//   k_cv_inverse  one unit per (boundary, instance, channel): irfft_N in LDS -> pend ring pend [V][C][KB + 1][B], slot j' mod (KB + 1),
//   k_cv_output   one workgroup per (instance, channel, tile of min(B, 256) samples aligned to the absolute count): the block's inputs up to
//                 the tile's end and the taps they meet are staged in LDS, one lane per sample adds pend + head,
//   k_cv_advance  one lane: n += L.
// A routed bank (fdsp_convolve_routed_create; NG > 0) keeps xin and spec per (instance, INPUT) -- [V][I][Rx], [V][I][R][B + 1]; k_cv_input and
// k_cv_forward run over V x I rows -- and zbuf, pend, h and G per (instance, output) as above.  The outputs of one input, in increasing
// output order, are cut into FAN GROUPS of at most CV_FAN = 2; the groups (full ones first) are part of CvConst, passed by value with every
// launch, never read from device memory.  Tail and head run per group instead of per output:
//   k_cv_tail_fan<F>    a lane owns bin k of one (instance, group) for CV_J boundaries: each X of the group's input is loaded ONCE and enters
//                       the F x CV_J sums of the group's outputs, every sum with its own window of response bins and p increasing from zero,
//   k_cv_output_fan<F>  one workgroup per (instance, group, tile): the block's input samples are staged in LDS once, the taps of the F outputs
//                       behind them ((1 + F) * B floats: 48 KiB at B = 4096, F = 2, under the 64 KiB a workgroup may take here); a lane
//                       computes the F heads of its sample, each in the order above, from ONE read of every xs[r - i].
// A group of one output runs the same two kernels at F = 1 (a permutation or the identity map is all such groups).  k_cv_inverse is the
// plain bank's.  A plain bank (NG = 0) launches k_cv_tail / k_cv_output exactly as before.
// A summing bank (fdsp_convolve_matrix_create; sum = 1) keeps xin and spec per (instance, input) as a routed bank does, h and G per (row,
// TERM) -- [rows][NT][..]; NT is the response-row count of every bank, C for a plain or routed one -- and zbuf and pend per (instance,
// output).  The term tables tin[16] and tfirst[9] (the first term of each output) travel in CvConst, never through device memory:
//   k_cv_tail_sum    a lane owns bin k of one (instance, output) for CV_J boundaries; the CV_J sums stay in registers across the output's
//                    terms, and each term runs k_cv_tail's whole step loop with its own response spectra, spectrum ring and window,
//   k_cv_output_sum  one workgroup per (instance, output, tile); LDS stays at 2 * B floats (16 terms staged at once would be 512 KiB at
//                    B = 4096), so the workgroup walks the terms: stage xs / hs, barrier, accumulate, barrier.  Every lane reaches every
//                    barrier; consecutive terms of one input keep xs.
// k_cv_input and k_cv_forward run over V x I rows, k_cv_inverse and k_cv_advance over V x O; KB keeps its formula with C = O.  Memory:
// V * (I * (Rx*4 + R*(B + 1)*8) + O * (KB*(B + 1)*8 + (KB + 1)*B*4)) + rows*NT * ((Pcap + 1)*B*4 + Pcap*(B + 1)*8).  Not built: loading an
// X once for several outputs that read the same inputs (the fan groups above; true stereo reads each twice), a register-blocked head.
// M and P live on the device too (dims), so a replayed capture follows set_response.  KB = clamp(256 MiB / (V * C * (B + 1) * 8 B), 8, 64).
// Memory: V*C * (Rx*4 + (R + KB)*(B + 1)*8 + (KB + 1)*B*4) + rows*C * ((Pcap + 1)*B*4 + Pcap*(B + 1)*8) bytes, rows = V with per-instance
// responses, else 1.  Routed: V * (I * (Rx*4 + R*(B + 1)*8) + C * (KB*(B + 1)*8 + (KB + 1)*B*4)) plus the same response tables; KB keeps its
// formula with C = outputs (zbuf is per output), so the chunks are the C-channel plain bank's.  A 1 -> 2 bank of 2 048 instances x 96 000
// taps (B = 1024, Pcap = 94, KB = 8, R = 102, Rx = 16 384) saves one input's rings against the 2 -> 2 bank fed the input twice:
// 2 048 * (16 384*4 + 102*1 025*8) = 1 847 164 928 bytes, 1.72 GiB of the 2 -> 2 bank's 3.83 GiB of state.
//
// Accuracy of the statement against a float64 convolution, max |y - y64| / (sum |h| * max |x|) (tests/test_convolve_ref.py, four times the
// largest figure measured over 8 seeds): 4.1e-7 at B = 64, 9.5e-7 at B = 128 .. 4096.  The error follows sqrt(P) * log2(2B) * 2^-24 with a
// constant of 0.33 at most; the largest figures belong to SHORT responses under a large capacity, where the transforms' noise of the order
// log2(2B) * 2^-24 stands against a small sum |h|, not to the long heads or the many partitions.
// Summing banks, max |y - y64| / (sum over the output's terms of sum |h_t| * max |x|) for K = 1, 2, 4, 8 terms per output
// (tests/test_convolve_matrix_ref.py, the largest figure of 8 seeds): 1.64e-7, 1.31e-7, 1.24e-7, 1.15e-7 at B = 64 and 2.37e-7, 1.97e-7,
// 1.69e-7, 1.30e-7 at B = 1024; asserted four times the largest, 6.6e-7 and 9.5e-7.  The reference's arithmetic (the plain bank's
// outputs added in f32, left fold) measures 1.64e-7, 9.49e-8, 5.89e-8, 6.38e-8 and 2.37e-7, 1.49e-7, 9.48e-8, 7.75e-8: inside the same
// bound, and below the statement's figures for K > 1.  The model sqrt(K P) * log2(2B) * 2^-24 holds with a constant of 0.39 at most.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fd {

constexpr int CV_MAX_CH = 8;
constexpr int CV_MIN_LOGB = 6, CV_MAX_LOGB = 12;   // B = 64 .. 4096
constexpr int CV_J = 8;                            // block boundaries per lane of the tail kernel
constexpr int CV_FAN = 2;                          // outputs of one input that a fan group renders together (routed banks)
constexpr int CV_MAX_TERMS = 16;                   // terms (response rows) of a summing bank

struct CvConst {
    int B, logB, C;
    int rows;                 // 1: one response per channel for every instance, V: per instance
    int Pcap;                 // partitions the capacity holds: ceil(max_len / B)
    size_t Hcap;              // taps per row and channel as stored: (Pcap + 1) * B, zero beyond M
    int KB;                   // blocks per chunk; Lmax = KB * B
    int R;                    // spectrum ring slots: Pcap + KB
    int Rx;                   // input ring length (power of two >= Lmax + B)
    float invN;               // 1 / (2B) (exact)
    const float2* tw;         // [B] (cos, -sin)(2 pi j / 2B)
    const float* h;           // [rows][NT][Hcap]
    const float2* G;          // [rows][NT][Pcap][B + 1]
    // routing (the contract's last bullet); a plain bank has I = C, the identity map and NG = 0
    int I;                    // inputs, 1 .. C
    int source[CV_MAX_CH];    // output c reads input source[c]
    int NG, NG2;              // fan groups; the first NG2 hold CV_FAN outputs, the others one.  NG = 0: the plain kernel sequence
    int gsrc[CV_MAX_CH];      // a group's input
    int gout[CV_MAX_CH][CV_FAN];   // its outputs, increasing (a group of one repeats its output)
    // response rows per bank row: h and G are [rows][NT][..] while zbuf and pend are [V][C][..].  A plain or routed bank has NT = C
    int NT;
    // summing (the contract's last bullet): sum = 1, C outputs, NT terms; term t convolves input tin[t] with response row t and the terms
    // of output o are tfirst[o] .. tfirst[o + 1] - 1.  Passed by value like the fan groups, never read from device memory
    int sum;
    int tin[CV_MAX_TERMS];
    int tfirst[CV_MAX_CH + 1];
};

struct CvState {
    float* xin;               // [V][I][Rx]
    float2* spec;             // [V][I][R][B + 1]
    float2* zbuf;             // [V][C][KB][B + 1]
    float* pend;              // [V][C][KB + 1][B]
    unsigned long long* samples;   // [1] samples since reset
    int* dims;                // [2] M, P
};

// host: B for a response capacity; the largest capacity a bank takes
int cv_block_length(size_t max_len);
// host: I, source and the fan groups of `c` (C set) from a source map of C entries that the caller has checked; fan = false: the plain bank
// (source may be NULL: the identity map, no groups)
void cv_set_routing(CvConst& c, int inputs, const int* source, bool fan);
constexpr size_t CV_MAX_LEN = (size_t)1 << 24;

namespace cv_ieee {
void cv_launch_render(const CvConst& c, const CvState& st, size_t V, const float* in, float* out, size_t T, size_t fstride, int layout,
                      hipStream_t stream);
void cv_launch_response(const CvConst& c, size_t row0, size_t nrows, hipStream_t stream);   // G of rows [row0, row0 + nrows) from h
}
namespace cv_ftz {   // the same kernels compiled with f32 denormals flushed (a Feedback node in front of the convolver)
void cv_launch_render(const CvConst& c, const CvState& st, size_t V, const float* in, float* out, size_t T, size_t fstride, int layout,
                      hipStream_t stream);
void cv_launch_response(const CvConst& c, size_t row0, size_t nrows, hipStream_t stream);
}

}  // namespace fd
