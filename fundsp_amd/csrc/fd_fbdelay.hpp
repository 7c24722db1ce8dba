// fd_fbdelay.hpp -- feedback delay banks: the identity-frame feedback around one or two delay lines (echo, comb, ping-pong), in the
// lane = FRAME formulation of fd_fdn.hpp / fd_fdnx.hpp:
//
//   line form:  feedback( L [>> reverse()] [* g] )                       Feedback<N, X, FrameId>   feedback.rs:108-146
//   loop form:  feedback2( L [>> reverse()], Y )                         Feedback2<N, X, Y, FrameId>  feedback.rs:233-276
//     L      = line | line_0 | line_1                                    N = 1 | 2 channels, inputs = outputs = N
//     line_i = delay(t_i) [>> fir(w_i..)] [>> F_i] [* g_i]               (loop form: delay [>> fir] only)
//     Y      = F [* g]  |  (F_0 [* g_0]) | (F_1 [* g_1])
//
// F is lowpole_hz(c) (filter.rs:19-66) or a FixedSvf of one mode (svf.rs:861-1031).  Per frame and channel c, f32, one rounding per
// operation: xin_c = in_c + value_c; d_c = Delay::tick(xin_c); o_c = Fir, then (line form) F_c, then * g_c; p_c = o_perm(c) (identity or
// reverse), then * g (the outer gain); line form: output_c = value_c = p_c -- FrameId::frame multiplies by nothing; loop form: output_c = p_c,
// value_c = F_c(p_c) [* g_c].
//
// Every delay is at least two blocks long, so all ring reads of a 64-frame block are known at its head: the kernel is the block steps of
// fd_fdn_frames.hpp with the permutation and the outer gain where the Hadamard networks have their butterflies, and the filter walked by
// lanes 0 .. N-1 over the LDS row (fdn_filter_walk, as in fd_fdnx.hip).  Parameters live in a device table of FbInst rows: one for the bank or one per instance.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "fd_fdnx.hpp"   // FDNX_NONE .. FDNX_IN_LOOP, FdnxDesc, FdnxState, FdnBus

namespace fd {

struct FbInst {            // one network's parameters at the bank's sample rate (24 words)
    int len[2];            // Delay ring length = delay in samples + 1 (delay.rs:108-110)
    float w[3][2];         // FIR weights [tap][channel], oldest tap first (fir.rs:57-70)
    float co[6][2];        // filter coefficients [coef][channel]: Lowpole coeff, 1 - coeff | FixedSvf a1 a2 a3 m0 m1 m2
    float g[2];            // the `* g_c` behind the line / the loop filter
    float outer;           // the `* g` behind the whole body
    int pad;
};

struct FbConst {
    int lines, taps;              // channels N (1 | 2); taps 0: no Fir node in the line
    int filter, place;            // FDNX_NONE | _LOWPOLE | _SVF; FDNX_IN_LINE | FDNX_IN_LOOP
    int has_gain, has_outer, reverse;
    int cap;                      // slots per ring (power of two >= the longest ring of every instance); rings are cap + 64 floats apart
    size_t ring_stride;           // floats per instance = lines * (cap + 64)
    size_t tab_stride;            // 0: one table row for all instances | 1: one per instance
    const FbInst* tab;
};

// host: the parameter table at `sample_rate` (instances rows, or 1) and the constants, from the description the two families share (FdnxDesc,
// lines = channels); returns the shortest delay in samples over all instances and channels (the caller applies the two-block rule) and -1
// when a ring would exceed 2^18 slots.  Reset is fdnx_launch_reset.
int fb_make_table(const FdnxDesc& d, size_t instances, double sample_rate, std::vector<FbInst>& tab, FbConst* c);
void fb_launch_render(const FbConst& c, const FdnxState& s, size_t instances, const float* in, float* out, size_t T, size_t fstride, int layout,
                      hipStream_t stream, const FdnBus& bus = FdnBus());

}  // namespace fd
