// fd_fdnx.hpp -- Hadamard feedback delay networks with a recursive filter in the line or in the loop, per-line FIR weights and
// per-instance parameters, in the lane = FRAME formulation of fd_fdn.hpp's generic network:
//
//   line form:  split | multisplit >> fdn(stacki(|i| delay(t_i) [>> fir(w_i..)] [>> F_i] [* g_i])) >> join | multijoin
//   loop form:  split | multisplit >> fdn2(stacki(|i| delay(t_i) [>> fir(w_i..)]), stacki(|i| F_i [* g_i])) >> join | multijoin
//
// F_i is lowpole_hz(c_i) (filter.rs:19-66) or a FixedSvf of one mode (svf.rs:861-1031) with per-line cutoff / q / gain, `* g_i`
// Unop<X, FrameMulScalar>.  The line form outputs and feeds back the filtered line (Feedback, feedback.rs:130-134); the loop form outputs
// the line before the filter and feeds back Hadamard(F(x) * g) (Feedback2::tick feedback.rs:260-264).
//
// As in k_fdn_frames_generic every delay is at least two blocks long, so all ring reads of a 64-frame block are known at its head and the
// FIR, the Hadamard and the ring stores run lane = frame.  The one time-serial part is the filter: the block's FIR outputs go through an
// LDS row per line to lanes 0 .. N-1 (lane = line), each of which walks its line's 64 frames in registers in the reference's operation
// order, and back.  The rows are the feedback rows of the generic kernel (no extra LDS: two workgroups per CU as before).
//
// Parameters live in a device table of FdnxInst entries: one for the whole bank or one per instance (wave-uniform, read with scalar
// loads; the filter coefficients are read per lane by the serial lanes).  The ring capacity is sized from the longest delay of any instance.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "fd_fdn.hpp"   // FdnBus, FdnState

namespace fd {

constexpr int FDNX_NONE = 0, FDNX_LOWPOLE = 1, FDNX_SVF = 2;   // the line filter F
constexpr int FDNX_IN_LINE = 0, FDNX_IN_LOOP = 1;              // fdn(x >> F) | fdn2(x, F)

struct FdnxInst {          // one network's parameters at the bank's sample rate
    int len[32];           // Delay ring length = delay in samples + 1 (delay.rs:108-110)
    float w[3][32];        // FIR weights [tap][line], oldest tap first (fir.rs:57-70)
    float co[6][32];       // filter coefficients [coef][line]: Lowpole coeff, 1 - coeff | FixedSvf a1 a2 a3 m0 m1 m2
    float g[32];           // the `* g` behind the filter
};

struct FdnxConst {
    int lines, taps, nin, nout;   // taps 0: no Fir node in the line (the delay output itself, not 0.0 + 1.0 * d)
    int filter, place, has_gain;
    int cap;                      // slots per ring (power of two >= the longest ring of every instance); rings are cap + 64 floats apart
    float had_scale;              // (1.0 / sqrt(N as f64)) as f32   feedback.rs:57
    size_t ring_stride;           // floats per instance = lines * (cap + 64)
    size_t tab_stride;            // 0: one table entry for all instances | 1: one per instance
    const FdnxInst* tab;
};

struct FdnxDesc {                 // host side: a line network as created (P = per_instance ? instances : 1 parameter sets), of this family
    int lines = 0, taps = 0, nin = 1, nout = 1;   // or of fd_fbdelay.hpp's (nin = nout = lines there)
    int filter = FDNX_NONE, svf_mode = 0, place = FDNX_IN_LINE, per_instance = 0, has_gain = 0;
    int has_outer = 0, reverse = 0;   // the feedback delay banks' outer gain and reverse()
    std::vector<double> delay;    // [P][lines] seconds
    std::vector<float> w;         // [P][lines][taps]
    std::vector<float> cutoff, q, gain, line_gain;   // [P][lines] (empty where the network has none)
    std::vector<float> outer;     // [P] (has_outer)
};

struct FdnxState : FdnState {     // the rings, the write position, the Fir carry and the feedback value of fd_fdn.hpp, and the filters' state
    float* s1;                    // [instances][32] Lowpole::value | FixedSvf ic1eq
    float* s2;                    // [instances][32] FixedSvf ic2eq
};

// host: the parameter table at `sample_rate` (instances entries, or 1) and the constants; returns the shortest delay in samples over all
// instances and lines (the caller applies the two-block rule) and -1 when a ring would exceed 2^18 slots (the per-line part of the table
// is fd_line_table.hpp's, for this family and the feedback delay banks)
int fdnx_make_table(const FdnxDesc& d, size_t instances, double sample_rate, std::vector<FdnxInst>& tab, FdnxConst* c);
// Feedback(2)::reset of either family (`ring_stride`: its constants'): fd_fdn.hpp's kernel, with the filters
inline void fdnx_launch_reset(size_t ring_stride, const FdnxState& s, size_t instances, hipStream_t stream) {
    fdn_launch_reset_state(s, s.s1, s.s2, ring_stride, instances, stream);
}
void fdnx_launch_render(const FdnxConst& c, const FdnxState& s, size_t instances, const float* in, float* out, size_t T, size_t fstride,
                        int layout, int tick_mode, hipStream_t stream, const FdnBus& bus = FdnBus());

}  // namespace fd
