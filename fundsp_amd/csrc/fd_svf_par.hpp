// fd_svf_par.hpp -- the time-parallel form of the fixed-coefficient SVF (tolerance mode only, "svf_exec" = FDSP_SVF_PARALLEL).
//
// With constant coefficients the SVF tick (svf.rs:995-1006) is a linear recurrence in its two-word state s = (ic1eq, ic2eq):
//     s' = A s + b v0,     y = c . s + d v0.
// So a run of frames splits into what the INPUT does from state zero and what the STATE carried into the run does with no input:
//     y[n] = yz[n] + r[n] . s_in,     s_out = P s_in + z,
// where yz / z are the outputs / end state of the run rendered from state (0, 0), r[n] = (dy_n/ds1, dy_n/ds2) and P = A^LC.
// A 64-frame block is cut into K chunks of LC = 64 / K frames; the zero-state passes of the chunks do not depend on one another.
//
// The ORDER of the operations, shared by the kernel (fd_tsp.hpp) and the host check (tests/host/check_svf_par.hip):
//   tables (per voice, per launch)  svfp_tables: the reference tick in f64 on zero input for LC frames from state (1, 0) and from
//                                   state (0, 1); every table entry is rounded to f32 once.  Outputs -> r[n].x / r[n].y, end states ->
//                                   the columns of P.
//   chunk pass                      svfp_tick<float> from state (0, 0) over the chunk's LC frames: the reference's operations in the
//                                   reference's order (SvfCore::tick), nothing contracted.  Leaves yz[n] and z_c.
//   fix-up, chunk c = 0 .. K-1      svfp_fix:    y[n] = yz[n] + fma(r.x, s_c.x, r.y * s_c.y)              for the chunk's LC frames, then
//                                   svfp_carry:  s_{c+1}.x = fma(P00, s_c.x, P01 * s_c.y) + z_c.x         (.y: P10, P11, z_c.y)
//                                   s_0 = the state carried in from the previous block, s_K goes to the next one (and to ic1eq / ic2eq).
// Every operation is f32 but the table build.  The two FMAs of svfp_fix / svfp_carry are explicit and everything else is kept
// uncontracted (pragma below, and the library is built with -ffp-contract=off): host and device compute the same bits.  Checked:
// tests/svf_par_ref.py restates this order in numpy, tests/test_svf_par_ref.py holds a host build of this header to it and
// tests/test_gpu_svf_par_bits.py the kernel, frames and end state, as uint32.
//
// Accuracy (tests/test_svf_par_host.py): a chunk pass starts from zero, so its rounding errors grow over LC frames
// instead of the whole launch, and the carried state goes through ONE rounded 2 x 2 product per chunk instead of LC ticks -- against an
// f64 rendering the chunked form is closer than the serial f32 tick bank-wide.
// Plain C++ with the HIP qualifiers where a HIP compiler reads it.
#pragma once

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define FD_SVFP_HD __host__ __device__ inline
#else
#define FD_SVFP_HD inline
#endif

namespace fd {

struct SvfpCoefs { float a1, a2, a3, m0, m1, m2; };

// one tick in the reference's operation order; F = float (chunk pass, serial check) or double (tables, truth)
template <class F>
FD_SVFP_HD F svfp_tick(F a1, F a2, F a3, F m0, F m1, F m2, F& ic1eq, F& ic2eq, F v0) {
#pragma clang fp contract(off)
    const F v3 = v0 - ic2eq;
    const F v1 = a1 * ic1eq + a2 * v3;
    const F v2 = ic2eq + a2 * ic1eq + a3 * v3;
    ic1eq = F(2) * v1 - ic1eq;
    ic2eq = F(2) * v2 - ic2eq;
    return m0 * v0 + m1 * v1 + m2 * v2;
}
FD_SVFP_HD float svfp_tick(const SvfpCoefs& k, float& ic1eq, float& ic2eq, float v0) {
    return svfp_tick<float>(k.a1, k.a2, k.a3, k.m0, k.m1, k.m2, ic1eq, ic2eq, v0);
}

template <int LC>
struct SvfpTables {
    float rx[LC], ry[LC];      // r[n] = (dy_n / d ic1eq, dy_n / d ic2eq) of the state at the chunk's start
    float p00, p01, p10, p11;  // P = A^LC: the chunk's end state from its start state, no input
};

template <int LC>
FD_SVFP_HD void svfp_tables(const SvfpCoefs& k, SvfpTables<LC>& t) {
    const double a1 = k.a1, a2 = k.a2, a3 = k.a3, m0 = k.m0, m1 = k.m1, m2 = k.m2;
    double s1 = 1.0, s2 = 0.0;
#pragma unroll
    for (int n = 0; n < LC; n++) t.rx[n] = (float)svfp_tick<double>(a1, a2, a3, m0, m1, m2, s1, s2, 0.0);
    t.p00 = (float)s1;
    t.p10 = (float)s2;
    s1 = 0.0, s2 = 1.0;
#pragma unroll
    for (int n = 0; n < LC; n++) t.ry[n] = (float)svfp_tick<double>(a1, a2, a3, m0, m1, m2, s1, s2, 0.0);
    t.p01 = (float)s1;
    t.p11 = (float)s2;
}

// one frame of the fix-up: the zero-state output plus what the chunk's start state (s1, s2) adds to it
FD_SVFP_HD float svfp_fix(float yz, float rx, float ry, float s1, float s2) {
#pragma clang fp contract(off)
    return yz + __builtin_fmaf(rx, s1, ry * s2);
}
// the state at the start of the next chunk, from this chunk's start state and its zero-state end state (z1, z2)
template <int LC>
FD_SVFP_HD void svfp_carry(const SvfpTables<LC>& t, float& s1, float& s2, float z1, float z2) {
#pragma clang fp contract(off)
    const float n1 = __builtin_fmaf(t.p00, s1, t.p01 * s2) + z1;
    const float n2 = __builtin_fmaf(t.p10, s1, t.p11 * s2) + z2;
    s1 = n1;
    s2 = n2;
}

// One 64-frame block in the order above, on one thread: what the K chunk waves and the fix-up wave of k_render_ts3p compute between
// them (the host check runs this; the kernel calls the same three functions with the tiles in LDS in between).
template <int LC>
FD_SVFP_HD void svfp_block(const SvfpCoefs& k, const SvfpTables<LC>& t, const float* in, float* out, float& s1, float& s2) {
    constexpr int K = 64 / LC;
    static_assert(K * LC == 64, "chunks tile the block");
    float yz[64], z1[K], z2[K];
    for (int c = 0; c < K; c++) {  // chunk pass
        z1[c] = 0.0f, z2[c] = 0.0f;
        for (int n = 0; n < LC; n++) yz[c * LC + n] = svfp_tick(k, z1[c], z2[c], in[c * LC + n]);
    }
    for (int c = 0; c < K; c++) {  // fix-up
        for (int n = 0; n < LC; n++) out[c * LC + n] = svfp_fix(yz[c * LC + n], t.rx[n], t.ry[n], s1, s2);
        svfp_carry(t, s1, s2, z1[c], z2[c]);
    }
}

}  // namespace fd
