// fd_math.hpp -- numeric substrate of the MI355X voice-bank engine (host + gfx950 device).
//
// FunDSP's scalar `Float`/`Real` traits dispatch f32 math to the `libm` crate and its SIMD block path to
// `wide::f32x8` (reference src/lib.rs:180-222, 296-335, 444-492, 596-670, 773-798).  To be sample-compatible
// with the reference's CPU `tick`/`process` the engine evaluates the SAME published algorithms instead of the
// GPU's own approximations (`__sinf`, `v_sin_f32` ...):
//   * libm 0.2 = musl/FreeBSD msun: sinf/cosf/tanf reduce by quadrant and evaluate the double-precision
//     kernels __sindf/__cosdf/__tandf; tanhf is built on expm1f.
//   * wide f32x8::sin = Agner Fog vectorclass sincos_f (Cody-Waite reduction + Cephes f32 polynomials),
//     unfused mul/add (default x86-64 build has no `fma` target feature).
// The f64 kernels cost 2x an f32 VALU op on CDNA4 (FP64 vector = half rate) and only run in `tick` mode and in
// coefficient updates; the block (`process`) path of Sine uses the all-f32 wide polynomial.
//
// Every function is written branch-light for wave64 execution: lanes of one wave hold different voices, so
// range selection is done with selects on a shared evaluation instead of divergent branches.
// Build with -ffp-contract=off: Rust never contracts a*b+c and parity with the CPU path depends on it.
#pragma once

#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#else  // hiprtc (fd_jit.hip): no system headers; its built-in runtime header keeps the fixed-width types in a namespace
using __hip_internal::int32_t;
using __hip_internal::int64_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
typedef unsigned long uintptr_t;
#endif

#define FD_HD __host__ __device__ __forceinline__

namespace fd {

constexpr float F32_PI = 3.14159274101257324f;   // core::f32::consts::PI
constexpr float F32_TAU = 6.28318548202514648f;  // core::f32::consts::TAU
constexpr float F32_SQRT_2 = 1.41421353816986084f;

FD_HD uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
FD_HD float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }

// ---- musl k_sinf.c / k_cosf.c / k_tanf.c ---------------------------------------------------------------
constexpr double S1 = -0x15555554cbac77.0p-55, S2 = 0x111110896efbb2.0p-59, S3 = -0x1a00f9e2cae774.0p-65,
                 S4 = 0x16cd878c3b46a7.0p-71;
constexpr double C0 = -0x1ffffffd0c5e81.0p-54, C1 = 0x155553e1053a42.0p-57, C2 = -0x16c087e80f1e27.0p-62,
                 C3 = 0x199342e0ee5069.0p-68;

FD_HD float k_sindf(double x) {
    double z = x * x;
    double w = z * z;
    double r = S3 + z * S4;
    double s = z * x;
    return (float)((x + s * (S1 + z * S2)) + s * w * r);
}
FD_HD float k_cosdf(double x) {
    double z = x * x;
    double w = z * z;
    double r = C2 + z * C3;
    return (float)(((1.0 + z * C0) + w * C1) + (w * z) * r);
}
FD_HD float k_tandf(double x, bool odd) {
    constexpr double T0 = 0x15554d3418c99f.0p-54, T1 = 0x1112fd38999f72.0p-55, T2 = 0x1b54c91d865afe.0p-57,
                     T3 = 0x191df3908c33ce.0p-58, T4 = 0x185dadfcecf44e.0p-61, T5 = 0x1362b9bf971bcd.0p-59;
    double z = x * x;
    double r = T4 + z * T5;
    double t = T2 + z * T3;
    double w = z * z;
    double s = z * x;
    double u = T0 + z * T1;
    r = (x + s * u) + (s * w) * (t + w * r);
    return (float)(odd ? -1.0 / r : r);
}

constexpr double PIO2 = 1.570796326794896558e+00;  // M_PI_2

#define FD_COLD __host__ __device__ inline __attribute__((noinline))

// musl __rem_pio2_large.c (libm crate src/math/rem_pio2_large.rs), the Payne-Hanek reduction, for the f32 callers:
// one 24-bit chunk x0 in [2^23, 2^24) (nx = 1, jx = 0), prec = 0 (jk = jp = 3).  Same loops, same order of operations
// as the published routine; only reached for |x| >= 2^28*pi/2, so it lives out of line (its arrays are scratch memory).
FD_COLD int rem_pio2_large1(double x0, int e0, double* y) {
    // ipio2[]: the bits of 2/pi in 24-bit pieces; PIo2[]: pi/2 in 24-bit-mantissa pieces (musl tables)
    static constexpr int32_t IPIO2[66] = {
        0xA2F983, 0x6E4E44, 0x1529FC, 0x2757D1, 0xF534DD, 0xC0DB62, 0x95993C, 0x439041, 0xFE5163, 0xABDEBB, 0xC561B7,
        0x246E3A, 0x424DD2, 0xE00649, 0x2EEA09, 0xD1921C, 0xFE1DEB, 0x1CB129, 0xA73EE8, 0x8235F5, 0x2EBB44, 0x84E99C,
        0x7026B4, 0x5F7E41, 0x3991D6, 0x398353, 0x39F49C, 0x845F8B, 0xBDF928, 0x3B1FF8, 0x97FFDE, 0x05980F, 0xEF2F11,
        0x8B5A0A, 0x6D1F6D, 0x367ECF, 0x27CB09, 0xB74F46, 0x3F669E, 0x5FEA2D, 0x7527BA, 0xC7EBE5, 0xF17B3D, 0x0739F7,
        0x8A5292, 0xEA6BFB, 0x5FB11F, 0x8D5D08, 0x560330, 0x46FC7B, 0x6BABF0, 0xCFBC20, 0x9AF436, 0x1DA9E3, 0x91615E,
        0xE61B08, 0x659985, 0x5F14A0, 0x68408D, 0xFFD880, 0x4D7327, 0x310606, 0x1556CA, 0x73A8C9, 0x60E27B, 0xC08C6B};
    static constexpr double PIO2_CHUNKS[8] = {
        1.57079625129699707031e+00, 7.54978941586159635335e-08, 5.39030252995776476554e-15, 3.28200341580791294123e-22,
        1.27065575308067607349e-29, 1.22933308981111328932e-36, 2.73370053816464559624e-44, 2.16741683877804819444e-51,
    };
    constexpr int jk = 3, jp = 3;
    int32_t jz, jv, carry, n, iq[20], i, j, k, q0, ih;
    double z, fw, f[20], fq[20], q[20];
    jv = (e0 - 3) / 24;
    if (jv < 0) jv = 0;
    q0 = e0 - 24 * (jv + 1);
    for (i = 0, j = jv; i <= jk; i++, j++) f[i] = (double)IPIO2[j];
    for (i = 0; i <= jk; i++) q[i] = 0.0 + x0 * f[i];
    jz = jk;
    for (;;) {
        for (i = 0, j = jz, z = q[jz]; j > 0; i++, j--) {  // distill q[] into iq[] reversingly
            fw = (double)(int32_t)(0x1p-24 * z);
            iq[i] = (int32_t)(z - 0x1p24 * fw);
            z = q[j - 1] + fw;
        }
        z = __builtin_scalbn(z, q0);
        z -= 8.0 * __builtin_floor(z * 0.125);
        n = (int32_t)z;
        z -= (double)n;
        ih = 0;
        if (q0 > 0) {
            i = iq[jz - 1] >> (24 - q0);
            n += i;
            iq[jz - 1] -= i << (24 - q0);
            ih = iq[jz - 1] >> (23 - q0);
        } else if (q0 == 0)
            ih = iq[jz - 1] >> 23;
        else if (z >= 0.5)
            ih = 2;
        if (ih > 0) {  // q > 0.5
            n += 1;
            carry = 0;
            for (i = 0; i < jz; i++) {
                j = iq[i];
                if (carry == 0) {
                    if (j != 0) {
                        carry = 1;
                        iq[i] = 0x1000000 - j;
                    }
                } else
                    iq[i] = 0xffffff - j;
            }
            if (q0 == 1) iq[jz - 1] &= 0x7fffff;
            if (q0 == 2) iq[jz - 1] &= 0x3fffff;
            if (ih == 2) {
                z = 1.0 - z;
                if (carry != 0) z -= __builtin_scalbn(1.0, q0);
            }
        }
        if (z != 0.0) break;
        j = 0;
        for (i = jz - 1; i >= jk; i--) j |= iq[i];
        if (j != 0) break;
        for (k = 1; iq[jk - k] == 0; k++) {}  // recomputation: k more terms
        for (i = jz + 1; i <= jz + k; i++) {
            f[i] = (double)IPIO2[jv + i];
            q[i] = 0.0 + x0 * f[i];
        }
        jz += k;
    }
    if (z == 0.0) {  // chop off zero terms
        jz -= 1;
        q0 -= 24;
        while (iq[jz] == 0) {
            jz--;
            q0 -= 24;
        }
    } else {  // break z into 24-bit if necessary
        z = __builtin_scalbn(z, -q0);
        if (z >= 0x1p24) {
            fw = (double)(int32_t)(0x1p-24 * z);
            iq[jz] = (int32_t)(z - 0x1p24 * fw);
            jz += 1;
            q0 += 24;
            iq[jz] = (int32_t)fw;
        } else
            iq[jz] = (int32_t)z;
    }
    fw = __builtin_scalbn(1.0, q0);
    for (i = jz; i >= 0; i--) {
        q[i] = fw * (double)iq[i];
        fw *= 0x1p-24;
    }
    for (i = jz; i >= 0; i--) {
        for (fw = 0.0, k = 0; k <= jp && k <= jz - i; k++) fw += PIO2_CHUNKS[k] * q[i + k];
        fq[jz - i] = fw;
    }
    fw = 0.0;
    for (i = jz; i >= 0; i--) fw += fq[i];
    *y = ih == 0 ? fw : -fw;
    return n & 7;
}

// musl __rem_pio2f.c (libm crate src/math/rem_pio2f.rs): medium branch for |x| < 2^28*pi/2, the rest through
// __rem_pio2_large on the mantissa scaled into [2^23, 2^24).  inf / NaN are handled by the callers.
FD_HD int rem_pio2f(float x, double* y) {
    constexpr double toint = 1.5 / 2.22044604925031308085e-16, invpio2 = 6.36619772367581382433e-01,
                     pio2_1 = 1.57079631090164184570e+00, pio2_1t = 1.58932547735281966916e-08;
    const uint32_t ix = f2u(x) & 0x7fffffffu;
    if (ix >= 0x4dc90fdbu) {
        const int e0 = (int)(ix >> 23) - (0x7f + 23);
        double ty;
        const int n = rem_pio2_large1((double)u2f(ix - ((uint32_t)e0 << 23)), e0, &ty);
        const bool sign = (f2u(x) >> 31) != 0;
        *y = sign ? -ty : ty;
        return sign ? -n : n;
    }
    double fn = (double)x * invpio2 + toint - toint;
    int n = (int32_t)fn;
    *y = x - fn * pio2_1 - fn * pio2_1t;
    return n;
}

// Quadrant decode shared by sinf/cosf/tanf: k = number of pi/2 steps removed (0..4) for |x| <= 9pi/4,
// y = reduced argument carrying the sign handling of musl's explicit cases.
struct quad {
    double y;
    int k;
    bool sign, small, big;
};
FD_HD quad quad_reduce(float x) {
    quad q;
    uint32_t ix = f2u(x);
    q.sign = (ix >> 31) != 0;
    ix &= 0x7fffffffu;
    q.small = ix < 0x39800000u;  // |x| < 2**-12
    q.big = ix > 0x40e231d5u;    // |x| > 9*pi/4 (or inf/nan)
    int k = (ix > 0x3f490fdau) + (ix > 0x4016cbe3u) + (ix > 0x407b53d1u) + (ix > 0x40afeddfu);
    double c = (double)k * PIO2;  // k*M_PI_2 rounded once, identical to musl's compile-time s{k}pio2 constants
    q.k = k;
    q.y = k == 0 ? (double)x : (q.sign ? (double)x + c : (double)x - c);
    return q;
}

// |x| > 9*pi/4, inf, NaN: musl's rem_pio2f branches.  Never taken by wrapped phases or filter arguments, so they live
// out of line: inlined into every kernel they would only bloat the code around the hot loops.
FD_COLD float sinf_big(float x) {
    uint32_t ix = f2u(x) & 0x7fffffffu;
    if (ix >= 0x7f800000u) return x - x;
    double y;
    int n = rem_pio2f(x, &y);
    switch (n & 3) {
    case 0: return k_sindf(y);
    case 1: return k_cosdf(y);
    case 2: return k_sindf(-y);
    default: return -k_cosdf(y);
    }
}
FD_COLD float cosf_big(float x) {
    uint32_t ix = f2u(x) & 0x7fffffffu;
    if (ix >= 0x7f800000u) return x - x;
    double y;
    int n = rem_pio2f(x, &y);
    switch (n & 3) {
    case 0: return k_cosdf(y);
    case 1: return k_sindf(-y);
    case 2: return -k_cosdf(y);
    default: return k_sindf(y);
    }
}
FD_COLD float tanf_big(float x) {
    uint32_t ix = f2u(x) & 0x7fffffffu;
    if (ix >= 0x7f800000u) return x - x;
    double y;
    int n = rem_pio2f(x, &y);
    return k_tandf(y, (n & 1) != 0);
}

// musl sinf.c
FD_HD float sinf_musl(float x) {
    quad q = quad_reduce(x);
    if (__builtin_expect(q.big, 0)) return sinf_big(x);
    // k=0: sindf(x); k=1: sign ? -cosdf(y) : cosdf(y); k=2: sindf(-y); k=3: sign ? cosdf(y) : -cosdf(y); k=4: sindf(y)
    double a = q.k == 2 ? -q.y : q.y;
    float s = k_sindf(a);
    float c = k_cosdf(a);
    bool use_cos = (q.k & 1) != 0;
    bool neg = use_cos && ((q.k == 1) == q.sign);
    float r = use_cos ? c : s;
    r = neg ? -r : r;
    return q.small ? x : r;
}

// musl cosf.c
FD_HD float cosf_musl(float x) {
    quad q = quad_reduce(x);
    if (__builtin_expect(q.big, 0)) return cosf_big(x);
    // k=0: cosdf(x); k=1: sign ? sindf(x+c) : sindf(c-x); k=2: -cosdf(y); k=3: sign ? sindf(-x-c) : sindf(x-c); k=4: cosdf(y)
    double a = q.y;
    if (q.k == 1) a = q.sign ? q.y : -q.y;
    if (q.k == 3) a = q.sign ? -q.y : q.y;
    float s = k_sindf(a);
    float c = k_cosdf(a);
    bool use_sin = (q.k & 1) != 0;
    float r = use_sin ? s : (q.k == 2 ? -c : c);
    return q.small ? 1.0f : r;
}

// musl tanf.c
FD_HD float tanf_musl(float x) {
    quad q = quad_reduce(x);
    if (__builtin_expect(q.big, 0)) return tanf_big(x);
    float r = k_tandf(q.y, (q.k & 1) != 0);
    return q.small ? x : r;
}

// musl expm1f.c, evaluated branch-light: the argument-reduction case (k, hi, lo) and the reconstruction case are
// chosen with selects around ONE shared polynomial, because the lanes of a wave (different voices) fall into
// different cases on almost every sample and divergent branches would execute every path.  Each lane still
// performs exactly the operations of the case musl would take for it, in the same order.
FD_HD float expm1f_musl(float x0) {
    constexpr float ln2_hi = 6.9313812256e-01f, ln2_lo = 9.0580006145e-06f, invln2 = 1.4426950216e+00f,
                    Q1 = -3.3333212137e-2f, Q2 = 1.5807170421e-3f;
    const uint32_t ui = f2u(x0);
    const uint32_t hx = ui & 0x7fffffffu;
    const bool sign = (ui >> 31) != 0;
    // early-outs that do not use the polynomial (rare: huge |x|, NaN, tiny |x|)
    const bool is_nan = hx > 0x7f800000u;
    const bool big = hx >= 0x4195b844u;               // |x| >= 27*ln2
    const bool ovf = big && !sign && x0 > 8.8721679688e+01f;
    const bool tiny = hx < 0x33000000u;               // |x| < 2**-25
    // argument reduction
    const bool reduce = hx > 0x3eb17218u;             // |x| > 0.5 ln2
    const bool near1 = hx < 0x3F851592u;              // |x| < 1.5 ln2
    // (every arm of a case is evaluated into a named value first and then selected: an arithmetic expression inside
    // `?:` comes out of the compiler as a divergent branch, and the one wave that runs a ladder filter pays for each)
    const float half = sign ? -0.5f : 0.5f;
    int kg = (int)(invln2 * x0 + half);
    float tg = (float)kg;
    const int k1 = sign ? -1 : 1;
    int k = reduce ? (near1 ? k1 : kg) : 0;
    const float ln2_hi_s = sign ? -ln2_hi : ln2_hi;   // x0 + ln2_hi == x0 - (-ln2_hi): one subtraction either way
    const float hi_near = x0 - ln2_hi_s, hi_far = x0 - tg * ln2_hi;
    const float lo_near = sign ? -ln2_lo : ln2_lo, lo_far = tg * ln2_lo;
    float hi = near1 ? hi_near : hi_far;
    float lo = near1 ? lo_near : lo_far;
    float xr = hi - lo;
    float cr = (hi - xr) - lo;
    float x = reduce ? xr : x0;
    float c = reduce ? cr : 0.0f;
    // primary range
    float hfx = 0.5f * x;
    float hxs = x * hfx;
    float r1 = 1.0f + hxs * (Q1 + hxs * Q2);
    float t = 3.0f - r1 * hfx;
    float e = hxs * ((r1 - t) / (6.0f - x * t));
    float res_k0 = x - (x * e - hxs);
    float e2 = x * (e - c) - c;
    e2 -= hxs;
    float res_km1 = 0.5f * (x - e2) - 0.5f;
    const float res_k1a = -2.0f * (e2 - (x + 0.5f)), res_k1b = 1.0f + 2.0f * (x - e2);
    float res_k1 = x < -0.25f ? res_k1a : res_k1b;
    float twopk = u2f((uint32_t)(0x7f + k) << 23);
    float y_out = x - e2 + 1.0f;
    const float y_out128 = y_out * 2.0f * 0x1p127f, y_outk = y_out * twopk;
    y_out = (k == 128) ? y_out128 : y_outk;
    float res_out = y_out - 1.0f;                      // k < 0 || k > 56
    float uf = u2f((uint32_t)(0x7f - k) << 23);
    float res_lt23 = (x - e2 + (1 - uf)) * twopk;
    float res_ge23 = (x - (e2 + uf) + 1) * twopk;
    float res = (k < 23) ? res_lt23 : res_ge23;
    res = (k < 0 || k > 56) ? res_out : res;
    res = (k == 1) ? res_k1 : res;
    res = (k == -1) ? res_km1 : res;
    res = (k == 0) ? res_k0 : res;
    res = tiny ? x0 : res;
    res = ovf ? x0 * 0x1p127f : res;
    res = (big && sign) ? -1.0f : res;
    res = is_nan ? x0 : res;
    return res;
}

typedef float v2f __attribute__((ext_vector_type(2)));  // one v_pk_*_f32 operand: two f32 in a VGPR pair

FD_HD v2f splat2(float x) { return v2f{x, x}; }

// n / d for operands that need none of the IEEE division's range handling (no denormal, no overflow, quotient far from
// both): the device's f32 division is v_div_scale x2, v_rcp, four fma / one mul of Newton-Raphson and residual
// correction, v_div_fmas, v_div_fixup; with nothing to scale, v_div_scale passes its operand through, v_div_fmas is an
// fma and v_div_fixup returns the quotient -- the same eight arithmetic instructions remain, three fewer in all.
// tanhf_musl uses it for both of its divisions; that this changes no result is checked, not argued: all 2^32 inputs on
// the device against the oracle, in the default mode and with denormals flushed (tests/host/check_tanh_device.hip).
FD_HD float div_inrange(float n, float d) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r = __builtin_amdgcn_rcpf(d);
    const float e0 = __builtin_fmaf(-d, r, 1.0f);
    r = __builtin_fmaf(e0, r, r);
    float q = n * r;
    const float e1 = __builtin_fmaf(-d, q, n);
    q = __builtin_fmaf(e1, r, q);
    const float e2 = __builtin_fmaf(-d, q, n);
    return __builtin_fmaf(e2, r, q);
#else
    return n / d;
#endif
}

// musl tanhf.c: t = expm1f(+-2|x|), then one division.  expm1f is restated here for the arguments tanhf can hand it,
// a = 2|x| for |x| > log(5/3)/2 and a = -2|x| below -- that removes the cases a ladder filter's one wave would otherwise
// evaluate and discard on every sample:
//   a < 0:  |a| <= 0.5108 < 1.5 ln2, so k = 0 (|a| <= 0.5 ln2, no reduction) or k = -1;
//   a > 0:  a > 0.5108 > 0.5 ln2, so k = 1 (a < 1.5 ln2) or k = (int)(invln2 a + 0.5) = 2 .. 29 (a <= 20; beyond that
//           tanhf's own |x| > 10 case overrides); for k = 1 the reduced argument is > -0.19, never the x < -0.25 form;
//   never:  k < -1, k > 56, the |a| >= 27 ln2 early-outs (only with |x| > 10 or NaN, both overridden).
// hi = a - k ln2_hi, lo = k ln2_lo also cover musl's k = +-1 special forms: a product with +-1 is exact.
// Each lane performs exactly the operations musl performs for its case (tests/host/check_tanh_expm1.hip: bit-identical
// to the branch-form oracle).
FD_HD float tanhf_musl(float x0) {
    constexpr float ln2_hi = 6.9313812256e-01f, ln2_lo = 9.0580006145e-06f, invln2 = 1.4426950216e+00f,
                    Q1 = -3.3333212137e-2f, Q2 = 1.5807170421e-3f;
    uint32_t w = f2u(x0);
    const bool sign = (w >> 31) != 0;
    w &= 0x7fffffffu;
    const float x = u2f(w);
    const bool c_big = w > 0x41200000u;    // |x| > 10
    const bool c1 = w > 0x3f0c9f54u;       // |x| > log(3)/2
    const bool c2 = w > 0x3e82c578u;       // |x| > log(5/3)/2
    const bool c3 = w >= 0x00800000u;      // normal
    const bool is_nan = w > 0x7f800000u;
    // ---- t = expm1f(a) ----
    const float two_x = 2 * x;
    const float a = c2 ? two_x : -two_x;
    const uint32_t ha = f2u(two_x);               // |a|
    const bool reduce = ha > 0x3eb17218u;         // |a| > 0.5 ln2
    const bool near1 = ha < 0x3F851592u;          // |a| < 1.5 ln2
    const int kg = (int)(invln2 * a + 0.5f);
    const float tg = (float)kg;
    const float tpos = near1 ? 1.0f : tg;
    const int kpos = near1 ? 1 : kg;
    const float tk = c2 ? tpos : -1.0f;
    const int k = c2 ? kpos : -1;                 // (used only where reduce holds)
    const float hi = a - tk * ln2_hi;
    const float lo = tk * ln2_lo;
    const float xr = hi - lo;
    const float cr = (hi - xr) - lo;
    const float xx = reduce ? xr : a;
    const float c = reduce ? cr : 0.0f;
    const float hfx = 0.5f * xx;
    const float hxs = xx * hfx;
    const float r1 = 1.0f + hxs * (Q1 + hxs * Q2);
    const float tt = 3.0f - r1 * hfx;
    const float e = hxs * div_inrange(r1 - tt, 6.0f - xx * tt);  // numerator ~ -2, denominator in [4.9, 7.1]
    const float res_k0 = xx - (xx * e - hxs);
    float e2 = xx * (e - c) - c;
    e2 -= hxs;
    const float res_km1 = 0.5f * (xx - e2) - 0.5f;
    // (k = 1: musl's 1 + 2 (x - e) and the k < 23 form ((x - e) + 0.5) * 2 are the same bits -- a scaling by two commutes
    // with the rounding of the sum --, so k = 1 takes the general form; the exhaustive device check covers it)
    const float twopk = u2f(((uint32_t)0x7f + (uint32_t)k) << 23);
    const float uf = u2f(((uint32_t)0x7f - (uint32_t)k) << 23);
    const float res_lt23 = (xx - e2 + (1 - uf)) * twopk;
    const float res_ge23 = (xx - (e2 + uf) + 1) * twopk;
    const float res_pos = (k < 23) ? res_lt23 : res_ge23;
    const float res_neg = reduce ? res_km1 : res_k0;
    const float t = c2 ? res_pos : res_neg;
    // (musl returns a itself for |a| < 2**-25; the k = 0 form gives the same bits there -- a + a*a/2 rounds to a --,
    // which the exhaustive device check confirms, so the case needs no select)
    // ---- tanhf ----
    const float mt = -t;
    const float num_small = c2 ? t : mt;
    const float num = c1 ? 2.0f : num_small;
    const float quo = div_inrange(num, t + 2);
    const float one_minus = 1 - quo;
    float r = c1 ? one_minus : quo;        // c1: 1 - 2/(t+2); c2: t/(t+2); c3: -t/(t+2)
    // |x| > 10 and NaN: musl's 1 + 0/x, without the division (a division inside `?:` becomes a divergent branch):
    // 0/x is +0 for every finite or infinite x > 10 and the quieted x for a NaN, so the sum is 1, or x + 1 for a NaN
    const float x_plus_1 = x + 1.0f;
    const float r_big = is_nan ? x_plus_1 : 1.0f;
    r = c_big ? r_big : r;                 // (a NaN is > 10 as a bit pattern: it takes this arm, as in musl)
    r = c3 ? r : x;                        // subnormal: t = x
    return sign ? -r : r;
}

// tanhf_musl for the arguments a ladder filter sees on (nearly) every sample: |x| <= 7.5, not NaN.  Outside that range --
// musl's |x| > 10 and NaN arms, and the k >= 23 form of expm1f's reconstruction (|x| >= 7.97) -- `wmax`, the running maximum
// of the argument's magnitude BITS (one v_max_u32; a NaN's bits exceed every finite value's), makes the caller re-render
// the tile with tanhf_musl (Moog::tripped, the rollback every packed-path shortcut of the engine uses).
//
// The ladder evaluates this once per sample on its one-sample feedback loop, where every instruction is an issue slot of the
// stage's single wave (~4.4 cycles) whatever its data dependencies: the instruction COUNT is the cost (config 4: 99 slots per
// sample for ladder + tanhf_musl-by-selects in round 2, 69 now).  Inside the guarded range the function is a function of ONE
// f32, so every shortening is proven by enumeration, not argued: tests/host/check_tanh_common_device.hip compares it with the
// device build of tanhf_musl on all 2^32 bit patterns, with denormals kept and flushed (profiles/r03_tanh_common_device_
// exhaustive.txt; its control -- FD_TANH_DIV_B=3, a quotient without any correction -- differs on 153 M patterns).  What the
// enumeration licenses:
//   * ONE form for every case.  musl's expm1f has special forms for k = 0, k = -1 and k = 1; each is the k-general form
//     (x - e + (1 - 2^-k)) 2^k with exact steps added or removed (c = 0, 2^-k = 1, 2^k = 1 for k = 0; a scaling by two
//     commutes with a rounding for k = +-1), so every lane runs the general form with its own k and the only selects left are
//     the sign of a = +-2|x| and tanhf's own |x| > log(3)/2.
//   * k = rint(invln2 a) instead of (int)(invln2 a +- 0.5) and the k = +-1 shortcuts: the same k on every reachable a.
//   * the two divisions as rcp, q = n r, one residual correction (4 instructions, div_common<2>): the textbook sequence with a
//     Newton step on r and two corrections is what rounds correctly for EVERY operand pair; on the 2^31 pairs that occur
//     here the short one gives the same bits.
//   * the numerator of tanhf's quotient as |t| (t > 0 for a > 0, t <= 0 for a < 0), and the sign put back with one v_bfi
//     (the magnitude is tanh |x| >= 0).
//   * two packed instructions for the two pairs of independent like operations (k {ln2_hi, ln2_lo}; {r1, 6} - {tt, x tt}).
// Host builds divide with `/` (tests/host/check_tanh_expm1.hip --common: all bit patterns against the branch-form oracle).
constexpr uint32_t TANH_COMMON_MAX_BITS = 0x40f00000u;  // 7.5f
#ifndef FD_FTZ
#define FD_FTZ 0             // 1 in translation units built with -fgpu-flush-denormals-to-zero (fd_fdn.hip, fd_jit.hip's Feedback graphs)
#endif
template <int LEVEL>
FD_HD float div_common(float n, float d) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (LEVEL == 0) return div_inrange(n, d);
    float r = __builtin_amdgcn_rcpf(d);
    if (LEVEL == 1) {
        const float e0 = __builtin_fmaf(-d, r, 1.0f);
        r = __builtin_fmaf(e0, r, r);
    }
    const float q = n * r;
    if (LEVEL == 3) return q;  // (NOT exact: the sensitivity control of the exhaustive check)
    const float e1 = __builtin_fmaf(-d, q, n);
    return __builtin_fmaf(e1, r, q);
#else
    return n / d;
#endif
}
FD_HD float tanhf_common(float x0, uint32_t& wmax) {
    constexpr float ln2_hi = 6.9313812256e-01f, ln2_lo = 9.0580006145e-06f, invln2 = 1.4426950216e+00f,
                    Q1 = -3.3333212137e-2f, Q2 = 1.5807170421e-3f;
    const uint32_t w0 = f2u(x0);
    const uint32_t w = w0 & 0x7fffffffu;
    wmax = wmax > w ? wmax : w;
    const float x = u2f(w);
    const bool c1 = w > 0x3f0c9f54u;       // |x| > log(3)/2:   tanh = 1 - 2 / (expm1(2|x|) + 2)
    const bool c2 = w > 0x3e82c578u;       // |x| > log(5/3)/2: tanh = t / (t + 2), t = expm1(2|x|); below: -t / (t + 2), t = expm1(-2|x|)
    const float two_x = 2 * x;
    const float a = c2 ? two_x : -two_x;
    // ---- expm1f(a), k-general form ----
    const float tk = __builtin_rintf(invln2 * a);
    const int k = (int)tk;
    const v2f hl = splat2(tk) * v2f{ln2_hi, ln2_lo};
    const float hi = a - hl.x;
    const float lo = hl.y;
    const float xx = hi - lo;
    const float c = (hi - xx) - lo;
    const float hfx = 0.5f * xx;
    const float hxs = xx * hfx;
    const float r1 = 1.0f + hxs * (Q1 + hxs * Q2);
    const float tt = 3.0f - r1 * hfx;
    const v2f nd = v2f{r1, 6.0f} - v2f{tt, xx * tt};
    const float e = hxs * div_common<2>(nd.x, nd.y);
    float e2 = xx * (e - c) - c;
    e2 -= hxs;
    const uint32_t kb = (uint32_t)k << 23;
    const float twopk = u2f(0x3f800000u + kb);
    const float uf = u2f(0x3f800000u - kb);
    const float t = (xx - e2 + (1 - uf)) * twopk;          // k < 23 throughout the range
    // ---- tanhf ----
    const float num = c1 ? 2.0f : __builtin_fabsf(t);
    const float quo = div_common<2>(num, t + 2);
    const float one_minus = 1 - quo;
    float r = c1 ? one_minus : quo;
#if FD_FTZ
    // musl returns a zero or subnormal x itself.  With denormals kept the arithmetic above does too (t = -2x exactly,
    // 2x / (2 - 2x) = x); a flush-to-zero build (graphs with a Feedback node) needs the select
    r = (w >= 0x00800000u) ? r : x;
#endif
    return u2f((f2u(r) & 0x7fffffffu) | (w0 & 0x80000000u));
}

// musl atanf.c (FreeBSD s_atanf.c), case selection by selects
FD_HD float atanf_musl(float x0) {
    constexpr float aT0 = 3.3333328366e-01f, aT1 = -1.9999158382e-01f, aT2 = 1.4253635705e-01f,
                    aT3 = -1.0648017377e-01f, aT4 = 6.1687607318e-02f;
    uint32_t ix = f2u(x0);
    const bool sign = (ix >> 31) != 0;
    ix &= 0x7fffffffu;
    if (__builtin_expect(ix >= 0x4c800000u, 0)) {  // |x| >= 2**26
        if (ix > 0x7f800000u) return x0;
        float z = 1.5707962513e+00f + 0x1p-120f;
        return sign ? -z : z;
    }
    const bool small = ix < 0x3ee00000u;  // |x| < 0.4375: no reduction
    const bool tiny = ix < 0x39800000u;   // |x| < 2**-12
    const float ax = __builtin_fabsf(x0);
    int id;
    float num, den;
    if (ix < 0x3f980000u) {      // |x| < 1.1875
        if (ix < 0x3f300000u) {  //  7/16 <= |x| < 11/16
            id = 0; num = 2.0f * ax - 1.0f; den = 2.0f + ax;
        } else {                 // 11/16 <= |x| < 19/16
            id = 1; num = ax - 1.0f; den = ax + 1.0f;
        }
    } else {
        if (ix < 0x401c0000u) {  // |x| < 2.4375
            id = 2; num = ax - 1.5f; den = 1.0f + 1.5f * ax;
        } else {                 // 2.4375 <= |x| < 2**26
            id = 3; num = -1.0f; den = ax;
        }
    }
    const float x = small ? x0 : num / den;
    const float z = x * x, w = z * z;
    const float s1 = z * (aT0 + w * (aT2 + w * aT4));
    const float s2 = w * (aT1 + w * aT3);
    const float hi = id == 0 ? 4.6364760399e-01f : id == 1 ? 7.8539812565e-01f : id == 2 ? 9.8279368877e-01f : 1.5707962513e+00f;
    const float lo = id == 0 ? 5.0121582440e-09f : id == 1 ? 3.7748947079e-08f : id == 2 ? 3.4473217170e-08f : 7.5497894159e-08f;
    const float r_small = x - x * (s1 + s2);
    const float zz = hi - ((x * (s1 + s2) - lo) - x);
    const float r_red = sign ? -zz : zz;
    const float r = small ? r_small : r_red;
    return tiny ? x0 : r;
}

// wide f32x8::atan, one lane (vectorclass atan_f): octant selection + degree-3 polynomial in z^2, unfused
FD_HD float wide_atanf(float self) {
    constexpr float P3 = 8.05374449538E-2f, P2 = -1.38776856032E-1f, P1 = 1.99777106478E-1f, P0 = -3.33329491539E-1f;
    constexpr float SQRT2 = 1.41421356237309504880f, FRAC_PI_2 = 1.57079632679489661923f, FRAC_PI_4 = 0.785398163397448309616f;
    float t = __builtin_fabsf(self);
    bool notsmal = t >= SQRT2 - 1.0f;
    bool notbig = t <= SQRT2 + 1.0f;
    float s = notbig ? FRAC_PI_4 : FRAC_PI_2;
    s = notsmal ? s : 0.0f;
    float a = notbig ? t : 0.0f;
    a = notsmal ? a - 1.0f : a;
    float b = notbig ? 1.0f : 0.0f;
    b = notsmal ? b + t : b;
    float z = a / b;
    float zz = z * z;
    // polynomial_3!(zz, P0, P1, P2, P3) = (P2 + P3*zz)*zz^2 + (P1*zz + P0)
    float z4 = zz * zz;
    float re = (zz * P3 + P2) * z4 + (zz * P1 + P0);
    re = re * (zz * z) + z + s;
    return (f2u(self) >> 31) ? -re : re;
}

// libm roundf (half away from zero) -- musl roundf.c semantics
FD_HD float roundf_musl(float x) { return __builtin_roundf(x); }

// libm 0.2 scalbnf for the normal range used by expf (|k| small)
FD_HD float scalbnf_small(float y, int k) { return y * u2f((uint32_t)(0x7f + k) << 23); }

// musl expf.c (2018, FreeBSD e_expf.c)
FD_HD float expf_musl(float x) {
    constexpr float ln2hi = 6.9314575195e-1f, ln2lo = 1.4286067653e-6f, invln2 = 1.4426950216e+0f,
                    P1 = 1.6666625440e-1f, P2 = -2.7667332906e-3f;
    float hi, lo, c, xx, y;
    int k;
    uint32_t hx = f2u(x);
    int sign = (int)(hx >> 31);
    hx &= 0x7fffffffu;
    if (hx >= 0x42aeac50u) {
        if (hx > 0x7f800000u) return x;
        if (hx >= 0x42b17218u && !sign) {
            x *= 0x1p127f;
            return x;
        }
        if (sign && hx >= 0x42cff1b5u) return 0.0f;
    }
    if (hx > 0x3eb17218u) {
        if (hx > 0x3f851592u)
            k = (int)(invln2 * x + (sign ? -0.5f : 0.5f));
        else
            k = 1 - sign - sign;
        hi = x - k * ln2hi;
        lo = k * ln2lo;
        x = hi - lo;
    } else if (hx > 0x39000000u) {
        k = 0;
        hi = x;
        lo = 0;
    } else {
        return 1 + x;
    }
    xx = x * x;
    c = x - xx * (P1 + xx * P2);
    y = 1 + (x * c / (2 - c) - lo + hi);
    if (k == 0) return y;
    if (k > -126 && k < 128) return scalbnf_small(y, k);
    // subnormal / overflow tails: two-step scaling like scalbnf
    float s1 = scalbnf_small(y, k / 2);
    return scalbnf_small(s1, k - k / 2);
}

// ---- wide f32x8::sin, one lane (all f32, unfused) --------------------------------------------------------
// f32x8::round_int of an integral value: NaN -> 0, saturating at both ends on every platform wide supports (its x86
// form masks NaNs and flips lanes >= 2^31 to i32::MAX around cvtps2dq).  On gfx950 this is what v_cvt_i32_f32 does.
FD_HD int32_t round_int_sat(float y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (int32_t)y;
#else
    return y != y ? 0 : y >= 2147483648.0f ? INT32_MAX : y <= -2147483648.0f ? INT32_MIN : (int32_t)y;
#endif
}
FD_HD float wide_sinf(float self) {
    constexpr float DP1F = 0.78515625f * 2.0f;
    constexpr float DP2F = 2.4187564849853515625E-4f * 2.0f;
    constexpr float DP3F = 3.77489497744594108E-8f * 2.0f;
    constexpr float P0sinf = -1.6666654611E-1f, P1sinf = 8.3321608736E-3f, P2sinf = -1.9515295891E-4f;
    constexpr float P0cosf = 4.166664568298827E-2f, P1cosf = -1.388731625493765E-3f, P2cosf = 2.443315711809948E-5f;
    constexpr float TWO_OVER_PI = 2.0f / 3.14159274101257324f;
    float xa = __builtin_fabsf(self);
    float y = __builtin_rintf(xa * TWO_OVER_PI);  // round half to even (v_rndne_f32)
    int32_t q = round_int_sat(y);
    float x = xa - y * DP1F;
    x = x - y * DP2F;
    x = x - y * DP3F;
    float x2 = x * x;
    float x4 = x2 * x2;
    float s = (x4 * P2sinf + (x2 * P1sinf + P0sinf)) * (x * x2) + x;
    float c = (x4 * P2cosf + (x2 * P1cosf + P0cosf)) * (x2 * x2) + (1.0f - 0.5f * x2);
    bool overflow = (q > 0x2000000) && (xa < __builtin_inff());
    s = overflow ? 0.0f : s;
    c = overflow ? 1.0f : c;
    float sin1 = (q & 1) ? c : s;
    uint32_t sign_sin = ((uint32_t)q << 30) ^ f2u(self);
    return u2f(f2u(sin1) ^ (sign_sin & 0x80000000u));
}

// ---- two-frame packed form of wide_sinf ------------------------------------------------------------------
// A lone wave issues one instruction per ~4 cycles whatever its type (profiles/r01_pmc_sq_run4.txt), and gfx950's
// packed-f32 VALU ops (v_pk_mul_f32 / v_pk_add_f32) do two lanes-ops per issue slot.  The feed-forward part of an
// oscillator (the sine polynomial of frame n and n+1) is therefore evaluated as one <2 x float> computation.
// Component-wise the arithmetic is IDENTICAL to wide_sinf (same operations, same order, no contraction).
// `tmax` accumulates the largest quadrant argument seen (one v_max3_f32): the shortcuts below are exact only while
// it stays < 8192; the caller checks it once per 64-sample block and, if it tripped, re-renders that block with the
// fully general scalar wide_sinf (optimistic execution + rollback keeps the hot loop branch-free).
// The form WITHOUT the tmax operand is for callers that have already established |quadrant index| < 8192 for every argument
// they will pass (SineB::begin_block, fd_nodes.hpp: one check per block from a bound of the node's input); the form WITH it
// is the same evaluation plus the v_max3_f32.
FD_HD v2f wide_sin2(v2f self) {
    constexpr float DP1F = 0.78515625f * 2.0f;                 //  8 significant bits
    constexpr float DP2F = 2.4187564849853515625E-4f * 2.0f;   // 11 significant bits
    constexpr float DP3F = 3.77489497744594108E-8f * 2.0f;
    constexpr float P0sinf = -1.6666654611E-1f, P1sinf = 8.3321608736E-3f, P2sinf = -1.9515295891E-4f;
    constexpr float P0cosf = 4.166664568298827E-2f, P1cosf = -1.388731625493765E-3f, P2cosf = 2.443315711809948E-5f;
    constexpr float TWO_OVER_PI = 2.0f / 3.14159274101257324f;
    constexpr float MAGIC = 12582912.0f;  // 1.5 * 2^23: adding it rounds |t| < 2^22 to the nearest-even integer
    // wide's algorithm works on |self| and restores the sign at the end.  Every operation below is odd- or even-
    // symmetric under round-to-nearest-even, so the SIGNED evaluation gives the same bits with fewer instructions:
    //   t, y, x flip sign with self (products / RNE sums of negated operands are the negated results);
    //   s(-x) = -s(x) and c(-x) = c(x) exactly;  the quadrant index becomes q' = -q (two's complement), whose low
    //   bits satisfy q'&1 == q&1 and, for odd q, bit1(q') == !bit1(q) -- exactly the extra flip sign(self) needs
    //   on the even cosine branch; for even q the odd sine branch carries sign(self) by itself.
    // The single exception is self == -0.0, where the final `poly*(x*x2) + x` sums (+0) + (-0) = +0 while wide
    // returns -0.0 (it flips the sign of sin(+0)): callers divert that argument (Sine::begin_block).
    // Out-of-domain arguments (|quadrant index| >= 8192: more than ~2000 cycles of phase inside one 64-sample block,
    // where the exact-FMA shortcuts and wide's q > 2^25 overflow rule would matter) only raise tmax here.
    v2f t = self * TWO_OVER_PI;
    // round(t) and its low integer bits from one add: for |t| < 2^13 the sum lies in [2^23, 2^24) where ulp = 1, so
    // ym = RNE(t) + MAGIC exactly, y = ym - MAGIC is exact, and mantissa(ym) = 0x400000 + RNE(t) (two's complement).
    v2f ym = t + MAGIC;
    v2f y = ym - MAGIC;
    uint32_t b0 = f2u(ym.x), b1 = f2u(ym.y);
    // |y| < 2^13 is an integer, so y*DP1F (13+8 bits) and y*DP2F (13+11 bits) are exact products: the fused and the
    // unfused forms of `x - y*DPn` round the same real number once -> identical bits.  Likewise 0.5*x2 below.
    v2f x = __builtin_elementwise_fma(y, splat2(-DP1F), self);
    x = __builtin_elementwise_fma(y, splat2(-DP2F), x);
    x = x - y * DP3F;
    v2f x2 = x * x;
    v2f x4 = x2 * x2;
    v2f s = (x4 * P2sinf + (x2 * P1sinf + P0sinf)) * (x * x2) + x;
    v2f c = (x4 * P2cosf + (x2 * P1cosf + P0cosf)) * x4 + __builtin_elementwise_fma(x2, splat2(-0.5f), splat2(1.0f));
    // (forcing v_bfe_i32 + v_bfi_b32 through inline asm instead of the and + cmp + cndmask the optimiser prefers saved
    // nothing: the asm also stopped the 4-pair unrolling of the caller's loop)
#if defined(__HIP_DEVICE_COMPILE__)
    // Odd-quadrant select as v_bfe_i32 (mask = bit 0 sign-extended) + v_bfi_b32 (mask ? c : s), through asm that the
    // optimiser cannot rewrite: left alone it turns the mask select below into v_and + v_cmp + v_cndmask, and a VALU
    // instruction that takes its lane mask from VCC / an SGPR pair costs several issue slots on gfx950
    // (profiles/r03_ubench_issue.txt).  Plain (non-volatile) asm: pure functions of their inputs, free to schedule.
    uint32_t m0, m1, r0, r1;
    asm("v_bfe_i32 %0, %1, 0, 1" : "=v"(m0) : "v"(b0));
    asm("v_bfe_i32 %0, %1, 0, 1" : "=v"(m1) : "v"(b1));
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r0) : "v"(m0), "v"(f2u(c.x)), "v"(f2u(s.x)));
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r1) : "v"(m1), "v"(f2u(c.y)), "v"(f2u(s.y)));
#else
    uint32_t m0 = (uint32_t)((int32_t)(b0 << 31) >> 31), m1 = (uint32_t)((int32_t)(b1 << 31) >> 31);  // odd quadrant
    uint32_t r0 = (f2u(c.x) & m0) | (f2u(s.x) & ~m0);
    uint32_t r1 = (f2u(c.y) & m1) | (f2u(s.y) & ~m1);
#endif
    return v2f{u2f(r0 ^ ((b0 << 30) & 0x80000000u)), u2f(r1 ^ ((b1 << 30) & 0x80000000u))};
}
FD_HD v2f wide_sin2(v2f self, float& tmax) {
    constexpr float TWO_OVER_PI = 2.0f / 3.14159274101257324f;
    v2f t = self * TWO_OVER_PI;  // (the same product as in wide_sin2(self): one instruction after CSE)
    tmax = __builtin_fmaxf(__builtin_fmaxf(tmax, __builtin_fabsf(t.x)), __builtin_fabsf(t.y));  // one v_max3_f32 per pair
    return wide_sin2(self);
}

// Scalar twin of wide_sin2 (same signed evaluation, same guard): used where two plain VALU ops beat one packed op.
FD_HD float wide_sin1(float self, float& tmax) {
    constexpr float DP1F = 0.78515625f * 2.0f, DP2F = 2.4187564849853515625E-4f * 2.0f, DP3F = 3.77489497744594108E-8f * 2.0f;
    constexpr float P0sinf = -1.6666654611E-1f, P1sinf = 8.3321608736E-3f, P2sinf = -1.9515295891E-4f;
    constexpr float P0cosf = 4.166664568298827E-2f, P1cosf = -1.388731625493765E-3f, P2cosf = 2.443315711809948E-5f;
    constexpr float TWO_OVER_PI = 2.0f / 3.14159274101257324f;
    constexpr float MAGIC = 12582912.0f;
    float t = self * TWO_OVER_PI;
    tmax = __builtin_fmaxf(tmax, __builtin_fabsf(t));
    float ym = t + MAGIC;
    float y = ym - MAGIC;
    uint32_t b = f2u(ym);
    float x = __builtin_fmaf(y, -DP1F, self);
    x = __builtin_fmaf(y, -DP2F, x);
    x = x - y * DP3F;
    float x2 = x * x;
    float x4 = x2 * x2;
    float s = (x4 * P2sinf + (x2 * P1sinf + P0sinf)) * (x * x2) + x;
    float c = (x4 * P2cosf + (x2 * P1cosf + P0cosf)) * x4 + __builtin_fmaf(x2, -0.5f, 1.0f);
    uint32_t m = (uint32_t)((int32_t)(b << 31) >> 31);
    uint32_t r = (f2u(c) & m) | (f2u(s) & ~m);
    return u2f(r ^ ((b << 30) & 0x80000000u));
}

// ---- tolerance mode (fdsp_set_option("math", FDSP_MATH_FAST)): a sine for Sine::process that is NOT wide's algorithm --
// Same argument x = fl(phase * TAU) as the reference (so the deviation does not compound with the argument rounding),
// then: half-period reduction r = x - rne(x/pi)*pi (two-constant Cody-Waite in FMAs), ONE odd degree-9 polynomial on
// [-pi/2, pi/2] (minimax, |error| < 5e-9 before rounding) in Horner form with FMAs, sign by parity of the period index
// folded into r (sin is odd).  13 VALU operations against wide's 28; |fast_sin(x) - wide_sin(x)| <= 1.2e-7 for phases
// within 64 turns, 3e-7 within 3000 (tests/host/check_fast_sin.hip); valid for |x/pi| < 2^22.  The phase recurrence is untouched.
FD_HD v2f fast_sin2(v2f x) {
    constexpr float INV_PI = 0.318309886183790671538f, PI_HI = 3.14159274101257324f, PI_LO = -8.74227765734758577e-8f;
    constexpr float C0 = -0.16666656732559204f, C1 = 0.008333017118275166f, C2 = -0.00019806601630989462f,
                    C3 = 2.600024345156271e-06f;
    constexpr float MAGIC = 12582912.0f;
    v2f ym = __builtin_elementwise_fma(x, splat2(INV_PI), splat2(MAGIC));
    v2f y = ym - MAGIC;
    v2f r = __builtin_elementwise_fma(y, splat2(-PI_HI), x);
    r = __builtin_elementwise_fma(y, splat2(-PI_LO), r);
    r = v2f{u2f(f2u(r.x) ^ (f2u(ym.x) << 31)), u2f(f2u(r.y) ^ (f2u(ym.y) << 31))};
    v2f z = r * r;
    v2f q = __builtin_elementwise_fma(splat2(C3), z, splat2(C2));
    q = __builtin_elementwise_fma(q, z, splat2(C1));
    q = __builtin_elementwise_fma(q, z, splat2(C0));
    return __builtin_elementwise_fma(q, r * z, r);
}
FD_HD float fast_sin1(float x) {
    constexpr float INV_PI = 0.318309886183790671538f, PI_HI = 3.14159274101257324f, PI_LO = -8.74227765734758577e-8f;
    constexpr float C0 = -0.16666656732559204f, C1 = 0.008333017118275166f, C2 = -0.00019806601630989462f,
                    C3 = 2.600024345156271e-06f;
    constexpr float MAGIC = 12582912.0f;
    float ym = __builtin_fmaf(x, INV_PI, MAGIC);
    float y = ym - MAGIC;
    float r = __builtin_fmaf(y, -PI_HI, x);
    r = __builtin_fmaf(y, -PI_LO, r);
    r = u2f(f2u(r) ^ (f2u(ym) << 31));
    float z = r * r;
    float q = __builtin_fmaf(C3, z, C2);
    q = __builtin_fmaf(q, z, C1);
    q = __builtin_fmaf(q, z, C0);
    return __builtin_fmaf(q, r * z, r);
}

// Tolerance-mode tanh (FDSP_MATH_FAST, Moog): 1 - 2 / (e^(2x) + 1) on the hardware exp2 / reciprocal (v_exp_f32,
// v_rcp_f32; 1 ulp each) for |x| >= 0.25, the odd Taylor polynomial to x^9 below (the exponential form cancels there:
// its ABSOLUTE error of ~1e-7 is a relative 1e-4 at |x| = 1e-3, and a resonating ladder carries a relative error of its
// quiet start into the phase of its loud steady state).  |error| <= 2.3e-7 absolute and <= 6.3e-7 relative over ALL finite
// f32, measured on the device (tests/host/check_tanh_device.hip); +-1 at the infinities, NaN stays NaN.  Both forms are evaluated and one selected: ~8 dependent instructions
// where musl's tanhf is ~150, which is what the one-sample feedback loop of the ladder waits for.
FD_HD float fast_tanh1(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    float e = __builtin_amdgcn_exp2f(x * 2.88539008177792681f);  // 2 log2(e)
    float r = __builtin_amdgcn_rcpf(e + 1.0f);
#else
    float e = __builtin_exp2f(x * 2.88539008177792681f);
    float r = 1.0f / (e + 1.0f);
#endif
    const float big = __builtin_fmaf(-2.0f, r, 1.0f);
    const float z = x * x;
    float q = __builtin_fmaf(0.0218694885361552f, z, -0.053968253968254f);  // 62/2835, -17/315
    q = __builtin_fmaf(q, z, 0.133333333333333f);                            // 2/15
    q = __builtin_fmaf(q, z, -0.333333333333333f);                           // -1/3
    const float small = __builtin_fmaf(x * z, q, x);
    return __builtin_fabsf(x) < 0.25f ? small : big;
}

// musl scalbnf / powf as of the 2018 port (FreeBSD e_powf.c; libm 0.2.15 scalbnf.rs, powf.rs), used by Dsf.
FD_HD float scalbnf_musl(float x, int n) {
    float y = x; /* musl scalbnf.c (libm 0.2 scalbnf.rs): two-step scaling, no double rounding into the subnormals */
    if (n > 127) {
        y *= 0x1p127f;
        n -= 127;
        if (n > 127) {
            y *= 0x1p127f;
            n -= 127;
            if (n > 127) n = 127;
        }
    } else if (n < -126) {
        y *= 0x1p-126f * 0x1p24f;
        n += 126 - 24;
        if (n < -126) {
            y *= 0x1p-126f * 0x1p24f;
            n += 126 - 24;
            if (n < -126) n = -126;
        }
    }
    return y * u2f((uint32_t)(0x7f + n) << 23);
}
FD_HD float powf_musl(float x, float y) {
    const float bp[2] = {1.0f, 1.5f}, dp_h[2] = {0.0f, 5.84960938e-01f}, dp_l[2] = {0.0f, 1.56322085e-06f};
    const float two24 = 16777216.0f, huge = 1.0e30f, tiny = 1.0e-30f;
    const float L1 = 6.0000002384e-01f, L2 = 4.2857143283e-01f, L3 = 3.3333334327e-01f, L4 = 2.7272811532e-01f,
                L5 = 2.3066075146e-01f, L6 = 2.0697501302e-01f;
    const float P1 = 1.6666667163e-01f, P2 = -2.7777778450e-03f, P3 = 6.6137559770e-05f, P4 = -1.6533901999e-06f,
                P5 = 4.1381369442e-08f;
    const float lg2 = 6.9314718246e-01f, lg2_h = 6.93145752e-01f, lg2_l = 1.42860654e-06f, ovt = 4.2995665694e-08f;
    const float cp = 9.6179670095e-01f, cp_h = 9.6191406250e-01f, cp_l = -1.1736857402e-04f;
    const float ivln2 = 1.4426950216e+00f, ivln2_h = 1.4426879883e+00f, ivln2_l = 7.0526075433e-06f;
    float z, ax, z_h, z_l, p_h, p_l, y1, t1, t2, r, s, sn, t, u, v, w;
    int32_t i, j, k, yisint, n, hx, hy, ix, iy, is;
    hx = (int32_t)f2u(x);
    hy = (int32_t)f2u(y);
    ix = hx & 0x7fffffff;
    iy = hy & 0x7fffffff;
    if (iy == 0) return 1.0f;                              /* x**0 = 1, even if x is NaN */
    if (hx == 0x3f800000) return 1.0f;                     /* 1**y = 1, even if y is NaN */
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;  /* NaN if either arg is NaN */
    yisint = 0;                                            /* is y an odd / even integer (only matters for x < 0) */
    if (hx < 0) {
        if (iy >= 0x4b800000) yisint = 2;
        else if (iy >= 0x3f800000) {
            k = (iy >> 23) - 0x7f;
            j = iy >> (23 - k);
            if ((j << (23 - k)) == iy) yisint = 2 - (j & 1);
        }
    }
    if (iy == 0x7f800000) { /* y is +-inf */
        if (ix == 0x3f800000) return 1.0f;
        else if (ix > 0x3f800000) return hy >= 0 ? y : 0.0f;
        else return hy >= 0 ? 0.0f : -y;
    }
    if (iy == 0x3f800000) return hy >= 0 ? x : 1.0f / x; /* y is +-1 */
    if (hy == 0x40000000) return x * x;                   /* y is 2 */
    if (hy == 0x3f000000) {                               /* y is 0.5 */
        if (hx >= 0) return __builtin_sqrtf(x);
    }
    ax = __builtin_fabsf(x);
    if (ix == 0x7f800000 || ix == 0 || ix == 0x3f800000) { /* x is +-0, +-inf, +-1 */
        z = ax;
        if (hy < 0) z = 1.0f / z;
        if (hx < 0) {
            if (((ix - 0x3f800000) | yisint) == 0) z = (z - z) / (z - z);
            else if (yisint == 1) z = -z;
        }
        return z;
    }
    sn = 1.0f; /* sign of the result */
    if (hx < 0) {
        if (yisint == 0) return (x - x) / (x - x);
        if (yisint == 1) sn = -1.0f;
    }
    if (iy > 0x4d000000) { /* |y| > 2**27 */
        if (ix < 0x3f7ffff8) return hy < 0 ? sn * huge * huge : sn * tiny * tiny;
        if (ix > 0x3f800007) return hy > 0 ? sn * huge * huge : sn * tiny * tiny;
        t = ax - 1;
        w = (t * t) * (0.5f - t * (0.333333333333f - t * 0.25f));
        u = ivln2_h * t;
        v = t * ivln2_l - w * ivln2;
        t1 = u + v;
        is = (int32_t)f2u(t1);
        t1 = u2f((uint32_t)is & 0xfffff000u);
        t2 = v - (t1 - u);
    } else {
        float s2, s_h, s_l, t_h, t_l;
        n = 0;
        if (ix < 0x00800000) { /* subnormal x */
            ax *= two24;
            n -= 24;
            ix = (int32_t)f2u(ax);
        }
        n += ((ix) >> 23) - 0x7f;
        j = ix & 0x007fffff;
        ix = j | 0x3f800000; /* normalize ix */
        if (j <= 0x1cc471) k = 0;      /* |x| < sqrt(3/2) */
        else if (j < 0x5db3d7) k = 1;  /* |x| < sqrt(3)   */
        else {
            k = 0;
            n += 1;
            ix -= 0x00800000;
        }
        ax = u2f((uint32_t)ix);
        u = ax - bp[k]; /* s = s_h + s_l = (x-1)/(x+1) or (x-1.5)/(x+1.5) */
        v = 1.0f / (ax + bp[k]);
        s = u * v;
        s_h = s;
        is = (int32_t)f2u(s_h);
        s_h = u2f((uint32_t)is & 0xfffff000u);
        is = (int32_t)((((uint32_t)ix >> 1) & 0xfffff000u) | 0x20000000u); /* t_h = ax + bp[k], high part */
        t_h = u2f((uint32_t)(is + 0x00400000 + (k << 21)));
        t_l = ax - (t_h - bp[k]);
        s_l = v * ((u - s_h * t_h) - s_h * t_l);
        s2 = s * s; /* log(ax) */
        r = s2 * s2 * (L1 + s2 * (L2 + s2 * (L3 + s2 * (L4 + s2 * (L5 + s2 * L6)))));
        r += s_l * (s_h + s);
        s2 = s_h * s_h;
        t_h = 3.0f + s2 + r;
        is = (int32_t)f2u(t_h);
        t_h = u2f((uint32_t)is & 0xfffff000u);
        t_l = r - ((t_h - 3.0f) - s2);
        u = s_h * t_h; /* u + v = s * (1 + ...) */
        v = s_l * t_h + t_l * s;
        p_h = u + v; /* 2/(3 log2) * (s + ...) */
        is = (int32_t)f2u(p_h);
        p_h = u2f((uint32_t)is & 0xfffff000u);
        p_l = v - (p_h - u);
        z_h = cp_h * p_h; /* cp_h + cp_l = 2/(3 log2) */
        z_l = cp_l * p_h + p_l * cp + dp_l[k];
        t = (float)n; /* log2(ax) = (s + ..) * 2/(3 log2) = n + dp_h + z_h + z_l */
        t1 = (((z_h + z_l) + dp_h[k]) + t);
        is = (int32_t)f2u(t1);
        t1 = u2f((uint32_t)is & 0xfffff000u);
        t2 = z_l - (((t1 - t) - dp_h[k]) - z_h);
    }
    is = (int32_t)f2u(y); /* split y into y1 + y2 and compute (y1 + y2) * (t1 + t2) */
    y1 = u2f((uint32_t)is & 0xfffff000u);
    p_l = (y - y1) * t1 + y * t2;
    p_h = y1 * t1;
    z = p_l + p_h;
    j = (int32_t)f2u(z);
    if (j > 0x43000000) return sn * huge * huge; /* z > 128: overflow */
    else if (j == 0x43000000) {                  /* z == 128 */
        if (p_l + ovt > z - p_h) return sn * huge * huge;
    } else if ((j & 0x7fffffff) > 0x43160000) return sn * tiny * tiny; /* z < -150: underflow */
    else if ((uint32_t)j == 0xc3160000u) {                              /* z == -150 */
        if (p_l <= z - p_h) return sn * tiny * tiny;
    }
    i = j & 0x7fffffff; /* 2**(p_h + p_l) */
    k = (i >> 23) - 0x7f;
    n = 0;
    if (i > 0x3f000000) { /* |z| > 0.5: n = [z + 0.5] */
        n = j + (0x00800000 >> (k + 1));
        k = ((n & 0x7fffffff) >> 23) - 0x7f; /* new k for n */
        t = u2f((uint32_t)(n & ~(0x007fffff >> k)));
        n = ((n & 0x007fffff) | 0x00800000) >> (23 - k);
        if (j < 0) n = -n;
        p_h -= t;
    }
    t = p_l + p_h;
    is = (int32_t)f2u(t);
    t = u2f((uint32_t)is & 0xffff8000u);
    u = t * lg2_h;
    v = (p_l - (t - p_h)) * lg2 + t * lg2_l;
    z = u + v;
    w = v - (z - u);
    t = z * z;
    t1 = z - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    r = (z * t1) / (t1 - 2.0f) - (w + z * w);
    z = 1.0f - (r - z);
    j = (int32_t)f2u(z);
    j += (int32_t)((uint32_t)n << 23);
    if ((j >> 23) <= 0) z = scalbnf_musl(z, n); /* subnormal output */
    else z = u2f((uint32_t)j);
    return sn * z;
}

// follow.rs:12-24 (f64).  log / exp are the device library's double routines; the reference's are libm 0.2.15's.  Both
// are accurate to < 1 ulp of f64 and the result is rounded to f32, so the f32 coefficient agrees except when the f64
// value lies within ~1e-16 relative of an f32 rounding boundary (same policy as the oracle: SURVEY 8c).
extern "C" __device__ double __ocml_log_f64(double);
extern "C" __device__ double __ocml_exp_f64(double);
extern "C" __device__ double __ocml_pow_f64(double, double);
FD_HD double log_f64(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ocml_log_f64(x);
#else
    return __builtin_log(x);
#endif
}
FD_HD double exp_f64(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ocml_exp_f64(x);
#else
    return __builtin_exp(x);
#endif
}
FD_HD double pow_f64(double x, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ocml_pow_f64(x, y);
#else
    return __builtin_pow(x, y);
#endif
}
FD_HD double halfway_coeff(double samples) {
    double r0 = log_f64(samples > 1.0 ? samples : 1.0) - 0.861624594696583;
    double r1 = 1.0 / (1.0 + exp_f64(0.0 - r0));
    double r2 = r1 * 1.13228543863477 - 0.1322853859;
    return 1.0 - (r2 < 0.9999999 ? r2 : 0.9999999);
}

// ---- integer hashing (bit-exact) -------------------------------------------------------------------------
FD_HD double rnd1(uint64_t x) {  // math.rs:569-576
    x = x ^ 0x5555555555555555ULL;
    x = x * 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    x = x ^ (x >> 31);
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}
FD_HD uint64_t hash1(uint64_t x) {  // math.rs:592-599
    x = x ^ 0x5555555555555555ULL;
    x = x * 0x517cc1b727220a95ULL;
    x = (x ^ (x >> 32)) * 0xd6e8feb86659fd93ULL;
    x = (x ^ (x >> 32)) * 0xd6e8feb86659fd93ULL;
    return x ^ (x >> 32);
}
FD_HD uint64_t atto(uint64_t state, uint64_t data) {  // AttoHash::hash math.rs:649-658
    uint64_t r = (state << 5) | (state >> 59);
    return (r ^ data) * 0x517cc1b727220a95ULL;
}
FD_HD uint32_t hash32x(uint32_t x) {  // noise.rs:154-158
    constexpr uint32_t MUL_X = 0x45d9f3b;
    x = (x ^ (x >> 16)) * MUL_X;
    x = (x ^ (x >> 16)) * MUL_X;
    return (x ^ (x >> 16)) * MUL_X;
}

}  // namespace fd
