// fd_reverb3_const.hpp -- rv3_make_const, the host half of reverb3_stereo's kernel (fd_reverb3.hpp): the read distances, the ring capacity and
// the filter coefficients at a sample rate.  Host code only, kept apart from the kernels so that a host program can compile it without them
// (tests/host/check_reverb3_const.hip).  It DEFINES a non-inline function: fd_reverb3.hip is the one translation unit of the library that
// includes it, after fd_reverb3.hpp, fd_math.hpp and fd_nodes.hpp.
#pragma once

#include <algorithm>
#include <cmath>

namespace fd {

static const int RV3_LDELAYS[32] = {401, 421, 443, 463, 487, 503, 523, 547, 563, 587, 607, 619, 643, 661, 683, 701,   // reverb.rs:163-166
                                    727, 743, 761, 787, 809, 823, 839, 863, 883, 907, 929, 947, 967, 983, 1009, 1021};
static const int RV3_RDELAYS[32] = {419, 433, 457, 479, 491, 509, 541, 557, 577, 593, 613, 631, 653, 673, 691, 719,   // :167-170
                                    733, 757, 773, 797, 811, 829, 853, 877, 887, 911, 937, 953, 977, 997, 1013, 1033};
static const int RV3_BDELAYS[8] = {1087, 1091, 1093, 1097, 1103, 1109, 1117, 1123};                                   // :171
static const int RV3_PDELAYS[4] = {245, 367, 263, 349};                                                                // :198

bool rv3_make_const(double time, double diffusion, const Rv3Filter& filter, double sample_rate, Rv3Const* c) {
    *c = Rv3Const{};
    // Delay::new(t) at DEFAULT_SR, then set_sample_rate: time_in_samples = round(t * sample_rate) (delay.rs:105-112)
    auto samples = [&](int at_default) { return (int)std::round(((double)at_default / 44100.0) * sample_rate); };
    int longest = 0, shortest = 1 << 30;
    for (int i = 0; i < 4; i++) c->dpre[i] = RV3_PDELAYS[i];  // (n - 1) samples + the allpass's own tick; never re-sized (reverb.rs:226-238)
    for (int b = 0; b < 8; b++) {
        for (int j = 0; j < 4; j++) {
            c->dap0[b][j] = samples(RV3_LDELAYS[b + j * 8] - 1) + 1;   // :175-186
            c->dap1[b][j] = samples(RV3_RDELAYS[b + j * 8] - 1) + 1;
            longest = std::max(longest, std::max(c->dap0[b][j], c->dap1[b][j]));
            shortest = std::min(shortest, std::min(c->dap0[b][j], c->dap1[b][j]));
        }
        c->dblk[b] = samples(RV3_BDELAYS[7 - b]) + (b == 0 ? 1 : 0);    // :187
        longest = std::max(longest, c->dblk[b]);
        shortest = std::min(shortest, c->dblk[b]);
    }
    if (shortest <= 128 || longest > (1 << 20)) return false;
    int cap = 256;
    while (cap < longest + 64) cap <<= 1;
    c->cap = cap;
    c->ring_stride = (size_t)72 * ((size_t)cap + 64);
    // lerp(0.5, 0.9, diffusion) as f32 (:173; Lerp: a * (1 - t) + b * t in f64, math.rs:169-178)
    c->eta = (float)(0.5 * (1.0 - diffusion) + 0.9 * diffusion);
    // pow(db_amp(-60.0), 0.035 / time) as f32 (:196); db_amp(x) = exp((x / 20) * LN_10) (math.rs:76-78, 294)
    c->a = (float)std::pow(std::exp((-60.0 / 20.0) * 2.302585092994046), 0.035 / time);
    const float sr = (float)sample_rate;
    c->fkind = filter.kind;
    if (filter.kind == 0) {
        c->c = expf_musl(-F32_TAU * filter.cutoff / sr);   // Lowpole::set_cutoff, F = f32 (filter.rs:35-38)
        c->omc = 1.0f - c->c;
    } else {
        const SvfCoefs k = svf_coefs(filter.mode, sr, filter.cutoff, filter.q, filter.gain);   // FixedSvf::set_sample_rate -> update (svf.rs:989-992, 236-239)
        c->sa1 = k.a1; c->sa2 = k.a2; c->sa3 = k.a3; c->sm0 = k.m0; c->sm1 = k.m1; c->sm2 = k.m2;
    }
    return true;
}

}  // namespace fd
