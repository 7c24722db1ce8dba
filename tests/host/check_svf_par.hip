// tests/host/check_svf_par.hip -- host-side check (hipcc, host only) of the time-parallel SVF arithmetic of k_render_ts3p: the header
// the kernel compiles (fd_svf_par.hpp: tables in f64, chunk pass from state zero, fix-up) against the serial f32 tick (SvfCore::tick, what
// every other kernel computes), both measured against the same tick in f64.
//   usage: check_svf_par [R]      R: the per-voice bound of (b) below, default 4
// Banks of 16 x 16 voices: cutoff 20 Hz .. 0.45 sr, q 0.1 .. 50, log-spaced; all nine modes; white noise at 0.5 rms and an FM sine of
// peak 3.5 as inputs; 9 600 frames at 48 kHz, rendered as launches of whole blocks with the state carried (tables rebuilt per launch).
//   (a) per input, over the bank of all nine modes x 256 voices: worst error of the chunked form <= worst error of the serial form
//       (the per-mode figures are printed: where the output is the input plus a correction -- notch, allpass, bell -- both forms sit at
//       an ulp or two of the output and the chunked one, which adds two rounded terms of its own, can be the worse by a tenth)
//   (b) per voice: err_par <= R * err_ser + 2^-23 * peak          (prints the worst err_par / err_ser it meets)
//   (c) 320 frames from a carried state == 64 + 128 + 128 frames, bit for bit, end state included
//   (d) an inf / a NaN in the input at a chosen frame: isfinite(parallel) == isfinite(serial) frame for frame
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define FD_HOST_ONLY 1
#include "fd_nodes.hpp"
#include "fd_svf_par.hpp"
using namespace fd;

#ifndef FD_TSP_K
#define FD_TSP_K 2  // as shipped (fd_tsp.hpp)
#endif
constexpr int LC = 64 / FD_TSP_K;

// one launch of T frames (whole blocks) the way the kernel runs it: tables from the coefficients, the state carried block to block
static void launch_par(const SvfpCoefs& k, const float* in, float* out, size_t T, float& s1, float& s2) {
    SvfpTables<LC> t;
    svfp_tables<LC>(k, t);
    for (size_t t0 = 0; t0 < T; t0 += 64) svfp_block<LC>(k, t, in + t0, out + t0, s1, s2);
}

int main(int argc, char** argv) {
    const double R = argc > 1 ? atof(argv[1]) : 4.0;
    const int NV = 256, T = 9600;
    const float sr = 48000.0f;
    uint64_t st = 11;
    auto rnd = [&]() { st = st * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(st >> 32); };
    auto uni = [&]() { return ((double)(rnd() >> 8) + 0.5) * (1.0 / 16777216.0); };
    // inputs, shared by the voices of a bank: gaussian noise at 0.5 rms | sin(carrier phase + modulator), peak 3.5
    std::vector<float> noise(T), fm(T);
    for (int i = 0; i < T; i++) noise[i] = (float)(0.5 * sqrt(-2.0 * log(uni())) * cos(6.283185307179586 * uni()));
    for (int i = 0; i < T; i++) fm[i] = (float)(3.5 * sin(6.283185307179586 * 220.0 * i / sr + 4.0 * sin(6.283185307179586 * 330.0 * i / sr)));
    int bad = 0;
    double worst_ratio = 0.0, all_par = 0.0, all_ser = 0.0;
    std::vector<float> yp(T), ys(T);
    for (int which = 0; which < 2; which++) {
        const std::vector<float>& x = which ? fm : noise;
        double in_par = 0.0, in_ser = 0.0;
        for (int mode = 0; mode < 9; mode++) {
            double bank_par = 0.0, bank_ser = 0.0, bank_ratio = 0.0;
            int worse = 0;
            for (int v = 0; v < NV; v++) {
                const float fc = (float)(20.0 * pow(0.45 * sr / 20.0, (v % 16) / 15.0)), q = (float)(0.1 * pow(500.0, (v / 16) / 15.0));
                const SvfCoefs c = svf_coefs(mode, sr, fc, q, 2.0f);
                const SvfpCoefs k{c.a1, c.a2, c.a3, c.m0, c.m1, c.m2};
                SvfCore core{};
                core.set(c);
                float s1 = 0.0f, s2 = 0.0f;
                launch_par(k, x.data(), yp.data(), T, s1, s2);
                double d1 = 0.0, d2 = 0.0, err_par = 0.0, err_ser = 0.0, peak = 0.0;
                for (int i = 0; i < T; i++) {
                    ys[i] = core.tick(x[i]);
                    const double y = svfp_tick<double>(k.a1, k.a2, k.a3, k.m0, k.m1, k.m2, d1, d2, (double)x[i]);
                    err_par = fmax(err_par, fabs((double)yp[i] - y));
                    err_ser = fmax(err_ser, fabs((double)ys[i] - y));
                    peak = fmax(peak, fabs(y));
                }
                bank_par = fmax(bank_par, err_par);
                bank_ser = fmax(bank_ser, err_ser);
                if (err_par > err_ser) worse++;
                if (err_ser > 0.0) bank_ratio = fmax(bank_ratio, err_par / err_ser);
                if (!(err_par <= R * err_ser + ldexp(peak, -23))) {
                    bad++;
                    printf("(b) FAILED mode %d input %d voice %d (fc %.1f q %.3f): err_par %.3e err_ser %.3e peak %.3e\n", mode, which, v, fc, q, err_par, err_ser, peak);
                }
            }
            printf("mode %d input %s: worst error chunked %.3e serial %.3e; chunked worse in %d of %d voices, by at most %.3f x\n", mode,
                   which ? "fm" : "noise", bank_par, bank_ser, worse, NV, bank_ratio);
            worst_ratio = fmax(worst_ratio, bank_ratio);
            in_par = fmax(in_par, bank_par);
            in_ser = fmax(in_ser, bank_ser);
        }
        printf("input %s, all modes: worst error chunked %.3e serial %.3e\n", which ? "fm" : "noise", in_par, in_ser);
        if (!(in_par <= in_ser)) {
            bad++;
            printf("(a) FAILED input %d\n", which);
        }
        all_par = fmax(all_par, in_par);
        all_ser = fmax(all_ser, in_ser);
    }
    printf("Lc %d: worst error chunked %.3e serial %.3e; worst ratio %.3f (R = %.3f)\n", LC, all_par, all_ser, worst_ratio, R);
    // (c) launch splits
    for (int v = 0; v < NV; v += 5) {
        const SvfCoefs c = svf_coefs(v % 9, sr, (float)(20.0 * pow(0.45 * sr / 20.0, (v % 16) / 15.0)), (float)(0.1 * pow(500.0, (v / 16) / 15.0)), 2.0f);
        const SvfpCoefs k{c.a1, c.a2, c.a3, c.m0, c.m1, c.m2};
        float a1 = 0.25f, a2 = -0.125f, b1 = a1, b2 = a2;
        std::vector<float> one(320), parts(320);
        launch_par(k, noise.data(), one.data(), 320, a1, a2);
        launch_par(k, noise.data(), parts.data(), 64, b1, b2);
        launch_par(k, noise.data() + 64, parts.data() + 64, 128, b1, b2);
        launch_par(k, noise.data() + 192, parts.data() + 192, 128, b1, b2);
        if (memcmp(one.data(), parts.data(), 320 * sizeof(float)) != 0 || f2u(a1) != f2u(b1) || f2u(a2) != f2u(b2)) {
            bad++;
            printf("(c) FAILED voice %d\n", v);
        }
    }
    // (d) non-finite inputs
    for (int trial = 0; trial < 64; trial++) {
        const SvfCoefs c = svf_coefs(trial % 9, sr, 200.0f + 150.0f * trial, 0.5f + 0.1f * trial, 2.0f);
        const SvfpCoefs k{c.a1, c.a2, c.a3, c.m0, c.m1, c.m2};
        std::vector<float> x(noise.begin(), noise.begin() + 256), p(256), s(256);
        const int at = 3 + 7 * trial % 250;
        x[at] = trial & 1 ? NAN : (trial & 2 ? -INFINITY : INFINITY);
        SvfCore core{};
        core.set(c);
        float s1 = 0.0f, s2 = 0.0f;
        launch_par(k, x.data(), p.data(), 256, s1, s2);
        for (int i = 0; i < 256; i++) s[i] = core.tick(x[i]);
        for (int i = 0; i < 256; i++)
            if (std::isfinite(p[i]) != std::isfinite(s[i])) {
                bad++;
                printf("(d) FAILED trial %d frame %d (non-finite input at %d): parallel %g serial %g\n", trial, i, at, p[i], s[i]);
                break;
            }
        if (std::isfinite(s1) != std::isfinite(core.ic1eq) || std::isfinite(s2) != std::isfinite(core.ic2eq)) {
            bad++;
            printf("(d) FAILED trial %d: end state\n", trial);
        }
    }
    printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
