// C++ host side (include/fundsp_hip.hpp) of the feedback delay banks -- Bank::feedback_delay -- against the oracle's generic Feedback graph,
// in the style of test_cpp_host.cpp.
//
//   test_cpp_feedback_delay --host   no device: the argument checks a host can trip without one
//   test_cpp_feedback_delay --gpu    on an MI355X: the ping-pong feedback((delay | delay) >> reverse() * g), block by block
//
// Test infrastructure: links oracle/libfundsp_oracle.so (the checker) and fundsp_amd/libfundsp_hip.so (the product).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fundsp_hip.hpp"
extern "C" {
#include "fundsp_oracle.h"
}

using namespace fundsp_hip;

static int failures = 0;
#define EXPECT(cond)                                                           \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            failures++;                                                        \
        }                                                                      \
    } while (0)

static bool bit_equal(const float* got, const float* want, size_t n, const char* what) {
    for (size_t i = 0; i < n; i++) {
        uint32_t a, b;
        std::memcpy(&a, got + i, 4);
        std::memcpy(&b, want + i, 4);
        if (a != b) {
            std::printf("FAIL %s: sample %zu got %.9g want %.9g\n", what, i, got[i], want[i]);
            failures++;
            return false;
        }
    }
    return true;
}

static void host_checks() {
    fdsp_bank* h = (fdsp_bank*)1;
    EXPECT(fdsp_feedback_delay_create(2, nullptr, 48000.0, &h) == FDSP_EINVAL && h == nullptr);
    EXPECT(std::string(fdsp_last_error()).find("network NULL") != std::string::npos);
    const double d[3] = {0.005, 0.005, 0.005};
    fdsp_feedback_delay net{};
    net.channels = 3;
    net.delays = d;
    bool threw = false;
    try {
        Bank b = Bank::feedback_delay(2, net, 48000.0);
    } catch (const Error& e) {
        threw = std::string(e.what()).find("channels") != std::string::npos;
    }
    EXPECT(threw);
}

static void gpu_checks() {
    const double SR = 48000.0;
    const float t0 = 200.0f / 48000.0f, t1 = 131.0f / 48000.0f, g = 0.5f;
    const double d[2] = {(double)t0, (double)t1};
    fdsp_feedback_delay net{};
    net.channels = 2;
    net.place = FDSP_FDN_IN_LINE;
    net.reverse = 1;
    net.delays = d;
    net.outer_gain = &g;
    Bank b = Bank::feedback_delay(2, net, SR);
    EXPECT(b.inputs() == 2 && b.outputs() == 2);
    onode* n = o_feedback(o_pipe(o_stack(o_delay((double)t0), o_delay((double)t1)), o_unop(O_MUL_SCALAR, o_reverse(2), g)), nullptr, 0);
    o_set_sample_rate(n, SR);
    uint32_t s = 99;
    for (int blk = 0; blk < 16; blk++) {   // 1024 frames: several trips round both lines
        std::vector<float> x(2 * 2 * 64, 0.0f), got(2 * 2 * 64), want(2 * 64);
        if (blk < 6)
            for (int i = 0; i < 128; i++) {
                s = s * 1664525u + 1013904223u;
                x[i] = x[128 + i] = (float)(s >> 8) * (1.0f / 8388608.0f) - 1.0f;
            }
        b.process(64, x.data(), got.data());
        o_process(n, 64, x.data(), want.data());
        if (!bit_equal(got.data(), want.data(), 128, "ping-pong instance 0")) break;
        if (!bit_equal(got.data() + 128, want.data(), 128, "ping-pong instance 1")) break;
        if (blk == 15) {
            float peak = 0.0f;
            for (float v : got) peak = v > peak ? v : (-v > peak ? -v : peak);
            EXPECT(peak > 1e-3f);   // the tail recirculates
        }
    }
    o_free(n);
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "--gpu") == 0;
    try {
        host_checks();
        if (gpu) gpu_checks();
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        failures++;
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
