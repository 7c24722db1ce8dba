// C++ host side (include/fundsp_hip.hpp) of scores -- Bank::set_score -- against the oracle's Sequencer, in the style of test_cpp_host.cpp.
//
//   test_cpp_score --host   no device: the argument checks a host can trip without one
//   test_cpp_score --gpu    on an MI355X: a pool of three voices plays four notes of the README's FM patch, one fresh oracle unit per note
//
// Test infrastructure: links oracle/libfundsp_oracle.so (the checker), fundsp_amd/libfundsp_hip.so (the product) and the HIP runtime for
// the device buffer fdsp_bank_process_events writes.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fundsp_hip.hpp"
extern "C" {  // (the header closes its own extern "C" block ahead of the Sequencer's declarations)
#include "fundsp_oracle.h"
}

extern "C" {  // the three HIP runtime calls this test needs (hip_runtime_api.h: hipError_t is an int-sized enum, hipMemcpyDeviceToHost = 2)
int hipMalloc(void** ptr, size_t size);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);
int hipFree(void* ptr);
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

static onode* oracle_fm(float f, float m, float fc, float q) {
    float c = f;
    onode* mod = o_pipe(o_constant(1, &c), o_sine());
    onode* g = o_unop(O_ADD_SCALAR, o_unop(O_MUL_SCALAR, o_unop(O_MUL_SCALAR, mod, f), m), f);
    return o_pipe(o_pipe(g, o_sine()), o_fixed_svf(O_SVF_LOWPASS, fc, q, 1.0f));
}

static void host_checks() {
    // the C entry point refuses what it can see without a device
    EXPECT(fdsp_bank_set_score(nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == FDSP_EINVAL);
    EXPECT(std::string(fdsp_last_error()).find("bank is NULL") != std::string::npos);
}

static void gpu_checks() {
    const double SR = 48000.0;
    const size_t V = 3, T = 64 * 3 + 9;
    const std::vector<uint64_t> seeds = {11, 12, 13};
    Bank b = Bank::from_graph(sine_hz(110.0f) * 110.0f * 2.0f + 110.0f >> sine() >> lowpass_hz(1000.0f, 1.0f), V, 0, SR);
    b.set_seed(seeds);
    // voice 0: two notes, legato, the second inside the first one's last block; voice 1: one note off the sample grid with both fades; voice 2: none
    const std::vector<int> voice = {1, 0, 0, 0};   // (not sorted: the engine sorts)
    const std::vector<double> ev = {20.3 / SR, 150.3 / SR, 30.0 / SR, 40.0 / SR,
                                    70.0 / SR, 90.0 / SR, 0.0, 5.0 / SR,
                                    0.0, 70.0 / SR, 10.0 / SR, 0.0,
                                    100.0 / SR, 400.0 / SR, 0.0, 0.0};
    const int fade[4] = {FDSP_FADE_POWER, FDSP_FADE_SMOOTH, FDSP_FADE_SMOOTH, FDSP_FADE_POWER};
    const float f[4] = {220.0f, 330.0f, 110.0f, 440.0f}, m[4] = {1.0f, 2.0f, 3.0f, 0.5f}, fc[4] = {900.0f, 2000.0f, 500.0f, 4000.0f}, q[4] = {0.7f, 1.0f, 2.0f, 3.0f};
    const std::vector<std::string> names = {"0.0.0.0.0.0:value[0]", "0.0.0.0:scalar", "0.0.0:scalar", "0.0:scalar", "1:cutoff", "1:q"};
    std::vector<float> rows;
    for (int k = 0; k < 4; k++)
        for (float x : {f[k], f[k], m[k], f[k], fc[k], q[k]}) rows.push_back(x);
    EXPECT([&] { try { b.set_score(voice, ev, names, std::vector<float>(5), fade); } catch (const Error& e) { return e.code == FDSP_EINVAL; } return false; }());
    b.set_score(voice, ev, names, rows, fade);
    float* d_out = nullptr;
    EXPECT(hipMalloc((void**)&d_out, V * T * sizeof(float)) == 0);
    b.process_events(T, nullptr, d_out);
    b.synchronize();
    std::vector<float> got(V * T);
    EXPECT(hipMemcpy(got.data(), d_out, got.size() * sizeof(float), 2) == 0);   // [frame][voice]
    hipFree(d_out);
    EXPECT(b.events_time() > 0.0);
    oseq* s = o_seq_new(0, 1, SR);
    for (int k = 0; k < 4; k++) {
        onode* n = oracle_fm(f[k], m[k], fc[k], q[k]);
        o_set_seed(n, seeds[voice[k]]);
        EXPECT(o_seq_push(s, ev[4 * k], ev[4 * k + 1], fade[k], ev[4 * k + 2], ev[4 * k + 3], n) == k);
    }
    std::vector<float> mix(T), per(4 * T);
    o_seq_render(s, T, 1, nullptr, mix.data(), per.data());
    EXPECT(b.events_time() == o_seq_time(s));
    o_seq_free(s);
    size_t sounding = 0;
    for (size_t v = 0; v < V; v++)
        for (size_t t = 0; t < T; t++) {
            float want = 0.0f;
            for (int k = 0; k < 4; k++) {
                uint32_t bits;
                std::memcpy(&bits, &per[k * T + t], 4);
                if ((size_t)voice[k] == v && bits != 0) want = per[k * T + t];
            }
            sounding += want != 0.0f;
            if (std::memcmp(&want, &got[t * V + v], 4) != 0) {
                std::printf("FAIL score voice %zu frame %zu: got %.9g want %.9g\n", v, t, got[t * V + v], want);
                failures++;
                return;
            }
        }
    EXPECT(sounding > 300);
}

int main(int argc, char** argv) {
    const bool gpu = argc > 1 && std::strcmp(argv[1], "--gpu") == 0;
    try {
        host_checks();
        if (gpu) gpu_checks();
    } catch (const std::exception& e) {
        std::printf("FAIL: exception %s\n", e.what());
        return 2;
    }
    std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "host", failures);
    return failures ? 1 : 0;
}
