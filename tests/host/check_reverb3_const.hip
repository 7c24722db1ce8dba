// tests/host/check_reverb3_const.hip -- what rv3_make_const (fd_reverb3_const.hpp) decides at each sample rate given on the command line:
// accept / refuse, the 72 read distances, the ring capacity and the ring stride.  Host code only: nothing is launched and no device is needed.
// tests/test_reverb3_cases.py compares every entry with the Python restatement in tests/reverb3_cases.py.
//
//   rate <hz> ok <0|1> cap <slots> stride <floats>
//   dap0 <32 distances, [block][j]>
//   dap1 <32 distances>
//   dblk <8 distances>
#include <cstdio>
#include <cstdlib>

#include "fd_reverb3.hpp"
#include "fd_math.hpp"
#include "fd_nodes.hpp"
#include "fd_reverb3_const.hpp"

int main(int argc, char** argv) {
    fd::Rv3Filter flt;   // lowpole_hz(1800): the filter has no part in the distances
    flt.cutoff = 1800.0f;
    for (int i = 1; i < argc; i++) {
        const double sr = std::strtod(argv[i], nullptr);
        fd::Rv3Const c;
        const bool ok = fd::rv3_make_const(2.0, 0.6, flt, sr, &c);
        std::printf("rate %.17g ok %d cap %d stride %zu\n", sr, ok ? 1 : 0, c.cap, c.ring_stride);
        std::printf("dap0");
        for (int b = 0; b < 8; b++)
            for (int j = 0; j < 4; j++) std::printf(" %d", c.dap0[b][j]);
        std::printf("\ndap1");
        for (int b = 0; b < 8; b++)
            for (int j = 0; j < 4; j++) std::printf(" %d", c.dap1[b][j]);
        std::printf("\ndblk");
        for (int b = 0; b < 8; b++) std::printf(" %d", c.dblk[b]);
        std::printf("\n");
    }
    return 0;
}
