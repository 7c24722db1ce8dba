// fd_kinds_fm_tsp.hip -- the time-split kernels with the time-parallel filter stage (fd_tsp.hpp k_render_ts3p) of the tolerance-mode
// config-1 / config-3 graph types, and their launchers; fd_kinds_fm.hip calls launch_tsp<G> through its declaration in fd_engine.hpp.
// A translation unit of its own: fd_kinds_fm_ts.o (k_render_ts3, exact bits) is not rebuilt differently because this kernel exists, and
// like that unit it is built with -amdgpu-sched-strategy=max-ilp (iterative-ilp crashes clang on the ts_stage loops; Makefile).
#include "fd_kinds_fm_tsp.hpp"
#include "fd_tsp.hpp"

namespace fd {
static_assert(TspPlan<SineHzLowpassFast>::ok && TspPlan<FmSvfFast>::ok && !TspPlan<Pipe<Noise, Biquad>>::ok && !TspPlan<Pipe<Sine, FixedSvf>>::ok,
              "TspPlan: two oscillator stages and one FixedSvf");
template void launch_tsp<SineHzLowpassFast>(const RenderPlan&, const RenderArgs&);
template void launch_tsp<FmSvfFast>(const RenderPlan&, const RenderArgs&);
}  // namespace fd
