// fd_kinds_fm_tsp.hpp -- which of the config-1 / config-3 graph types have the time-split kernel with the time-parallel filter stage
// (fd_tsp.hpp k_render_ts3p, "svf_exec" = FDSP_SVF_PARALLEL): the tolerance-mode twins only -- the kernel's arithmetic is not the
// reference's, so a bank in exact mode never reaches it.  fd_kinds_fm.hip (the kinds) reads this, fd_kinds_fm_tsp.hip holds the kernels.
#pragma once

#include "fd_kinds_fm.hpp"

namespace fd {
using SineHzLowpassFast = FastOf<SineHzLowpass>::type;
using FmSvfFast = FastOf<FmSvf>::type;
template <> struct TspKernel<SineHzLowpassFast> { static constexpr bool ok = true; };
template <> struct TspKernel<FmSvfFast> { static constexpr bool ok = true; };
}  // namespace fd
