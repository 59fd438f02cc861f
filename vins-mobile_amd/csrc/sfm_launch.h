// sfm_launch.h — the device launch of the batched bundle adjustment (vio_sfm.hip), for the units that run it as one stage
// of a longer call (vio_init_sfm.hip): the kernels stay in the unit that is built with the solver's flags.
#pragma once
#include <hip/hip_runtime.h>

#include "sfm_core.h"

namespace vio {
namespace sfm {

// large: the layout of more than kSmallFrames frames (B.hcc and B.slab set); in_lds: the landmark state in LDS (small layout,
// points_fit_lds). The caller owns every buffer of B. VIO_OK / VIO_ENODEV.
int prepare_ba(const Batch &B, bool large, bool in_lds);  // the kernel's dynamic LDS limit for this batch: before launch_ba
int launch_ba(const Batch &B, bool large, bool in_lds, hipStream_t st);  // one workgroup per problem of B on stream st

}  // namespace sfm
}  // namespace vio
