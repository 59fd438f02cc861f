// vio_window_variants.h -- the instantiations of the window kernel (vio_window_kernel.inc) and how the launcher reaches them. The table
// of variants (kTraits) is host-only and lives with the launcher's plan, wk_plan.h.
// Every (variant, stage clock on / off) pair is a translation unit of its own (vio_wk_unit.hip compiled once per pair, csrc/Makefile):
// the kernel is ~70 k instructions per instantiation and the units build in parallel.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "wk_plan.h"

namespace vio_wk {

struct VariantFns {
  const void *fn;  // the kernel (hipFuncSetAttribute, occupancy queries)
  void (*launch)(int grid, size_t lds_bytes, hipStream_t st, const vio::BatchPtrs &B, const vio::MargPtrs &MP);
};
// (vio_backend.hip) prof: the instantiation with the stage clock compiled in (vio_backend_set_profile)
const VariantFns &variant(int v, bool prof);

}  // namespace vio_wk
