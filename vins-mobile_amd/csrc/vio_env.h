// vio_env.h -- every environment variable the library reads goes through env_flag / env_int below. Plain C++ (no HIP):
// the host-only translation units include it too. None of the variables is needed in normal use.
#pragma once
#include <stdlib.h>

namespace vio {

//   read once per process, at first use:
//     VIO_AMD_ALLOW_TWO_RUNTIMES=1  create contexts although two HIP runtimes are mapped (vio_device.h)
//     VIO_AMD_HOST_TIMING=1         host-side timings of the back-end and device buffer growth on stderr
//     VIO_AMD_POISON=1              NaN patterns in staging, device scratch and every CU's LDS before each window launch
//     VIO_AMD_STORE_PROF=1          cycle stamps of the resident store kernels' passes
//     VIO_AMD_TU_PROF=1             cycle stamps of track_update_kernel on stderr (synchronizes every step)
//     VIO_AMD_HOST_POOLS=n          number of host pools (vio_pool.h; default 2 on hosts with >= 128 CPUs, else 1; at most 4)
//     VIO_AMD_HOST_NUMA=0           leave the pools' workers unbound on a multi-socket host
//     VIO_AMD_HOST_THREADS=n        workers per host pool (default from the usable CPUs, the CPU quota and the ranks below)
//     LOCAL_WORLD_SIZE, OMPI_COMM_WORLD_LOCAL_SIZE, MV2_COMM_WORLD_LOCAL_SIZE   ranks on this node, the first that is set
//   read at create:
//     VIO_AMD_DETECT_ALWAYS=1       front-end: run corner detection also for sequences that need no new corner
//     VIO_AMD_REDO_REPORT=1         front-end: destroy prints how many sequence-frames the detector redid from a full-size list
//     VIO_AMD_CS_PROF=1             front-end: cycle stamps of corner_select_kernel on stderr (synchronizes every publish step)
//     VIO_AMD_HOST_PRIORS=1         estimator: marginalization priors travel through host memory
//     VIO_AMD_RESIDENT=0            estimator: no device-resident landmark store
//     VIO_AMD_RESIDENT_IMU=1        estimator: the device integrates the IMU samples of resident sequences
//   read at every back-end upload:
//     VIO_AMD_PROF_TID=n            work-item that keeps the window kernel's stage clock (default 0)
//     VIO_AMD_WAVE_ROT=n            force the window kernel's wave-role rotation (default -1: from the hardware wave slot)
//   read at every launch or front-end step (tests change them within one process):
//     VIO_AMD_COOP=1|2|4            width of cooperative windows (1: off), within what the device holds
//     VIO_AMD_COOP_SPIN=n           spin limit of a cooperative window's waits (test hook of the timeout path)
//     VIO_AMD_COOP_FAULT=1          helper workgroups of a cooperative window leave at once (test hook of the timeout path)
//     VIO_AMD_COPY_LEVEL0=1         copy resident frames into pyramid level 0 instead of reading them where they lie
// env_flag: set and its first character is `on` ('1' for every flag above; RESIDENT and HOST_NUMA test for '0').
inline bool env_flag(const char *name, char on = '1') {
  const char *v = getenv(name);
  return v && v[0] == on;
}
// env_int: atoi of the value when set, else `fallback`.
inline int env_int(const char *name, int fallback) {
  const char *v = getenv(name);
  return v ? atoi(v) : fallback;
}
inline bool host_timing() {
  static const bool on = env_flag("VIO_AMD_HOST_TIMING");
  return on;
}

}  // namespace vio
