// vio_posegraph_launch.h — the launch of posegraph_kernel (vio_posegraph.hip) for callers inside the library that already
// hold the solver's input arrays on the device: vio_posegraph_optimize fills them from host graphs, the keyframe database
// (vio_keyframe_db.hip) writes them with kfdb_build and never leaves the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace vio {

constexpr int kPgThreads = 512;
constexpr int kPgHdr = 4;  // n_nodes, n_edges, N, max_iterations

struct PgPtrs {
  int ld;          // leading dimension of the dense matrices = 4 * max_nodes rounded up to 16
  int node_cap, edge_cap;
  const int *hdr;           // [g][kPgHdr]
  const int *col;           // [g][node_cap]: node -> first of its 4 unknowns, -1 constant / not in the program
  const double *node0;      // [g][node_cap][4]: yaw, t of every node as given
  const int *edge_i, *edge_j, *edge_kind;  // [g][edge_cap]
  const double *meas;       // [g][edge_cap][6]
  double *H, *A;            // [g][ld * ld]; zero beyond what the kernel writes (whole 16 x 16 tiles are read)
  double *xout;             // [g][ld]
  double *stats_d;          // [g][kStatsDoubles]
  int *stats_i;             // [g][kStatsInts]
};

inline int pg_ld(int max_nodes) { return (4 * max_nodes + 15) / 16 * 16; }
// dynamic LDS of one workgroup: seven N-vectors, the reduction scratch, the tile envelope
inline size_t pg_lds_bytes(int ld) {
  return ((size_t)7 * ld + 6 * (kPgThreads / 64) + 2) * sizeof(double) + ((size_t)2 * (ld / 16) + 4) * sizeof(int);
}
// once per context, before the first launch: lets the kernel take a whole CU's LDS
hipError_t pg_prepare();
// n graphs, one workgroup each; no synchronization
hipError_t launch_posegraph(const PgPtrs &P, int n, size_t lds_bytes, hipStream_t stream);

}  // namespace vio
