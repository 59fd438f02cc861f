// mfma_tiles.h — wave-level linear algebra on the matrix cores: 9 x 9 and 16 x 16 register tiles of
// v_mfma_f64_16x16x4, their loads / stores, the one-wave Cholesky factorizations and the tile TRSM / update.
// Built by hipcc and, with -DVIO_SIMT, on the host with the lane semantics of tests/emul/simt.h.
#pragma once

#include "spmd.h"

namespace vio {

constexpr int kSB = 9;           // speed-bias block

#ifdef VIO_SIMT
typedef ::simt::v4d v4d;
#else
typedef double v4d __attribute__((ext_vector_type(4)));
#endif

// v_mfma_f64_16x16x4_f64: D = A(16x4) B(4x16) + C. Lane l supplies A[l&15][l>>4] and B[l>>4][l&15]; it receives
// D[(l>>4) + 4 r][l&15] in element r (the f64 C/D map differs from the f32 one, cdna_hip_programming.md §3).
VIO_DEV v4d mfma_f64(double a, double b, v4d c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// ---- wave-level device helpers (matrix cores, v_readlane) ------------------------------------------

// Value of x held by `lane` (compile-time constant) broadcast to the whole wave through SGPRs.
VIO_DEV double lane_bcast(double x, int lane) {
  int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
  int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
  return __hiloint2double(hi, lo);
}
// Sum over the four lanes of a quad (DPP quad_perm [1,0,3,2] then [2,3,0,1]); every lane of the quad gets the total.
VIO_DEV double quad_sum_f64(double v) {
  v += dpp_move_f64<0xB1, 0xf>(v);
  v += dpp_move_f64<0x4E, 0xf>(v);
  return v;
}

// Layouts of v_mfma_f64_16x16x4 (lane l: li = l & 15, kq = l >> 4):
//   operand layout of a tile X: k-step s takes X[li][4 s + kq] as A operand (rows of the product) and, for products
//   with X^T on the right, as B operand;  accumulator layout: element r is [kq + 4 r][li].
// The accumulator layout of a tile T is at the same time the B-operand layout of T over four k-steps (element r = k-step
// r), so chains of products M1 (M2 T) never leave the registers.

// Under register pressure the scheduler sinks every LDS read to its first use: a ds_read, s_waitcnt lgkmcnt(0), the
// select that masks it, the next ds_read... -- one LDS latency (~120 cycles) per VALUE on the serial chains of the
// factorization. The fetch helpers below therefore read raw (clamped addresses, nothing consumes the value), then a
// scheduling fence, then mask: one latency per batch.

// ---- 9 x 9 speed-bias blocks (row-major, ld 9) in 16 x 16 register tiles --------------------------------------------
// X[li][4 s + kq], zero outside the block (k-steps 0..2 cover k < 12)
VIO_DEV void load_op9_raw(cldsd X, int li, int kq, double out[3]) {
  cldsd p = X + (li < kSB ? li : 0) * kSB + kq;
  out[0] = p[0], out[1] = p[4], out[2] = p[kq == 0 ? 8 : 0];
}
VIO_DEV void mask_op9(int li, int kq, double out[3]) {
  const bool iok = li < kSB;
  out[0] = iok ? out[0] : 0.0, out[1] = iok ? out[1] : 0.0, out[2] = (iok && kq == 0) ? out[2] : 0.0;
}
VIO_DEV void load_op9(cldsd X, int li, int kq, double out[3]) {
  load_op9_raw(X, li, kq, out);
  VIO_SCHED_FENCE();
  mask_op9(li, kq, out);
}
// Linv[li][4 s + kq] of a factored diagonal block (potrf9_inv_wave): strict lower part of L^-1 transposed above the
// diagonal (D[kk][n] = Linv[n][kk], kk < n), 1 / L_nn in ldinv_k. As A operand: Linv (.) ; as B operand: (.) L^-T.
VIO_DEV void load_linv9_raw(cldsd D, cldsd ldinv_k, int li, int kq, double out[4]) {
  const int n = li < kSB ? li : 0;
  out[3] = ldinv_k[n];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const int kk = 4 * s + kq;
    out[s] = D[(kk < n ? kk : 0) * kSB + n];
  }
}
VIO_DEV void mask_linv9(int li, int kq, double out[4]) {
  const bool iok = li < kSB;
  const int n = iok ? li : 0;
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const int kk = 4 * s + kq;
    out[s] = (iok && kk < n) ? out[s] : ((iok && kk == n) ? out[3] : 0.0);
  }
}
VIO_DEV void load_linv9(cldsd D, cldsd ldinv_k, int li, int kq, double out[4]) {
  load_linv9_raw(D, ldinv_k, li, kq, out);
  VIO_SCHED_FENCE();
  mask_linv9(li, kq, out);
}

// Cholesky of one 9 x 9 diagonal block AND the inverse of its factor by one wave, entirely on the matrix cores.
// The block lives in the f64 accumulator layout as a full symmetric matrix; pivot c: row c sits in the 16 lanes
// kq == (c & 3), element c >> 2, which is exactly where the A and the B operand of k-slot (c & 3) are fetched from, so the
// rank-1 update D -= l l^T is ONE v_mfma with a = b = l and no data movement. ET (initially I) receives the same
// eliminations, ET -= l e^T with e = ET[c][:] / L_cc, which leaves e = row c of L^-1. with_update: D -= E E^T first
// (E = the factored coupling block to the frame eliminated before, operand layout from LDS) -- the look-ahead of the
// band. Stored: L in the lower triangle (with diagonal), L^-1's strict lower part TRANSPOSED in the strict upper
// triangle, 1 / L_cc in ldinv_k. Returns false if a pivot is <= 0.
// (Four pivots per step like potrf16_wave -- 4 + 4 + 1 -- was built for this block as well: 2 196 against 2 124 cycles alone, 2 473
// against 2 440 with the E update, window kernel +0.5 %: with ONE matrix instruction per pivot and the next pivot's reciprocal root in
// its shadow the rank-1 form is already at the cost of the blocked one. Not kept.)
VIO_DEV bool potrf9_inv_wave(ldsd D, cldsd Eprev, bool with_update, ldsd ldinv_k, int lane) {
  // Round 6: ONE matrix instruction per pivot. The block only fills 9 x 9 of the 16 x 16 tile; the inverse rides in the rest of
  // the SAME tile as a symmetric border:  T = [ A  E ; E^T  * ],  E = columns 0..6 of the running inverse (rows 0..8, tile
  // columns 9..15; initially the identity). The rank-1 update T -= v v^T with v = (row c of T) / L_cc = [l | e] then applies
  // A -= l l^T and E -= l e^T at once -- rounds 3-5 kept the inverse in a second accumulator and paid a second 64-cycle
  // instruction per pivot (an f64 matrix instruction is 16 passes of the vector unit's own double-precision pipe on this chip).
  // Column 7 of the inverse has ONE entry below the diagonal, L^-1[8][7] = -L[8][7] / (L_77 L_88): formed by hand; column 8 none.
  const int n = lane & 15, kq = lane >> 4;
  v4d A;
  double l[3];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = kq + 4 * r;
    const bool ok = m < kSB && n < kSB;
    const int hi = m > n ? m : n, lo = m > n ? n : m;
    A[r] = D[ok ? hi * kSB + lo : 0];
  }
  load_op9_raw(Eprev, n, kq, l);
  VIO_SCHED_FENCE();
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = kq + 4 * r;
    // (the border: E[m][n - 9] = [m == n - 9] right of the block, its transpose below it)
    A[r] = (m < kSB && n < kSB) ? A[r] : ((m + 9 == n || n + 9 == m) ? 1.0 : 0.0);
  }
  if (with_update) {
    mask_op9(n, kq, l);
#pragma unroll
    for (int s = 0; s < 3; s++) A = mfma_f64(-l[s], l[s], A);
  }
  // Everything in this loop is on the critical path of the solve and nothing in a wave overlaps its own matrix
  // instructions, so the loop carries no bookkeeping: a pivot <= 0 shows up as a NaN / inf reciprocal root and is tested
  // once at the end.
  double keep[3] = {0.0, 0.0, 0.0}, myinv = 0.0, l87 = 0.0, y7 = 0.0, linv87 = 0.0;
  double dcc = lane_bcast(A[0], 0);
#pragma unroll
  for (int c = 0; c < kSB; c++) {
    double y = __builtin_amdgcn_rsq(dcc);
    const double h = 0.5 * dcc;
    y = y * fma(-h * y, y, 1.5);  // (v_rsq_f64 is specified to 2^29 ulp, ~2^-23 relative: one Newton step leaves ~1.5 e^2 = ~2^-45
                                  //  in every pivot, nine orders below the 1e-6 bar against the reference
                                  //  (tests/test_backend_gpu.py::test_step_quality_traces_on_badly_conditioned_windows holds low-parallax windows at
                                  //  the smallest mu to it); the second step cost 3 dependent operations on the pivot chain)
    const bool sel = kq == (c & 3);
    const double a = sel ? A[c >> 2] * y : 0.0;  // v: l[n] = L[n][c] for n < 9 (n == c: dcc / sqrt(dcc)), e[n - 9] = L^-1[c][n - 9] right of it
    keep[c >> 2] = sel ? a : keep[c >> 2];
    myinv = (n == c) ? y : myinv;
    if (c == 7) l87 = lane_bcast(a, 16 * 3 + 8), y7 = y;
    if (c == 8) linv87 = -(l87 * y7) * y;
    if (c + 1 < kSB) {
      // the next pivot D[c+1][c+1] - l[c+1]^2 is formed ahead of the matrix instruction, so its rsqrt chain runs in
      // its shadow instead of behind it
      const double lnext = lane_bcast(a, 16 * (c & 3) + c + 1);
      const double dold = lane_bcast(A[(c + 1) >> 2], 16 * ((c + 1) & 3) + c + 1);
      dcc = fma(-lnext, lnext, dold);
    }
    A = mfma_f64(-a, a, A);
  }
  // lane (n, kq) captured, at pivot c = kq + 4 j, L[n][c] (n >= c) or -- in the border -- L^-1[c][n - 9] (n - 9 < c), which goes
  // TRANSPOSED above the diagonal of the stored block
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int c = kq + 4 * j;
    if (c < kSB) {
      if (n < kSB && n >= c) D[n * kSB + c] = keep[j];
      if (n >= kSB && n - kSB < c) D[(n - kSB) * kSB + c] = keep[j];
    }
  }
  if (lane == 0) D[7 * kSB + 8] = linv87;
  if (kq == 0 && n < kSB) ldinv_k[n] = myinv;
  // rsq of a pivot <= 0 (or NaN) is NaN / inf, and every later pivot inherits it
  const bool bad = n < kSB && !(myinv > 0.0 && myinv < 1.7976931348623157e308);
  return __builtin_amdgcn_ballot_w64(bad) == 0;
}

// ---- 16 x 16 tiles of a row-major matrix (leading dimension per tile row) -------------------------------------------
// operand X[li][kq + 4 s]; rows >= rows are zero (the lane reads row 0 instead)
template <class MP>
VIO_DEV void tile_load_op_raw(MP X, int ld, int rows, int li, int kq, double out[4]) {
  auto p = X + (li < rows ? li : 0) * ld + kq;
  out[0] = p[0], out[1] = p[4], out[2] = p[8], out[3] = p[12];
}
VIO_DEV void tile_mask_op(int rows, int li, double out[4]) {
  const bool ok = li < rows;
  out[0] = ok ? out[0] : 0.0, out[1] = ok ? out[1] : 0.0, out[2] = ok ? out[2] : 0.0, out[3] = ok ? out[3] : 0.0;
}
template <class MP>
VIO_DEV void tile_load_op(MP X, int ld, int rows, int li, int kq, double out[4]) {
  tile_load_op_raw(X, ld, rows, li, kq, out);
  VIO_SCHED_FENCE();
  tile_mask_op(rows, li, out);
}
template <class MP>
VIO_DEV v4d tile_load_acc_raw(MP C, int ld, int rows, int li, int kq) {
  v4d a;
#pragma unroll
  for (int r = 0; r < 4; r++) a[r] = C[(kq + 4 * r < rows ? kq + 4 * r : 0) * ld + li];
  return a;
}
VIO_DEV v4d tile_mask_acc(v4d a, int rows, int kq) {
#pragma unroll
  for (int r = 0; r < 4; r++) a[r] = kq + 4 * r < rows ? a[r] : 0.0;
  return a;
}
template <class MP>
VIO_DEV v4d tile_load_acc(MP C, int ld, int rows, int li, int kq) {
  v4d a = tile_load_acc_raw(C, ld, rows, li, kq);
  VIO_SCHED_FENCE();
  return tile_mask_acc(a, rows, kq);
}
template <class MP>
VIO_DEV void tile_store_acc(MP C, int ld, int rows, int li, int kq, v4d a) {
  if (rows >= 16) {  // (uniform: four plain stores instead of four exec-masked regions)
    auto p = C + kq * ld + li;
    p[0] = a[0], p[4 * ld] = a[1], p[8 * ld] = a[2], p[12 * ld] = a[3];
    return;
  }
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (kq + 4 * r < rows) C[(kq + 4 * r) * ld + li] = a[r];
}
// Diagonal tile of the pose matrix: like potrf9_inv_wave on 16 x 16. nvalid rows / columns of the tile exist, the first
// npiv of them are pivots; rows past npiv (the carried right-hand side) are eliminated along and end up as their row of L.
// with_update: D -= Lprev Lprev^T first (the panel tile left of D, same tile row).
// Round 6: FOUR pivots per step. A rank-1 update used one of the four k-slots of the matrix instruction (a = b = the scaled pivot
// row in the lanes kq == c & 3, zeros elsewhere) and every pivot paid the chain matrix instruction -> vector read -> two broadcasts
// -> reciprocal root: ~306 cycles x 16. The rows 4 cb .. 4 cb + 3 of the running matrix are accumulator element cb of ALL lanes, i.e.
// exactly the B operand of one k-step: with M = L44^-1, the inverse Cholesky factor of the 4 x 4 diagonal block (ten broadcasts, then
// formed redundantly by every lane: four reciprocal roots, ~40 multiply-adds),
//     V = M R          one matrix instruction (A operand: M in the lanes li < 4; B operand: accumulator element cb)
//     T -= V^T V       one matrix instruction with a = b = V -- its four rows land in element 0 of the lanes kq = row: operand layout
// eliminates four pivots; the same M applied to the rows of the inverse's accumulator gives its four rows. 4 matrix instructions per
// four pivots instead of 8, and one broadcast / reciprocal-root round per block instead of four.
template <class MP>
VIO_DEV bool potrf16_wave(MP D, MP Lprev, int ld, int nvalid, int npiv, bool with_update, ldsd ldinv_k, int lane) {
  const int n = lane & 15, kq = lane >> 4;
  v4d A, E;
  double l[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = kq + 4 * r;
    const bool ok = m < nvalid && n < nvalid;
    const int hi = m > n ? m : n, lo = m > n ? n : m;
    A[r] = D[ok ? hi * ld + lo : 0];
  }
  tile_load_op_raw(Lprev, ld, nvalid, n, kq, l);
  VIO_SCHED_FENCE();
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = kq + 4 * r;
    A[r] = (m < nvalid && n < nvalid) ? A[r] : 0.0;
    E[r] = (m == n) ? 1.0 : 0.0;
  }
  if (with_update) {
    tile_mask_op(nvalid, n, l);
#pragma unroll
    for (int s = 0; s < 4; s++) A = mfma_f64(-l[s], l[s], A);
  }
  double keep[4] = {0.0, 0.0, 0.0, 0.0}, myinv = 0.0;
  const int mi = (n < 4 && kq <= n) ? n * (n + 1) / 2 + kq : -1;  // which entry of M this lane feeds into the A operand
#pragma unroll
  for (int cb = 0; cb < 4; cb++) {
    if (4 * cb < npiv) {  // (uniform)
      // the diagonal block: element (row 4 cb + i, column 4 cb + j) is accumulator element cb of lane (n = 4 cb + j, kq = i)
      double b[10];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) b[i * (i + 1) / 2 + j] = lane_bcast(A[cb], 16 * i + 4 * cb + j);
      const bool p1 = 4 * cb + 1 < npiv, p2 = 4 * cb + 2 < npiv, p3 = 4 * cb + 3 < npiv;  // (pivots past npiv: their row of M is zero)
      auto rsq1 = [](double d) {
        double y = __builtin_amdgcn_rsq(d);
        return y * fma(-(0.5 * d) * y, y, 1.5);  // (one Newton step: potrf9_inv_wave)
      };
      const double y0 = rsq1(b[0]);
      const double l10 = b[1] * y0, l20 = b[3] * y0, l30 = b[6] * y0;
      const double y1 = rsq1(fma(-l10, l10, b[2]));
      const double l21 = fma(-l20, l10, b[4]) * y1, l31 = fma(-l30, l10, b[7]) * y1;
      const double y2 = rsq1(fma(-l21, l21, fma(-l20, l20, b[5])));
      const double l32 = fma(-l31, l21, fma(-l30, l20, b[8])) * y2;
      const double y3 = rsq1(fma(-l32, l32, fma(-l31, l31, fma(-l30, l30, b[9]))));
      // M = L44^-1 (lower), row i scaled by y_i
      double M[10];
      M[0] = y0;
      M[1] = p1 ? -(l10 * y0) * y1 : 0.0, M[2] = p1 ? y1 : 0.0;
      M[3] = p2 ? -fma(l21, M[1], l20 * y0) * y2 : 0.0, M[4] = p2 ? -(l21 * M[2]) * y2 : 0.0, M[5] = p2 ? y2 : 0.0;
      M[6] = p3 ? -fma(l32, M[3], fma(l31, M[1], l30 * y0)) * y3 : 0.0, M[7] = p3 ? -fma(l32, M[4], l31 * M[2]) * y3 : 0.0;
      M[8] = p3 ? -(l32 * M[5]) * y3 : 0.0, M[9] = p3 ? y3 : 0.0;
      double mop = 0.0;
#pragma unroll
      for (int q = 0; q < 10; q++) mop = mi == q ? M[q] : mop;
      const v4d z = {0.0, 0.0, 0.0, 0.0};
      const v4d V = mfma_f64(mop, A[cb], z), VE = mfma_f64(mop, E[cb], z);
      const double vv = V[0], ve = VE[0];
      A = mfma_f64(-vv, vv, A);
      E = mfma_f64(-vv, ve, E);
      const int c = 4 * cb + kq;  // this lane's pivot of the block: column c of L below the diagonal, row c of L^-1 left of it
      keep[cb] = n >= c ? vv : ve;
      const double yn = (n & 3) == 0 ? y0 : (n & 3) == 1 ? y1 : (n & 3) == 2 ? y2 : y3;  // (1 / L_nn in every lane of column n)
      myinv = (n >> 2) == cb ? yn : myinv;
    }
  }
  if (n < nvalid) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int c = kq + 4 * j;
      if (c < npiv) D[n * ld + c] = keep[j];
    }
    if (kq == 0 && n < npiv) ldinv_k[n] = myinv;
  }
  const bool bad = n < npiv && !(myinv > 0.0 && myinv < 1.7976931348623157e308);
  return __builtin_amdgcn_ballot_w64(bad) == 0;
}
// (the rank-1 form of rounds 2-5: one pivot per step; tools/microbench/band_bench.hip times the two side by side)
template <class MP>
VIO_DEV bool potrf16_wave_rank1(MP D, MP Lprev, int ld, int nvalid, int npiv, bool with_update, ldsd ldinv_k, int lane) {
  const int n = lane & 15, kq = lane >> 4;
  v4d A, E;
  double l[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = kq + 4 * r;
    const bool ok = m < nvalid && n < nvalid;
    const int hi = m > n ? m : n, lo = m > n ? n : m;
    A[r] = D[ok ? hi * ld + lo : 0];
  }
  tile_load_op_raw(Lprev, ld, nvalid, n, kq, l);
  VIO_SCHED_FENCE();
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int m = kq + 4 * r;
    A[r] = (m < nvalid && n < nvalid) ? A[r] : 0.0;
    E[r] = (m == n) ? 1.0 : 0.0;
  }
  if (with_update) {
    tile_mask_op(nvalid, n, l);
#pragma unroll
    for (int s = 0; s < 4; s++) A = mfma_f64(-l[s], l[s], A);
  }
  double keep[4] = {0.0, 0.0, 0.0, 0.0}, myinv = 0.0;
  double dcc = lane_bcast(A[0], 0);
#pragma unroll
  for (int c = 0; c < 16; c++) {  // (constant trip count: c is a compile-time constant in every copy of the body)
    if (c < npiv) {
      double y = __builtin_amdgcn_rsq(dcc);
      const double h = 0.5 * dcc;
      y = y * fma(-h * y, y, 1.5);  // (one Newton step: potrf9_inv_wave)
      const bool sel = kq == (c & 3);
      const double a = sel ? A[c >> 2] * y : 0.0;
      const double e = sel ? E[c >> 2] * y : 0.0;
      keep[c >> 2] = sel ? (n >= c ? a : e) : keep[c >> 2];
      myinv = (n == c) ? y : myinv;
      if (c + 1 < 16) {
        const double lnext = lane_bcast(a, 16 * (c & 3) + c + 1);
        const double dold = lane_bcast(A[(c + 1) >> 2], 16 * ((c + 1) & 3) + c + 1);
        dcc = fma(-lnext, lnext, dold);
      }
      A = mfma_f64(-a, a, A);
      E = mfma_f64(-a, e, E);
    }
  }
  if (n < nvalid) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int c = kq + 4 * j;
      if (c < npiv) D[n * ld + c] = keep[j];
    }
    if (kq == 0 && n < npiv) ldinv_k[n] = myinv;
  }
  const bool bad = n < npiv && !(myinv > 0.0 && myinv < 1.7976931348623157e308);
  return __builtin_amdgcn_ballot_w64(bad) == 0;
}
// A_ik <- A_ik L_kk^-T (panel tile below a factored FULL diagonal tile: 16 pivots)
template <class MP>
VIO_DEV void tile_trsm(MP Aik, int ld_i, int rows, MP Dkk, int ld_k, cldsd ldinv_k, int li, int kq) {
  double a[4], x[4];
  tile_load_op_raw(Aik, ld_i, rows, li, kq, a);
  const double dg = ldinv_k[li];
#pragma unroll
  for (int s = 0; s < 4; s++) x[s] = Dkk[(4 * s + kq) * ld_k + li];  // B[kk][li] = Linv[li][kk]: above the diagonal of Dkk for kk < li
  VIO_SCHED_FENCE();
  tile_mask_op(rows, li, a);
  v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int kk = 4 * s + kq;
    const double bb = kk < li ? x[s] : (kk == li ? dg : 0.0);
    acc = mfma_f64(a[s], bb, acc);
  }
  tile_store_acc(Aik, ld_i, rows, li, kq, acc);
}
// C_ij -= A_ik A_jk^T
template <class MP>
VIO_DEV void tile_update(MP C, int ld_i, int rows_i, MP A, MP B, int ld_j, int rows_j, int li, int kq) {
  double a[4], b[4];
  tile_load_op_raw(A, ld_i, rows_i, li, kq, a), tile_load_op_raw(B, ld_j, rows_j, li, kq, b);
  v4d acc = tile_load_acc_raw(C, ld_i, rows_i, li, kq);
  VIO_SCHED_FENCE();
  tile_mask_op(rows_i, li, a), tile_mask_op(rows_j, li, b);
  acc = tile_mask_acc(acc, rows_i, kq);
#pragma unroll
  for (int s = 0; s < 4; s++) acc = mfma_f64(-a[s], b[s], acc);
  tile_store_acc(C, ld_i, rows_i, li, kq, acc);
}

}  // namespace vio
