// factors.h — the factor evaluations the solvers share (window solve and marginalization, motion-only PnP window):
// visual projection, raw IMU residual and the dx of a prior block, in local coordinates. Plain per-thread code.
#pragma once

#include "spmd.h"

namespace vio {

constexpr int kPreintDoubles = 467;

// ProjectionFactor::Evaluate (projection_facor.cpp:16-99) in local coordinates. Jex optional.
template <class PA, class PE>
VIO_DEV void projection_eval(double s_info, PA pose_i, PA pose_j, PE ex, double inv_dep, const double *pts_i,
                             const double *pts_j, bool jac, double *r, double *Ji, double *Jj, double *Jex, double *Jl) {
  Quat Qi{pose_i[3], pose_i[4], pose_i[5], pose_i[6]}, Qj{pose_j[3], pose_j[4], pose_j[5], pose_j[6]},
      qic{ex[3], ex[4], ex[5], ex[6]};
  double pc_i[3] = {pts_i[0] / inv_dep, pts_i[1] / inv_dep, pts_i[2] / inv_dep};
  double t[3], p_imu_i[3], p_w[3], p_imu_j[3], p_c_j[3];
  qrot(qic, pc_i, t);
  for (int k = 0; k < 3; k++) p_imu_i[k] = t[k] + ex[k];
  qrot(Qi, p_imu_i, t);
  for (int k = 0; k < 3; k++) p_w[k] = t[k] + pose_i[k];
  double d[3] = {p_w[0] - pose_j[0], p_w[1] - pose_j[1], p_w[2] - pose_j[2]};
  qrot(qinv(Qj), d, p_imu_j);
  double e[3] = {p_imu_j[0] - ex[0], p_imu_j[1] - ex[1], p_imu_j[2] - ex[2]};
  qrot(qinv(qic), e, p_c_j);
  double dep_j = p_c_j[2];
  r[0] = s_info * (p_c_j[0] / dep_j - pts_j[0]);
  r[1] = s_info * (p_c_j[1] / dep_j - pts_j[1]);
  if (!jac) return;
  double Ri[9], Rj[9], ric[9], ricT[9], RjT[9];
  qtoR(Qi, Ri), qtoR(Qj, Rj), qtoR(qic, ric);
  mat3T(ric, ricT), mat3T(Rj, RjT);
  double red[6] = {s_info * (1. / dep_j), 0, s_info * (-p_c_j[0] / (dep_j * dep_j)),
                   0, s_info * (1. / dep_j), s_info * (-p_c_j[1] / (dep_j * dep_j))};
  double A[9], B[9], S[9], T9[9];
  mat3mul(ricT, RjT, A);
  mat3mul(A, Ri, B);
  skew3(p_imu_i, S);
  mat3mul(B, S, T9);
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 3; j++) {
      Ji[i * 6 + j] = red[i * 3] * A[j] + red[i * 3 + 1] * A[3 + j] + red[i * 3 + 2] * A[6 + j];
      Ji[i * 6 + 3 + j] = -(red[i * 3] * T9[j] + red[i * 3 + 1] * T9[3 + j] + red[i * 3 + 2] * T9[6 + j]);
    }
  skew3(p_imu_j, S);
  mat3mul(ricT, S, T9);
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 3; j++) {
      Jj[i * 6 + j] = -(red[i * 3] * A[j] + red[i * 3 + 1] * A[3 + j] + red[i * 3 + 2] * A[6 + j]);
      Jj[i * 6 + 3 + j] = red[i * 3] * T9[j] + red[i * 3 + 1] * T9[3 + j] + red[i * 3 + 2] * T9[6 + j];
    }
  double Bric[9], v3[3];
  mat3mul(B, ric, Bric);
  if (Jex) {  // projection_facor.cpp:76-86 (the extrinsic is a kept block of the marginalization prior)
    double RjTRi[9], M1[9], C1[9], Spc[9], T1[9], v[3], Sv[9], u[3], w3[3], Sw[9];
    mat3mul(RjT, Ri, RjTRi);
    for (int i = 0; i < 9; i++) M1[i] = RjTRi[i] - (i % 4 == 0);
    mat3mul(ricT, M1, C1);
    skew3(pc_i, Spc);
    mat3mul(Bric, Spc, T1);
    mat3vec(Bric, pc_i, v);
    skew3(v, Sv);
    double exv[3] = {ex[0], ex[1], ex[2]};
    mat3vec(Ri, exv, u);
    for (int k = 0; k < 3; k++) u[k] += pose_i[k] - pose_j[k];
    mat3vec(RjT, u, w3);
    for (int k = 0; k < 3; k++) w3[k] -= ex[k];
    mat3vec(ricT, w3, u);
    skew3(u, Sw);
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < 3; j++) {
        Jex[i * 6 + j] = red[i * 3] * C1[j] + red[i * 3 + 1] * C1[3 + j] + red[i * 3 + 2] * C1[6 + j];
        double c0 = -T1[j] + Sv[j] + Sw[j], c1 = -T1[3 + j] + Sv[3 + j] + Sw[3 + j],
               c2 = -T1[6 + j] + Sv[6 + j] + Sw[6 + j];
        Jex[i * 6 + 3 + j] = red[i * 3] * c0 + red[i * 3 + 1] * c1 + red[i * 3 + 2] * c2;
      }
  }
  mat3vec(Bric, pts_i, v3);
  for (int i = 0; i < 2; i++)
    Jl[i] = (red[i * 3] * v3[0] + red[i * 3 + 1] * v3[1] + red[i * 3 + 2] * v3[2]) * -1.0 / (inv_dep * inv_dep);
}

// The same factor from rotation MATRICES prepared once per evaluation (w.rot: one per frame, then r_ic), for the
// solver's inner loops: four mat-vecs for the residual and, with jac, (reduce A) chained through R_i and r_ic instead
// of five dense 3x3 products. Equal to projection_eval up to rounding (different association of the same products).
// Jex (marginalization: the extrinsic is a kept block of the next prior) from the same chains: with B = r_ic^T R_j^T R_i,
//   d r / d t_ic     = reduce (B - r_ic^T)
//   d r / d theta_ic = reduce (-B r_ic skew(pc_i) + skew(p_c_j))
// (projection_facor.cpp:76-86 adds skew(B r_ic pc_i) and skew(r_ic^T (R_j^T (R_i t_ic + P_i - P_j) - t_ic)): the two vectors sum
// to p_c_j).
template <class PR, class PA, class PE>
VIO_DEV void projection_eval_rot(double s_info, PR Ri_, PA pose_i, PR Rj_, PA pose_j, PR ric_, PE ex, double inv_dep,
                                 const double *pts_i, const double *pts_j, bool jac, double *r, double *Ji, double *Jj,
                                 double *Jl, double *Jex = nullptr) {
  double Ri[9], Rj[9], ric[9];
#pragma unroll
  for (int k = 0; k < 9; k++) Ri[k] = Ri_[k], Rj[k] = Rj_[k], ric[k] = ric_[k];
  const double tic[3] = {ex[0], ex[1], ex[2]};
  const double pi3[3] = {pts_i[0], pts_i[1], pts_i[2]};
  const double dep_i = rcp_f(inv_dep);
  const double pc_i[3] = {pi3[0] * dep_i, pi3[1] * dep_i, pi3[2] * dep_i};
  double p_imu_i[3], p_w[3], p_imu_j[3], p_c_j[3], d[3], e[3];
  for (int a = 0; a < 3; a++) p_imu_i[a] = ric[3 * a] * pc_i[0] + ric[3 * a + 1] * pc_i[1] + ric[3 * a + 2] * pc_i[2] + tic[a];
  for (int a = 0; a < 3; a++) p_w[a] = Ri[3 * a] * p_imu_i[0] + Ri[3 * a + 1] * p_imu_i[1] + Ri[3 * a + 2] * p_imu_i[2] + pose_i[a];
  for (int a = 0; a < 3; a++) d[a] = p_w[a] - pose_j[a];
  for (int a = 0; a < 3; a++) p_imu_j[a] = Rj[a] * d[0] + Rj[3 + a] * d[1] + Rj[6 + a] * d[2];  // R_j^T d
  for (int a = 0; a < 3; a++) e[a] = p_imu_j[a] - tic[a];
  for (int a = 0; a < 3; a++) p_c_j[a] = ric[a] * e[0] + ric[3 + a] * e[1] + ric[6 + a] * e[2];  // r_ic^T e
  const double idep_j = rcp_f(p_c_j[2]);
  r[0] = s_info * (p_c_j[0] * idep_j - pts_j[0]);
  r[1] = s_info * (p_c_j[1] * idep_j - pts_j[1]);
  if (!jac) return;
  // reduce (2x3, projection_facor.cpp:46-50) has the sparsity [s/z 0 -s x/z^2 ; 0 s/z -s y/z^2]
  const double rz = s_info * idep_j, rx = -(rz * p_c_j[0]) * idep_j, ry = -(rz * p_c_j[1]) * idep_j;
  double A[9];  // r_ic^T R_j^T
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) A[3 * a + b] = ric[a] * Rj[3 * b] + ric[3 + a] * Rj[3 * b + 1] + ric[6 + a] * Rj[3 * b + 2];
  double RA[6], RB[6], RC[6], RT[6];
  for (int b = 0; b < 3; b++) RA[b] = rz * A[b] + rx * A[6 + b], RA[3 + b] = rz * A[3 + b] + ry * A[6 + b];  // reduce A
  for (int i = 0; i < 2; i++)
    for (int b = 0; b < 3; b++) {
      RB[3 * i + b] = RA[3 * i] * Ri[b] + RA[3 * i + 1] * Ri[3 + b] + RA[3 * i + 2] * Ri[6 + b];        // reduce A R_i
      RT[3 * i + b] = (i == 0 ? rz * ric[3 * b] : rz * ric[3 * b + 1]) + (i == 0 ? rx : ry) * ric[3 * b + 2];  // reduce r_ic^T
    }
  for (int i = 0; i < 2; i++)
    for (int b = 0; b < 3; b++)
      RC[3 * i + b] = RB[3 * i] * ric[b] + RB[3 * i + 1] * ric[3 + b] + RB[3 * i + 2] * ric[6 + b];     // reduce A R_i r_ic
  for (int i = 0; i < 2; i++) {
    const double *u = RB + 3 * i, *t = RT + 3 * i;
    // u skew(p) = (u1 p2 - u2 p1, u2 p0 - u0 p2, u0 p1 - u1 p0)
    Ji[i * 6 + 0] = RA[3 * i], Ji[i * 6 + 1] = RA[3 * i + 1], Ji[i * 6 + 2] = RA[3 * i + 2];
    Ji[i * 6 + 3] = -(u[1] * p_imu_i[2] - u[2] * p_imu_i[1]);
    Ji[i * 6 + 4] = -(u[2] * p_imu_i[0] - u[0] * p_imu_i[2]);
    Ji[i * 6 + 5] = -(u[0] * p_imu_i[1] - u[1] * p_imu_i[0]);
    Jj[i * 6 + 0] = -RA[3 * i], Jj[i * 6 + 1] = -RA[3 * i + 1], Jj[i * 6 + 2] = -RA[3 * i + 2];
    Jj[i * 6 + 3] = t[1] * p_imu_j[2] - t[2] * p_imu_j[1];
    Jj[i * 6 + 4] = t[2] * p_imu_j[0] - t[0] * p_imu_j[2];
    Jj[i * 6 + 5] = t[0] * p_imu_j[1] - t[1] * p_imu_j[0];
    Jl[i] = -(RC[3 * i] * pi3[0] + RC[3 * i + 1] * pi3[1] + RC[3 * i + 2] * pi3[2]) * (dep_i * dep_i);
    if (Jex) {
      const double *c = RC + 3 * i;
      const double q0 = i == 0 ? rz : 0.0, q1 = i == 0 ? 0.0 : rz, q2 = i == 0 ? rx : ry;  // row i of reduce
      Jex[i * 6 + 0] = u[0] - t[0], Jex[i * 6 + 1] = u[1] - t[1], Jex[i * 6 + 2] = u[2] - t[2];
      Jex[i * 6 + 3] = (q1 * p_c_j[2] - q2 * p_c_j[1]) - (c[1] * pc_i[2] - c[2] * pc_i[1]);
      Jex[i * 6 + 4] = (q2 * p_c_j[0] - q0 * p_c_j[2]) - (c[2] * pc_i[0] - c[0] * pc_i[2]);
      Jex[i * 6 + 5] = (q0 * p_c_j[1] - q1 * p_c_j[0]) - (c[0] * pc_i[1] - c[1] * pc_i[0]);
    }
  }
}

// Raw (un-whitened) IMU residual and, if Jraw != NULL, the dense 15x30 Jacobian [pose_i 6 | sb_i 9 | pose_j 6 | sb_j 9]
// (imu_factor.h:68-180 before the sqrt_info multiplication; integration_base.h:171-198).
template <class PA>
VIO_DEV void imu_eval_raw(double gravity, const double *pre, PA pose_i, PA sb_i, PA pose_j, PA sb_j, double *res,
                          double *Jraw) {
  const double sum_dt = pre[0];
  const double *delta_p = pre + 1, *delta_q = pre + 4, *delta_v = pre + 8, *lin_ba = pre + 11, *lin_bg = pre + 14;
  const double *J = pre + 17;
  PA Pi = pose_i, Pj = pose_j, Vi = sb_i, Bai = sb_i + 3, Bgi = sb_i + 6, Vj = sb_j, Baj = sb_j + 3, Bgj = sb_j + 6;
  Quat Qi{pose_i[3], pose_i[4], pose_i[5], pose_i[6]}, Qj{pose_j[3], pose_j[4], pose_j[5], pose_j[6]};
  Quat dq{delta_q[0], delta_q[1], delta_q[2], delta_q[3]};
  double dp_dba[9], dp_dbg[9], dq_dbg[9], dv_dba[9], dv_dbg[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      dp_dba[i * 3 + j] = J[(0 + i) * 15 + 9 + j];
      dp_dbg[i * 3 + j] = J[(0 + i) * 15 + 12 + j];
      dq_dbg[i * 3 + j] = J[(3 + i) * 15 + 12 + j];
      dv_dba[i * 3 + j] = J[(6 + i) * 15 + 9 + j];
      dv_dbg[i * 3 + j] = J[(6 + i) * 15 + 12 + j];
    }
  double dba[3], dbg[3], th[3], t1[3], t2[3], cdv[3], cdp[3];
  for (int k = 0; k < 3; k++) dba[k] = Bai[k] - lin_ba[k], dbg[k] = Bgi[k] - lin_bg[k];
  mat3vec(dq_dbg, dbg, th);
  Quat cdq = qmul(dq, Quat{th[0] / 2.0, th[1] / 2.0, th[2] / 2.0, 1.0});
  mat3vec(dv_dba, dba, t1), mat3vec(dv_dbg, dbg, t2);
  for (int k = 0; k < 3; k++) cdv[k] = delta_v[k] + t1[k] + t2[k];
  mat3vec(dp_dba, dba, t1), mat3vec(dp_dbg, dbg, t2);
  for (int k = 0; k < 3; k++) cdp[k] = delta_p[k] + t1[k] + t2[k];
  const double T = sum_dt;
  const double G[3] = {0, 0, gravity};
  Quat Qi_inv = qinv(Qi);
  double a[3], b[3], ra[3], rb[3];
  for (int k = 0; k < 3; k++) {
    a[k] = 0.5 * G[k] * T * T + Pj[k] - Pi[k] - Vi[k] * T;
    b[k] = G[k] * T + Vj[k] - Vi[k];
  }
  qrot(Qi_inv, a, ra), qrot(Qi_inv, b, rb);
  Quat qr = qmul(qinv(cdq), qmul(Qi_inv, Qj));
  for (int k = 0; k < 3; k++) {
    res[0 + k] = ra[k] - cdp[k];
    res[6 + k] = rb[k] - cdv[k];
    res[9 + k] = Baj[k] - Bai[k];
    res[12 + k] = Bgj[k] - Bgi[k];
  }
  res[3] = 2 * qr.x, res[4] = 2 * qr.y, res[5] = 2 * qr.z;
  if (!Jraw) return;
  // Jraw was zeroed once per solve (setup_imu_info); every evaluation overwrites the same non-zero 3x3 blocks
  double Rinv[9], M[9], S[9], Mq[9];
  qtoR(Qi_inv, Rinv);
  // columns: pose_i [0,6), sb_i [6,15), pose_j [15,21), sb_j [21,30)
  const int ld = 30, cpi = 0, csi = 6, cpj = 15, csj = 21;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Jraw[(0 + i) * ld + cpi + j] = -Rinv[i * 3 + j];
  skew3(ra, S);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Jraw[(0 + i) * ld + cpi + 3 + j] = S[i * 3 + j];
  qleft_qright33(qmul(qinv(Qj), Qi), cdq, M);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Jraw[(3 + i) * ld + cpi + 3 + j] = -M[i * 3 + j];
  skew3(rb, S);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Jraw[(6 + i) * ld + cpi + 3 + j] = S[i * 3 + j];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      Jraw[(0 + i) * ld + csi + 0 + j] = -Rinv[i * 3 + j] * T;
      Jraw[(0 + i) * ld + csi + 3 + j] = -dp_dba[i * 3 + j];
      Jraw[(0 + i) * ld + csi + 6 + j] = -dp_dbg[i * 3 + j];
      Jraw[(6 + i) * ld + csi + 0 + j] = -Rinv[i * 3 + j];
      Jraw[(6 + i) * ld + csi + 3 + j] = -dv_dba[i * 3 + j];
      Jraw[(6 + i) * ld + csi + 6 + j] = -dv_dbg[i * 3 + j];
      Jraw[(9 + i) * ld + csi + 3 + j] = -(double)(i == j);
      Jraw[(12 + i) * ld + csi + 6 + j] = -(double)(i == j);
    }
  qleft33(qmul(qmul(qinv(Qj), Qi), cdq), M);
  mat3mul(M, dq_dbg, Mq);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Jraw[(3 + i) * ld + csi + 6 + j] = -Mq[i * 3 + j];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Jraw[(0 + i) * ld + cpj + j] = Rinv[i * 3 + j];
  qleft33(qmul(qmul(qinv(cdq), Qi_inv), Qj), M);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Jraw[(3 + i) * ld + cpj + 3 + j] = M[i * 3 + j];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      Jraw[(6 + i) * ld + csj + 0 + j] = Rinv[i * 3 + j];
      Jraw[(9 + i) * ld + csj + 3 + j] = (double)(i == j);
      Jraw[(12 + i) * ld + csj + 6 + j] = (double)(i == j);
    }
}

// dx of one prior block (marginalization_factor.cpp:349-367)
template <class PX, class PD>
VIO_DEV void prior_block_dx(int gsize, PX x, const double *x0, PD dx) {
  if (gsize != 7) {
    for (int k = 0; k < gsize; k++) dx[k] = x[k] - x0[k];
    return;
  }
  for (int k = 0; k < 3; k++) dx[k] = x[k] - x0[k];
  Quat q = qmul(qinv(qfrom_pose(x0)), Quat{x[3], x[4], x[5], x[6]});
  double sgn = (q.w >= 0) ? 1.0 : -1.0;
  dx[3] = sgn * 2.0 * q.x, dx[4] = sgn * 2.0 * q.y, dx[5] = sgn * 2.0 * q.z;
}

}  // namespace vio
