// at_rigtrack.h -- rig track: the robot's field pose over a sliding window of recorded instants
// linked by odometry (a fixed-lag smoother), shared by host and device.
//
// The window is the last N <= kTrkMaxWindow instants, one connected chain.  An instant holds, per
// camera, the rig pose's selection of layout tags (CalCamObs, as the rig calibration stores it)
// and the odometry since its predecessor: the robot now in the previous instant's robot frame,
// x_prev = R_m x_now + t_m, with standard deviations sigma_rot (rad) and sigma_trans (m).  An
// instant without a tag is stored all the same and is held by its odometry alone.
//
// Unknowns: the robot's field pose at every instant, x_field = R_k x_robot + t_k, parameters
// (w, dt) as rig_apply_step.  Cost, a sum of squares:
//   vision    every selected corner of every camera at every instant, projected as rig_point does,
//             the pixel residual divided by sigma_px: the pixel sums of at_rigpose.h (64-slot tree
//             per camera, the cameras added in order) times wpx = 1 / (sigma_px sigma_px); a corner
//             with Pz <= 0 costs HUGE_VAL;
//   odometry  for k >= 1, with a = k - 1, b = k and E = R_m^T (R_a^T R_b):
//             rho = 1/2 (E[7] - E[5], E[2] - E[6], E[3] - E[1]) / sigma_rot,
//             tau = (R_a^T (t_b - t_a) - t_m) / sigma_trans.
//             Jacobian (trk_odom_rows), exact to first order in both poses' columns:
//             d rho / d w_b = 1/2 (tr(E) I - E^T),  d rho / d w_a = -1/2 (tr(E) I - E) R_m^T,
//             d tau / d w_a = [q]x with q = R_a^T (t_b - t_a),  d tau / d t_b = R_a^T = -d tau / d t_a.
//
// Start, a pure function of the stored window: an instant's own start is rig_solve_instant over
// its stored tags (trk_start; computed once per stored instant and kept, it depends on nothing
// else).  trk_fill, at every solve: the first instant with an own start takes it; going up, an
// instant with an own start takes it and one without takes its predecessor's pose composed with
// its odometry; the instants in front of the first are filled downwards the same way.  Nothing
// derived from another instant is kept between solves.
//
// `iters` Levenberg-Marquardt iterations, fixed, lambda from 1e-3.  The normal equations are block
// tridiagonal: D_k = (wpx U_k + Db_k) + Da_{k+1} (6 x 6; U_k the instant's vision sums, Da / Db
// the odometry factors' J_a^T J_a / J_b^T J_b, a missing term left out), g_k likewise, the coupling
// O_k = J_b^T J_a between k - 1 and k; every product sum over the six residual rows ascending.
//   accumulate  (trk_accum, per instant) the sums above at one state: the current one in the first
//               iteration, the candidate in every later one;
//   decide      (trk_decide, one team) the state's total cost, instants ascending, each
//               wpx px_k + odo_k; `factor_ok && cn < cost` takes the candidate (TrkCtl::which flips),
//               lambda / 10 (floor 1e-9), else lambda x 10;
//   solve       (trk_solve, the same team) D_k's diagonal times (1 + lambda) as d + lambda d; block
//               Cholesky in ascending k: L_0 = chol(D_0), B_k = O_k L_{k-1}^-T (row by row, columns
//               ascending), L_k = chol(D_k - B_k B_k^T) (the product's sum ascending, subtracted
//               once; the factor column by column as fp_solve6 forms it, except that a column's
//               i_j = 1 / L[j][j] is formed once and every division by a diagonal entry, here and
//               in B_k, the substitutions and the covariance, is a product with it: the chain is
//               serial and a division costs it several times a product); forward
//               y_k = L_k^-1 (-g_k - B_k y_{k-1}), back x_k = L_k^-T (y_k - B_{k+1}^T x_{k+1}), each
//               B product summed ascending from its first term and subtracted once.  A pivot that
//               is not positive is a failed factor: every step is zero, the iteration is rejected.
//               The candidates are rig_apply_step of the current poses.
// Both sets of sums are kept (sums[which], sums[which ^ 1]), so a rejected candidate costs nothing
// more.  After the last decision the same solve runs undamped at the final state; the covariance of
// the latest pose is (L_{N-1} L_{N-1}^T)^-1, order (w, t), no rescale (the residuals carry their
// sigmas); without a factor cov_valid = 0 and zeros.
//
// The kernels (at_kernels.hip: k_trk_*) and the CPU twin (at_rigtrack.cpp) instantiate these
// functions with at_rigcal.h's team over the same TrkBufs, device or host pointers.
// at_fieldpose.h's rules hold: no contraction, only + - * / sqrt, every sum in one stated order.
#pragma once

#include "at_rigcal.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace at {

constexpr int kTrkMaxWindow = 64;  // AT_RIGTRACK_MAX_WINDOW
constexpr int kTrkMaxIters = 16;
// an instant's sums at one state: U 21, g 6, px 1 | Da 36 | Db 36 | O 36 | ga 6 | gb 6 | odo 1
constexpr int kTrkDa = 28, kTrkDb = 64, kTrkO = 100, kTrkGa = 136, kTrkGb = 142, kTrkOdo = 148;
constexpr int kTrkSums = 152;

struct TrkOdom {
  double R[9], t[3];
  double sigma_rot, sigma_trans;
};

struct TrkCtl {
  double lambda, cost, cost0;
  double px, px0;     // the summed squared pixel error of the state, of the start
  int32_t which;      // the current state is pose[which], sums[which]; the candidate the other
  int32_t accepted, rejected;
  int32_t factor_ok;  // the last solve had a factor
  int32_t corners, used, cov_valid;
  int32_t any;        // an instant of the window has a start: else nothing is solved
};

struct TrkBufs {
  // per slot of the ring (an instant keeps its slot while it is in the window)
  const CalCamObs* obs;  // [W][n_cams]
  const TrkOdom* odom;   // [W] from the instant's predecessor to it
  RigRecord* rec;        // [W] the own start's record
  CalPose* own;          // [W] the own start
  int32_t* own_nt;       // [W] its n_tags; 0: none
  // per position k of the window, oldest first
  CalPose* pose[2];      // [W]
  double* sums[2];       // [W][kTrkSums]
  double* instpx;        // [W] the final state's summed squared pixel error
  double* cov;           // [36]
  TrkCtl* ctl;
  FpLayout lay;
  double tag_size, wpx;
  double fx[kRigMaxCams], fy[kRigMaxCams], cx[kRigMaxCams], cy[kRigMaxCams];
  CalPose ext[kRigMaxCams];
  int N, W, head, n_cams;
  AT_CAL_M int slot(int k) const { return (head + k) % W; }
  AT_CAL_M RigCam rigcam(int c) const {
    RigCam r = {fx[c], fy[c], cx[c], cy[c], {}, {}};
    for (int k = 0; k < 9; k++) r.ER[k] = ext[c].R[k];
    for (int k = 0; k < 3; k++) r.Et[k] = ext[c].t[k];
    return r;
  }
};

// the slots whose own start is still to be computed
struct TrkTodo {
  int32_t n;
  uint8_t slot[kTrkMaxWindow];
};

struct TrkSrc {
  const TrkBufs* b;
  int s;  // slot
  AT_CAL_M CalCamSrc cam(int c) const { return {b->obs + (size_t)s * b->n_cams + c}; }
  AT_CAL_M RigCam rigcam(int c) const { return b->rigcam(c); }
};

struct TrkShared {
  double cs[kRigMaxCams][kRigSums];
  double Ja[36], Jb[36], r[6];
};
struct TrkSolveShared {
  double D[kTrkMaxWindow][36];  // D_k, then D_k - B_k B_k^T
  double B[kTrkMaxWindow][36];  // O_k, then B_k
  double L[kTrkMaxWindow][36];
  double I[kTrkMaxWindow][6];   // 1 / L_k[j][j]
  double px[kTrkMaxWindow], odo[kTrkMaxWindow];  // the evaluated state's per-instant costs
  int32_t nt[kTrkMaxWindow];                     // own_nt by position
  double x[kTrkMaxWindow][6];   // -g_k, then y_k, then x_k
  double lambda;
  int32_t which, any;
};

// c = a^T b, 3x3 row-major, each entry (p + q) + r
AT_FP_HD void trk_mul_atb(const double* a, const double* b, double* c) {
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) c[r * 3 + k] = (a[r] * b[k] + a[3 + r] * b[3 + k]) + a[6 + r] * b[6 + k];
}

// pose b from pose a and the odometry from a to b: R_b = R_a R_m, t_b = R_a t_m + t_a
AT_FP_HD void trk_forward(const CalPose& a, const TrkOdom& m, CalPose* o) {
  double Rn[9], rt[3];
  fp_mul_ab(a.R, m.R, Rn);
  fp_rot(a.R, m.t, rt);
  for (int k = 0; k < 9; k++) o->R[k] = Rn[k];
  for (int k = 0; k < 3; k++) o->t[k] = rt[k] + a.t[k];
}
// pose a from pose b and the odometry from a to b: R_a = R_b R_m^T, t_a = t_b - R_a t_m
AT_FP_HD void trk_backward(const CalPose& b, const TrkOdom& m, CalPose* o) {
  double Rn[9], rt[3];
  fp_mul_abt(b.R, m.R, Rn);
  fp_rot(Rn, m.t, rt);
  for (int k = 0; k < 9; k++) o->R[k] = Rn[k];
  for (int k = 0; k < 3; k++) o->t[k] = b.t[k] - rt[k];
}

// the odometry residual r[6] between poses a and b, and its rows for a (Ja) and b (Jb), [6][6]
AT_FP_HD void trk_odom_rows(const CalPose& a, const CalPose& b, const TrkOdom& m, double* r, double* Ja, double* Jb) {
  double M[9], E[9], G[9], H[9];
  trk_mul_atb(a.R, b.R, M);
  trk_mul_atb(m.R, M, E);
  const double sr = m.sigma_rot, st = m.sigma_trans;
  r[0] = (0.5 * (E[7] - E[5])) / sr;
  r[1] = (0.5 * (E[2] - E[6])) / sr;
  r[2] = (0.5 * (E[3] - E[1])) / sr;
  const double d0 = b.t[0] - a.t[0], d1 = b.t[1] - a.t[1], d2 = b.t[2] - a.t[2];
  double q[3];
  for (int k = 0; k < 3; k++) {
    q[k] = (a.R[k] * d0 + a.R[3 + k] * d1) + a.R[6 + k] * d2;
    r[3 + k] = (q[k] - m.t[k]) / st;
  }
  const double tr = (E[0] + E[4]) + E[8];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) G[3 * i + j] = (i == j ? tr : 0.0) - E[3 * i + j];
  fp_mul_abt(G, m.R, H);
  for (int k = 0; k < 36; k++) Ja[k] = Jb[k] = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      Ja[6 * i + j] = (-0.5 * H[3 * i + j]) / sr;
      Jb[6 * i + j] = (0.5 * ((i == j ? tr : 0.0) - E[3 * j + i])) / sr;
      Ja[6 * (3 + i) + 3 + j] = -a.R[3 * j + i] / st;
      Jb[6 * (3 + i) + 3 + j] = a.R[3 * j + i] / st;
    }
  Ja[6 * 3 + 1] = -q[2] / st;
  Ja[6 * 3 + 2] = q[1] / st;
  Ja[6 * 4 + 0] = q[2] / st;
  Ja[6 * 4 + 2] = -q[0] / st;
  Ja[6 * 5 + 0] = -q[1] / st;
  Ja[6 * 5 + 1] = q[0] / st;
}

// sum over the six residual rows of x[i][a] y[i][b], ascending
AT_FP_HD double trk_col_dot(const double* x, int a, const double* y, int b) {
  double acc = x[a] * y[b];
  for (int i = 1; i < 6; i++) acc = acc + x[6 * i + a] * y[6 * i + b];
  return acc;
}

// the slots of held camera ci of the instant in slot s: the stored tags are the selection
template <class T>
AT_FP_HD void trk_slots(const T& tm, const TrkBufs& b, int s, int ci, FpSlot* slots) {
  const CalCamSrc cs = {b.obs + (size_t)s * b.n_cams + ci};
  uint32_t my_cand[T::NS], my_id[T::NS];
  const int m = cs.n();
#pragma unroll
  for (int q = 0; q < T::NS; q++) {
    const int j = tm.wave().slot(q) >> 2;
    my_cand[q] = j < m ? (uint32_t)j : 0u;
    my_id[q] = j < m ? (uint32_t)cs.id(j) : 0u;
  }
  fp_points(tm.wave(), cs, b.lay, b.tag_size, m, my_cand, my_id, slots);
}

// ---- the own start of the instant in slot s ----
template <class T>
AT_FP_HD void trk_start(const T& tm, RigShared& sh, const TrkBufs& b, int s) {
  const TrkSrc src = {&b, s};
  rig_solve_instant(tm, src, sh, b.lay, b.n_cams, b.tag_size, b.rec + s, (RigRecord*)nullptr);
  if (tm.leader()) {
    const RigRecord& r = b.rec[s];
    b.own_nt[s] = r.n_tags;
    for (int k = 0; k < 9; k++) b.own[s].R[k] = r.R[k];
    for (int k = 0; k < 3; k++) b.own[s].t[k] = r.t[k];
  }
}

// ---- every instant's start from the own starts and the odometry (one team; serial) ----
template <class T>
AT_FP_HD void trk_fill(const T& tm, const TrkBufs& b) {
  if (!tm.leader()) return;
  TrkCtl c = {};
  int k0 = -1;
  for (int k = 0; k < b.N && k0 < 0; k++)
    if (b.own_nt[b.slot(k)] > 0) k0 = k;
  c.any = k0 >= 0;
  if (k0 >= 0) {
    b.pose[0][k0] = b.own[b.slot(k0)];
    for (int k = k0 + 1; k < b.N; k++) {
      const int s = b.slot(k);
      if (b.own_nt[s] > 0) b.pose[0][k] = b.own[s];
      else trk_forward(b.pose[0][k - 1], b.odom[s], &b.pose[0][k]);
    }
    for (int k = k0 - 1; k >= 0; k--) trk_backward(b.pose[0][k + 1], b.odom[b.slot(k + 1)], &b.pose[0][k]);
  }
  *b.ctl = c;
}

// ---- instant k's sums at state pose[which ^ cand] ----
template <class T>
AT_FP_HD void trk_accum(const T& tm, TrkShared& sh, const TrkBufs& b, int k, bool cand) {
  if (!b.ctl->any) return;
  const int e = cand ? b.ctl->which ^ 1 : b.ctl->which;
  const int s = b.slot(k), nc = b.n_cams;
  double* out = b.sums[e] + (size_t)k * kTrkSums;
  const CalPose pose = b.pose[e][k];
  const bool tags = b.own_nt[s] > 0;
  if (tags) {
    for (int h = 0; h < T::NC; h++) {
      const int ci = tm.cam(h);
      if (ci >= nc) continue;
      FpSlot slots[T::NS];
      trk_slots(tm, b, s, ci, slots);
      const RigCam cam = b.rigcam(ci);
      double v[T::NS][kRigSums];
#pragma unroll
      for (int q = 0; q < T::NS; q++) {
        rig_slot_normal(slots[q], cam, pose.R, pose.t, v[q]);
        v[q][27] = rig_slot_cost(slots[q], cam, pose.R, pose.t);
      }
      tm.template wave_sums<kRigSums>(v, sh.cs[ci]);
    }
  }
  if (k >= 1 && tm.leader()) trk_odom_rows(b.pose[e][k - 1], pose, b.odom[s], sh.r, sh.Ja, sh.Jb);
  tm.barrier();
  for (int i = tm.first(); i < kTrkSums; i += tm.stride()) {
    double val = 0.0;
    if (i < kTrkDa) {
      if (tags) {
        val = sh.cs[0][i];
        for (int c = 1; c < nc; c++) val = val + sh.cs[c][i];
      }
    } else if (k >= 1) {
      if (i < kTrkDb) val = trk_col_dot(sh.Ja, (i - kTrkDa) / 6, sh.Ja, (i - kTrkDa) % 6);
      else if (i < kTrkO) val = trk_col_dot(sh.Jb, (i - kTrkDb) / 6, sh.Jb, (i - kTrkDb) % 6);
      else if (i < kTrkGa) val = trk_col_dot(sh.Jb, (i - kTrkO) / 6, sh.Ja, (i - kTrkO) % 6);
      else if (i < kTrkGb) {
        val = sh.Ja[i - kTrkGa] * sh.r[0];
        for (int q = 1; q < 6; q++) val = val + sh.Ja[6 * q + (i - kTrkGa)] * sh.r[q];
      } else if (i < kTrkOdo) {
        val = sh.Jb[i - kTrkGb] * sh.r[0];
        for (int q = 1; q < 6; q++) val = val + sh.Jb[6 * q + (i - kTrkGb)] * sh.r[q];
      } else if (i == kTrkOdo) {
        val = sh.r[0] * sh.r[0];
        for (int q = 1; q < 6; q++) val = val + sh.r[q] * sh.r[q];
      }
    }
    out[i] = val;
  }
}

// ---- the cost of the state just accumulated and what follows from it (leader) ----
// first: it is the start; else the candidate, taken or not.  px, odo, nt: the instants' pixel and
// odometry costs of that state and own_nt, by position (the team has read them side by side)
AT_FP_HD void trk_decide(const TrkBufs& b, const double* px_k, const double* odo_k, const int32_t* nt_k, bool first) {
  TrkCtl& c = *b.ctl;
  double cn = b.wpx * px_k[0], px = px_k[0];
  int tags = 0, used = 0;
  for (int k = 0; k < b.N; k++) {
    const int nt = nt_k[k];
    tags += nt > 0 ? nt : 0;
    used += nt > 0;
    if (k == 0) continue;
    cn = cn + (b.wpx * px_k[k] + odo_k[k]);
    px = px + px_k[k];
  }
  if (first) {
    c.lambda = 1e-3;
    c.cost = c.cost0 = cn;
    c.px = c.px0 = px;
    c.corners = 4 * tags;
    c.used = used;
    return;
  }
  if (c.factor_ok && cn < c.cost) {
    c.which ^= 1;
    c.cost = cn;
    c.px = px;
    c.accepted++;
    c.lambda = c.lambda / 10.0;
    if (c.lambda < 1e-9) c.lambda = 1e-9;
  } else {
    c.rejected++;
    c.lambda = c.lambda * 10.0;
  }
}

// ---- decide, then the block-tridiagonal solve at the current state (one team) ----
// final: undamped, the latest pose's covariance and the per-instant pixel sums; else the candidates
template <class T>
AT_FP_HD void trk_solve(const T& tm, TrkSolveShared& sh, const TrkBufs& b, bool first, bool final) {
  {
    const double* sm = b.sums[first ? b.ctl->which : b.ctl->which ^ 1];
    for (int k = tm.first(); k < b.N; k += tm.stride()) {
      sh.px[k] = sm[(size_t)k * kTrkSums + 27];
      sh.odo[k] = sm[(size_t)k * kTrkSums + kTrkOdo];
      sh.nt[k] = b.own_nt[b.slot(k)];
    }
  }
  tm.barrier();
  if (tm.leader()) {
    if (b.ctl->any) trk_decide(b, sh.px, sh.odo, sh.nt, first);
    sh.any = b.ctl->any;
    sh.which = b.ctl->which;
    sh.lambda = final ? 0.0 : b.ctl->lambda;
  }
  tm.barrier();
  if (!sh.any) return;
  const int N = b.N, which = sh.which;
  const double lambda = sh.lambda;
  const double* sums = b.sums[which];
  // assemble
#pragma unroll 6
  for (int e = tm.first(); e < N * 42; e += tm.stride()) {
    const int k = e / 42, i = e % 42;
    const double* q = sums + (size_t)k * kTrkSums;
    const bool tags = sh.nt[k] > 0;
    if (i < 36) {
      const int r = i / 6, c = i % 6;
      double v = tags ? b.wpx * q[r <= c ? fp_tri(r, c) : fp_tri(c, r)] : 0.0;
      if (k >= 1) v = v + q[kTrkDb + i];
      if (k + 1 < N) v = v + q[kTrkSums + kTrkDa + i];
      if (r == c) v = v + lambda * v;
      sh.D[k][i] = v;
      sh.B[k][i] = k >= 1 ? q[kTrkO + i] : 0.0;
    } else {
      const int a = i - 36;
      double v = tags ? b.wpx * q[21 + a] : 0.0;
      if (k >= 1) v = v + q[kTrkGb + a];
      if (k + 1 < N) v = v + q[kTrkSums + kTrkGa + a];
      sh.x[k][a] = -v;
    }
  }
  tm.barrier();
  // factor
  bool ok = true;
  for (int k = 0; k < N; k++) {
    if (k >= 1) {
      for (int r = tm.first(); r < 6; r += tm.stride()) {
        double row[6], Lp[36], Ip[6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
          row[c] = sh.B[k][6 * r + c];
          Ip[c] = sh.I[k - 1][c];
#pragma unroll
          for (int m = 0; m < c; m++) Lp[6 * c + m] = sh.L[k - 1][6 * c + m];
        }
#pragma unroll
        for (int c = 0; c < 6; c++) {
          double v = row[c];
#pragma unroll
          for (int m = 0; m < c; m++) v = v - row[m] * Lp[6 * c + m];
          row[c] = v * Ip[c];
        }
#pragma unroll
        for (int c = 0; c < 6; c++) sh.B[k][6 * r + c] = row[c];
      }
      tm.barrier();
      for (int e = tm.first(); e < 36; e += tm.stride()) {
        const double* bi = sh.B[k] + 6 * (e / 6);
        const double* bj = sh.B[k] + 6 * (e % 6);
        double acc = bi[0] * bj[0];
        for (int m = 1; m < 6; m++) acc = acc + bi[m] * bj[m];
        sh.D[k][e] = sh.D[k][e] - acc;
      }
      tm.barrier();
    }
    double* L = sh.L[k];
    const double* S = sh.D[k];
    for (int j = 0; j < 6; j++) {
      double s = S[6 * j + j];
      for (int m = 0; m < j; m++) s = s - L[6 * j + m] * L[6 * j + m];
      if (!(s > 0.0)) ok = false;
      const double ljj = sqrt(s), inv = 1.0 / ljj;
      for (int i = j + tm.first(); i < 6; i += tm.stride()) {
        if (i == j) {
          L[6 * j + j] = ljj;
          sh.I[k][j] = inv;
          continue;
        }
        double v = S[6 * i + j];
        for (int m = 0; m < j; m++) v = v - L[6 * i + m] * L[6 * j + m];
        L[6 * i + j] = v * inv;
      }
      tm.barrier();
    }
  }
  if (final) {
    const double* L = sh.L[N - 1];
    const double* I = sh.I[N - 1];
    for (int p = tm.first(); p < 6; p += tm.stride()) {
      double w[6];
      for (int i = 0; i < 6; i++) {
        double v = i == p ? 1.0 : 0.0;
        for (int m = 0; m < i; m++) v = v - L[6 * i + m] * w[m];
        w[i] = v * I[i];
      }
      for (int i = 5; i >= 0; i--) {
        double v = w[i];
        for (int m = i + 1; m < 6; m++) v = v - L[6 * m + i] * w[m];
        w[i] = v * I[i];
      }
      for (int i = 0; i < 6; i++) b.cov[6 * p + i] = ok ? w[i] : 0.0;
    }
    for (int k = tm.first(); k < N; k += tm.stride()) b.instpx[k] = sums[(size_t)k * kTrkSums + 27];
    if (tm.leader()) b.ctl->cov_valid = ok ? 1 : 0;
    return;
  }
  // substitute (one thread; a block's L, B and the neighbour's solution are read into locals first,
  // so the dependent chain runs in registers on the device: the operations and their order are the
  // stated ones)
  if (tm.leader()) {
    double Lr[36], Br[36], Ir[6], prev[6], cur[6];
    for (int k = 0; k < N; k++) {
#pragma unroll
      for (int i = 0; i < 6; i++) {
        cur[i] = sh.x[k][i];
        Ir[i] = sh.I[k][i];
#pragma unroll
        for (int m = 0; m < i; m++) Lr[6 * i + m] = sh.L[k][6 * i + m];
      }
      if (k >= 1) {
#pragma unroll
        for (int e = 0; e < 36; e++) Br[e] = sh.B[k][e];
      }
#pragma unroll
      for (int i = 0; i < 6; i++) {
        double v = cur[i];
        if (k >= 1) {
          double acc = Br[6 * i] * prev[0];
#pragma unroll
          for (int m = 1; m < 6; m++) acc = acc + Br[6 * i + m] * prev[m];
          v = v - acc;
        }
#pragma unroll
        for (int m = 0; m < i; m++) v = v - Lr[6 * i + m] * cur[m];
        cur[i] = v * Ir[i];
      }
#pragma unroll
      for (int i = 0; i < 6; i++) {
        sh.x[k][i] = cur[i];
        prev[i] = cur[i];
      }
    }
    for (int k = N - 1; k >= 0; k--) {
#pragma unroll
      for (int i = 0; i < 6; i++) {
        cur[i] = sh.x[k][i];
        Ir[i] = sh.I[k][i];
#pragma unroll
        for (int m = 0; m < i; m++) Lr[6 * i + m] = sh.L[k][6 * i + m];
      }
      if (k + 1 < N) {
#pragma unroll
        for (int e = 0; e < 36; e++) Br[e] = sh.B[k + 1][e];
      }
#pragma unroll
      for (int i = 5; i >= 0; i--) {
        double v = cur[i];
        if (k + 1 < N) {
          double acc = Br[i] * prev[0];
#pragma unroll
          for (int m = 1; m < 6; m++) acc = acc + Br[6 * m + i] * prev[m];
          v = v - acc;
        }
#pragma unroll
        for (int m = i + 1; m < 6; m++) v = v - Lr[6 * m + i] * cur[m];
        cur[i] = v * Ir[i];
      }
#pragma unroll
      for (int i = 0; i < 6; i++) {
        sh.x[k][i] = cur[i];
        prev[i] = cur[i];
      }
    }
    b.ctl->factor_ok = ok ? 1 : 0;
  }
  tm.barrier();
  for (int k = tm.first(); k < N; k += tm.stride()) {
    double d[6];
    for (int i = 0; i < 6; i++) d[i] = ok ? sh.x[k][i] : 0.0;
    const CalPose p = b.pose[which][k];
    CalPose pn;
    rig_apply_step(p.R, p.t, d, pn.R, pn.t);
    b.pose[which ^ 1][k] = pn;
  }
}

}  // namespace at

// ---- the tracker's host side (at_rigtrack.cpp; at_api.cpp adds the device buffers) ----
namespace at {
struct TrkGpu;  // at_api.cpp
}
struct at_rigtrack {
  int n_cams, max_hamming, window, iters;
  double tag_size, sigma_px;
  at_rigtrack_camera cams[at::kRigMaxCams];
  std::vector<int16_t> lut;
  std::vector<at::FpTag> tags;
  // the ring: slot (head + k) % window holds position k
  std::vector<at::CalCamObs> obs;  // [window][n_cams]
  std::vector<at::TrkOdom> odom;
  std::vector<double> stamp;
  std::vector<at::CalPose> own;    // the twin's own starts
  std::vector<int32_t> own_nt;     // -1: not yet computed
  std::vector<uint8_t> dev_stale;  // the slot's device copy and own start are not this instant's
  int head, n;
  // the last solve
  at_rigtrack_result result;
  std::vector<at_rigtrack_instant> instants;
  uint64_t ns[4];  // all kernels, start, accumulate, solve
  int profiling;
  at::TrkGpu* gpu;
  void (*gpu_free)(at::TrkGpu*);
};
namespace at {
// the parts of TrkBufs that do not depend on where the buffers live
void trk_fill_bufs(const at_rigtrack& t, TrkBufs* b);
// the records of a finished solve from its final buffers (host copies)
void trk_finish(at_rigtrack* t, const TrkCtl& ctl, const CalPose* pose, const double* cov, const double* instpx,
                const int32_t* own_nt, at_rigtrack_result* out);
}  // namespace at
