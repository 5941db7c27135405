// at_rigpose.h -- one robot pose per instant from the layout tags of every camera of a
// rig, shared by host and device.
//
// A rig is 1..kRigMaxCams cameras, each with its own intrinsics and its extrinsics
// x_robot = E_R x_cam + E_t (at_tag_detections' convention).  Frame f of every member's
// last batch is instant f.  The unknown is the robot in the field, x_field = R x_robot + t:
// the Levenberg-Marquardt minimum of the summed squared reprojection error, in pixels, of
// every selected corner of every camera, started from the best single-tag pose, with the
// covariance sigma^2 (J^T J)^-1 of the final pose.
//
// Camera i's slot 4j + c is corner c of its j-th selected tag; selection (fp_select), the
// slots' field points and pixels (fp_points), the 6 x 6 solve (fp_solve6) and the rotation
// helpers are at_fieldpose.h's.  A slot projects as
//   Q = R^T (X - t),  P = E_R^T (Q - E_t),  u = fx Px / Pz + cx,  v = fy Py / Pz + cy,
// and one with Pz <= 0 costs HUGE_VAL, so a sum with such a slot in it is never less than
// a finite cost: the one comparison `cn < cost` is the whole accept rule.
//
// The kernel (at_kernels.hip: k_rig, one workgroup per instant, one wave per camera, one
// lane per slot) and the CPU twin (at_rigpose.cpp: at_rig_pose_host, one thread holding
// every slot of every camera) instantiate rig_solve_instant with a "team" that tells how
// cameras and slots are spread over threads.  Both run the same IEEE operations in the same
// order (at_fieldpose.h's rules: no contraction, only + - * / sqrt), and every sum over
// the corners has one order:
//   * within a camera the 64-slot xor butterfly 32 .. 1 (unused slots hold +0.0);
//   * across cameras ((c0 + c1) + c2) + .. in camera order up to n_cams, a camera without
//     a tag adding +0.0.
// The per-camera sums cross through RigShared (LDS on the device, a local on the host):
// each camera's wave stores its sums in its row, a barrier, the rows are added up.  Two
// buffers are used in turn, so one barrier per sum is enough: a thread that stores into a
// buffer again has passed the barrier of the sum in between, which no thread reaches
// before it has read the buffer's earlier values.
// The tree fixes which pairs are added, not which lane adds them, and a + b == b + a bit for
// bit: the kernel's waves halve the values a lane carries at every butterfly step (lane i
// keeps one half of them and sends i ^ off the other), so each sum ends in one lane pair at a
// sixth of the shuffles, and lane i adds value i over the cameras for its whole wave.
#pragma once

#include "at_fieldpose.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace at {

constexpr int kRigMaxCams = 8;   // AT_RIG_MAX_CAMS
constexpr int kRigSums = 28;     // most values one sum carries: 21 J^T J + 6 J^T r (+ 1 spare)
constexpr int kRigChunk = 4;     // start candidates costed per sum

struct RigCam {
  double fx, fy, cx, cy;
  double ER[9], Et[3];  // x_robot = ER x_cam + Et
};

// at_rig_pose
struct RigRecord {
  int32_t n_tags;
  int32_t n_cams_used;
  int32_t tags_per_cam[kRigMaxCams];
  int32_t ids[kRigMaxCams][kFpMaxTags];
  double R[9];
  double t[3];
  double cov[36];
  double rms_px;
  int32_t cov_valid;
  int32_t steps_taken;
  int32_t rejected;
  int32_t dropped;
};
static_assert(sizeof(RigRecord) == 960, "RigRecord: 960 B per instant");

struct RigShared {
  double red[2][kRigMaxCams][kRigSums];
  double cand[kRigMaxCams][kFpMaxTags][12];  // each selected tag's field_T_robot: R (9), t (3)
  int32_t m[kRigMaxCams];
  int32_t dropped[kRigMaxCams];
  int32_t ids[kRigMaxCams][kFpMaxTags];
};

// P = E_R^T (R^T (X - t) - E_t); Q is kept for the Jacobian
AT_FP_HD void rig_point(const RigCam& cam, const double* R, const double* t, const double* X, double* Q, double* P) {
  const double d0 = X[0] - t[0], d1 = X[1] - t[1], d2 = X[2] - t[2];
#pragma unroll
  for (int k = 0; k < 3; k++) Q[k] = (R[k] * d0 + R[3 + k] * d1) + R[6 + k] * d2;
  const double e0 = Q[0] - cam.Et[0], e1 = Q[1] - cam.Et[1], e2 = Q[2] - cam.Et[2];
#pragma unroll
  for (int k = 0; k < 3; k++) P[k] = (cam.ER[k] * e0 + cam.ER[3 + k] * e1) + cam.ER[6 + k] * e2;
}

// squared reprojection error of one slot under (R, t); HUGE_VAL with its Z not positive
AT_FP_HD double rig_slot_cost(const FpSlot& s, const RigCam& cam, const double* R, const double* t) {
  if (!s.valid) return 0.0;
  double Q[3], P[3];
  rig_point(cam, R, t, s.X, Q, P);
  if (!(P[2] > 0.0)) return HUGE_VAL;
  const double ru = (cam.fx * (P[0] / P[2]) + cam.cx) - s.u;
  const double rv = (cam.fy * (P[1] / P[2]) + cam.cy) - s.v;
  return ru * ru + rv * rv;
}

// the slot's two residual rows: 21 J^T J products (upper triangle), then 6 J^T r, in o[27].
// Parameters (w, dt): R' = R dR(w), t' = t + dt, so dQ/dw = [Q]x, dQ/dt = -R^T, dP = E_R^T dQ.
AT_FP_HD void rig_slot_normal(const FpSlot& s, const RigCam& cam, const double* R, const double* t, double* o) {
  if (!s.valid) {
#pragma unroll
    for (int k = 0; k < 27; k++) o[k] = 0.0;
    return;
  }
  double Q[3], P[3];
  rig_point(cam, R, t, s.X, Q, P);
  const double xn = P[0] / P[2], yn = P[1] / P[2];
  const double ru = (cam.fx * xn + cam.cx) - s.u;
  const double rv = (cam.fy * yn + cam.cy) - s.v;
  // du/dP = (A, 0, B), dv/dP = (0, C, D)
  const double A = cam.fx / P[2], B = -(cam.fx * xn) / P[2];
  const double C = cam.fy / P[2], D = -(cam.fy * yn) / P[2];
  const double dQ[3][6] = {{0.0, -Q[2], Q[1], -R[0], -R[3], -R[6]},
                           {Q[2], 0.0, -Q[0], -R[1], -R[4], -R[7]},
                           {-Q[1], Q[0], 0.0, -R[2], -R[5], -R[8]}};
  double ju[6], jv[6];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const double m0 = (cam.ER[0] * dQ[0][c] + cam.ER[3] * dQ[1][c]) + cam.ER[6] * dQ[2][c];
    const double m1 = (cam.ER[1] * dQ[0][c] + cam.ER[4] * dQ[1][c]) + cam.ER[7] * dQ[2][c];
    const double m2 = (cam.ER[2] * dQ[0][c] + cam.ER[5] * dQ[1][c]) + cam.ER[8] * dQ[2][c];
    ju[c] = A * m0 + B * m2;
    jv[c] = C * m1 + D * m2;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = i; j < 6; j++) o[fp_tri(i, j)] = ju[i] * ju[j] + jv[i] * jv[j];
    o[21 + i] = ju[i] * ru + jv[i] * rv;
  }
}

// R' = R dR(w) with dR from q = (1, w / 2) normalised; t' = t + dt.  d = (w, dt).
AT_FP_HD void rig_apply_step(const double* R, const double* t, const double* d, double* Rn, double* tn) {
  const double h0 = 0.5 * d[0], h1 = 0.5 * d[1], h2 = 0.5 * d[2];
  const double n = sqrt(1.0 + ((h0 * h0 + h1 * h1) + h2 * h2));
  double dR[9];
  fp_quat_to_R(1.0 / n, h0 / n, h1 / n, h2 / n, dR);
  fp_mul_ab(R, dR, Rn);
  for (int k = 0; k < 3; k++) tn[k] = t[k] + d[3 + k];
}

// One sum of N values over every slot of every camera, in two halves.  rig_put: held camera
// k's wave sums its slots' values vals[s][i] (the 64-slot tree) and stores the N sums in the
// camera's row of red[buf].  rig_get: a barrier, then the rows are added in camera order; every
// thread returns with the same out[].  How a wave forms its sums and how the totals reach
// every thread is the team's business (wave_sums, across): the pairs added are the same.
template <class T>
AT_FP_HD int rig_next_buf(int* phase) {
  const int buf = *phase & 1;
  *phase = *phase + 1;
  return buf;
}
template <int N, class T>
AT_FP_HD void rig_put(const T& tm, RigShared& sh, int buf, int k, double (*vals)[N]) {
  tm.template wave_sums<N>(vals, sh.red[buf][tm.cam(k)]);
}
template <int N, class T>
AT_FP_HD void rig_get(const T& tm, RigShared& sh, int buf, int n_cams, double* out) {
  tm.barrier();
  tm.template across<N>(sh.red[buf], n_cams, out);
}

// cost of all slots of all cameras under (R, t)
template <class T>
AT_FP_HD double rig_cost(const T& tm, RigShared& sh, int* phase, int n_cams, FpSlot (*slots)[T::NS],
                         const RigCam* cams, const double* R, const double* t) {
  const int buf = rig_next_buf<T>(phase);
  for (int k = 0; k < T::NC; k++) {
    if (tm.cam(k) >= n_cams) continue;
    double e[T::NS][1];
#pragma unroll
    for (int s = 0; s < T::NS; s++) e[s][0] = rig_slot_cost(slots[k][s], cams[k], R, t);
    rig_put<1>(tm, sh, buf, k, e);
  }
  double c;
  rig_get<1>(tm, sh, buf, n_cams, &c);
  return c;
}

// the 21 + 6 sums of the normal equations at (R, t) into o[27]
template <class T>
AT_FP_HD void rig_normal(const T& tm, RigShared& sh, int* phase, int n_cams, FpSlot (*slots)[T::NS],
                         const RigCam* cams, const double* R, const double* t, double* o) {
  const int buf = rig_next_buf<T>(phase);
  for (int k = 0; k < T::NC; k++) {
    if (tm.cam(k) >= n_cams) continue;
    double ps[T::NS][27];
#pragma unroll
    for (int s = 0; s < T::NS; s++) rig_slot_normal(slots[k][s], cams[k], R, t, ps[s]);
    rig_put<27>(tm, sh, buf, k, ps);
  }
  rig_get<27>(tm, sh, buf, n_cams, o);
}

// Team T: NC cameras held by a thread, NS slots of each; cam(k) the k-th held camera's index
// (>= n_cams: none), wave() the FpWave / FpHostWave of a camera's 64 slots, wave_leader(),
// leader() (one thread of the team), barrier(), wave_sums<N>(vals, row) and
// across<N>(rows, n_cams, out) (rig_put / rig_get).
// Src: cam(i) the candidates of camera i at this instant, as fp_solve_frame's Src;
// rigcam(i) its RigCam.
// Every thread ends with the same record; the leader stores it to out (and out2 when given).
template <class T, class Src>
AT_FP_HD void rig_solve_instant(const T& tm, const Src& src, RigShared& sh, const FpLayout& lay, int n_cams,
                                double tag_size, RigRecord* out, RigRecord* out2) {
  // ---- per camera: select, points, each tag's own pose as a robot pose ----
  FpSlot slots[T::NC][T::NS];
  RigCam cams[T::NC];
  for (int k = 0; k < T::NC; k++) {
    const int ci = tm.cam(k);
    if (ci >= n_cams) continue;
    const auto cs = src.cam(ci);
    cams[k] = src.rigcam(ci);
    uint32_t my_cand[T::NS], my_id[T::NS];
    int m, dropped;
    fp_select(tm.wave(), cs, lay, my_cand, my_id, &m, &dropped);
    fp_points(tm.wave(), cs, lay, tag_size, m, my_cand, my_id, slots[k]);
    for (int j = 0; j < m; j++) {
      const int c = (int)tm.wave().from_slot(my_cand, 4 * j);
      const uint32_t id = tm.wave().from_slot(my_id, 4 * j);
      const FpTag& tg = lay.tags[lay.lut[id]];
      // field_T_cam = field_T_tag (cam_T_tag)^-1, then field_T_robot = field_T_cam (robot_T_cam)^-1
      double Rfc[9], tfc[3], rt[3], Rj[9], re[3];
      fp_mul_abt(tg.R, cs.pose_R(c), Rfc);
      fp_rot(Rfc, cs.pose_t(c), rt);
      for (int i = 0; i < 3; i++) tfc[i] = tg.t[i] - rt[i];
      fp_mul_abt(Rfc, cams[k].ER, Rj);
      fp_rot(Rj, cams[k].Et, re);
      if (tm.wave_leader()) {
        for (int i = 0; i < 9; i++) sh.cand[ci][j][i] = Rj[i];
        for (int i = 0; i < 3; i++) sh.cand[ci][j][9 + i] = tfc[i] - re[i];
        sh.ids[ci][j] = (int32_t)id;
      }
    }
    if (tm.wave_leader()) {
      sh.m[ci] = m;
      sh.dropped[ci] = dropped;
    }
  }
  tm.barrier();
  int n_tags = 0, n_used = 0, dropped = 0;
  for (int i = 0; i < n_cams; i++) {
    n_tags += sh.m[i];
    n_used += sh.m[i] > 0;
    dropped += sh.dropped[i];
  }

  // ---- start: the single-tag pose with the least total error ----
  int phase = 0;
  double R[9], t[3];
  double cost = HUGE_VAL;
  bool found = false;
  for (int i = 0; i < n_cams; i++) {
    const int mi = sh.m[i];
    for (int j0 = 0; j0 < mi; j0 += kRigChunk) {
      const int buf = rig_next_buf<T>(&phase);
      for (int k = 0; k < T::NC; k++) {
        if (tm.cam(k) >= n_cams) continue;
        double e[T::NS][kRigChunk];
#pragma unroll
        for (int q = 0; q < kRigChunk; q++) {
          const bool have = j0 + q < mi;
          const double* cd = sh.cand[i][have ? j0 + q : j0];
#pragma unroll
          for (int s = 0; s < T::NS; s++) e[s][q] = have ? rig_slot_cost(slots[k][s], cams[k], cd, cd + 9) : 0.0;
        }
        rig_put<kRigChunk>(tm, sh, buf, k, e);
      }
      double tot[kRigChunk];
      rig_get<kRigChunk>(tm, sh, buf, n_cams, tot);
#pragma unroll
      for (int q = 0; q < kRigChunk; q++)
        if (j0 + q < mi && tot[q] < cost) {  // (a NaN or an infinite cost never wins; ties stay with the earlier)
          cost = tot[q];
          found = true;
          const double* cd = sh.cand[i][j0 + q];
          for (int e = 0; e < 9; e++) R[e] = cd[e];
          for (int e = 0; e < 3; e++) t[e] = cd[9 + e];
        }
    }
  }
  if (!found) {  // no layout tag at this instant, or none whose pose puts every point in front
    if (tm.leader()) {
      RigRecord z = {};
      z.dropped = dropped;
      *out = z;
      if (out2) *out2 = z;
    }
    return;
  }
  fp_project_rotation(R);
  {
    const double c0 = rig_cost(tm, sh, &phase, n_cams, slots, cams, R, t);
    if (c0 < HUGE_VAL) cost = c0;  // (else: the start's own cost bounds the first step)
  }

  // ---- refine: kFpIters Levenberg-Marquardt iterations on the pixel residuals ----
  double lambda = 1e-3;
  int steps = 0, rejected = 0;
  for (int it = 0; it < kFpIters; it++) {
    double ag[27];
    rig_normal(tm, sh, &phase, n_cams, slots, cams, R, t, ag);
    double d[6], Rn[9], tn[3];
    // (a failed factor leaves d unusable, but the step's cost is summed all the same: every
    // thread passes the same barriers)
    const bool ok = fp_solve6(ag, ag + 21, lambda, d);
    if (!ok)
      for (int k = 0; k < 6; k++) d[k] = 0.0;
    rig_apply_step(R, t, d, Rn, tn);
    const double cn = rig_cost(tm, sh, &phase, n_cams, slots, cams, Rn, tn);
    if (ok && cn < cost) {
      for (int k = 0; k < 9; k++) R[k] = Rn[k];
      for (int k = 0; k < 3; k++) t[k] = tn[k];
      cost = cn;
      steps++;
      lambda = lambda / 10.0;
      if (lambda < 1e-9) lambda = 1e-9;
    } else {
      rejected++;
      lambda = lambda * 10.0;
    }
  }
  const double rms = sqrt(cost / (double)(4 * n_tags));

  // ---- covariance: sigma^2 (J^T J)^-1 at the final pose, by the same Cholesky ----
  double cov[36];
  bool cov_ok = true;
  {
    double ag[27];
    rig_normal(tm, sh, &phase, n_cams, slots, cams, R, t, ag);
    const double s2 = cost / (double)(8 * n_tags - 6);
#pragma unroll
    for (int k = 0; k < 6; k++) {
      double rhs[6], x[6];
#pragma unroll
      for (int i = 0; i < 6; i++) rhs[i] = i == k ? -1.0 : -0.0;
      if (!fp_solve6(ag, rhs, 0.0, x)) cov_ok = false;
#pragma unroll
      for (int i = 0; i < 6; i++) cov[k * 6 + i] = s2 * x[i];
    }
  }

  // ---- the record ----
  if (tm.leader()) {
    for (int q = 0; q < 2; q++) {
      RigRecord* o = q ? out2 : out;
      if (!o) continue;
      o->n_tags = n_tags;
      o->n_cams_used = n_used;
      for (int i = 0; i < kRigMaxCams; i++) {
        const int mi = i < n_cams ? sh.m[i] : 0;
        o->tags_per_cam[i] = mi;
        for (int j = 0; j < kFpMaxTags; j++) o->ids[i][j] = j < mi ? sh.ids[i][j] : 0;
      }
      for (int i = 0; i < 9; i++) o->R[i] = R[i];
      for (int i = 0; i < 3; i++) o->t[i] = t[i];
#pragma unroll
      for (int i = 0; i < 36; i++) o->cov[i] = cov_ok ? cov[i] : 0.0;
      o->rms_px = rms;
      o->cov_valid = cov_ok ? 1 : 0;
      o->steps_taken = steps;
      o->rejected = rejected;
      o->dropped = dropped;
    }
  }
}

// Every slot of every camera held by one host thread.
struct RigHostTeam {
  static constexpr int NC = kRigMaxCams;
  static constexpr int NS = kFpSlots;
  int cam(int k) const { return k; }
  FpHostWave wave() const { return FpHostWave(); }
  bool wave_leader() const { return true; }
  bool leader() const { return true; }
  void barrier() const {}
  template <int N>
  void wave_sums(double (*vals)[N], double* row) const {
    for (int i = 0; i < N; i++) {
      double col[kFpSlots];
      for (int s = 0; s < kFpSlots; s++) col[s] = vals[s][i];
      row[i] = FpHostWave().sum(col);
    }
  }
  template <int N>
  void across(double (*rows)[kRigSums], int n_cams, double* out) const {
    for (int i = 0; i < N; i++) {
      double acc = rows[0][i];
      for (int c = 1; c < n_cams; c++) acc = acc + rows[c][i];
      out[i] = acc;
    }
  }
};

}  // namespace at
