// at_rigcal.h -- rig calibration: the camera -> robot extrinsics of a rig from N recorded
// instants, shared by host and device.
//
// A joint least-squares solve (bundle adjustment).  Unknowns: the robot's field pose at every
// instant (x_field = R x_robot + t) and the extrinsics (x_robot = E_R x_cam + E_t) of every
// camera parameter not held fixed.  Cost: the summed squared reprojection error in pixels of
// every selected layout-tag corner of every camera at every instant, projected as at_rigpose.h
// does (rig_point; Pz <= 0 costs HUGE_VAL).
//
// Parameters: per instant (w, dt) as rig_apply_step; per camera (we, de) with
// E_R' = E_R dR(we), E_t' = E_t + de, so dP/dwe = [P]x and dP/dde = -E_R^T.  A camera's
// free_rot / free_trans flags free we / de; a parameter that is not free has row and column
// zero, 1 on the diagonal and +0.0 on the right-hand side of the reduced system, and the
// rotation / translation it belongs to is copied, not multiplied.
//
// kCalIters Levenberg-Marquardt iterations, fixed, on the whole problem, by the Schur
// complement of the pose blocks.  With U, g the normal equations of an instant's pose, V_c, h_c
// those of camera c over that instant's corners and W_c = Jp^T Jc, an iteration is
//   accumulate  (cal_accum, per instant) the 90 sums of every camera over its 64 slots (the xor
//               tree of at_fieldpose.h), U and g added up in camera order; Y_c =
//               (U + lambda diag U)^-1 W_c and y = (U + lambda diag U)^-1 g column by column by
//               fp_solve6; the instant's part of the reduced system of size M = 6 n_cams:
//               S[6c+a][6c'+b] = [c == c'] V_c[a][b] - sum_k W_c[k][a] Y_c'[k][b]  (c <= c'),
//               rhs[6c+a] = h_c[a] - sum_k W_c[k][a] y[k], and the diagonal of V_c; k ascending;
//   sum         (cal_chunk_entry, cal_reduced) every entry over the instants: ascending within
//               chunks of kCalChunk, then the chunk sums in ascending order; an instant that
//               takes no part adds +0.0;
//   solve       (cal_reduced, one team) lambda times the summed V diagonal on the free diagonals,
//               Cholesky column by column, each entry (a - sum_k L[i][k] L[j][k]) / L[j][j] with
//               k ascending, forward and back substitution; a pivot that is not positive is a
//               failed factor: every step is zero and the iteration counts as rejected;
//   back        (cal_back, per instant) the pose step -(U + lambda diag U)^-1 (g + sum_c W_c dc_c),
//               both steps applied to the candidate copies, the candidate's cost;
//   decide      (cal_decide, one team) `cn < cost` takes the candidates (CalCtl::which flips) and
//               divides lambda by 10 (floor 1e-9), else lambda grows tenfold.
// The start is rig_solve_instant under the initial extrinsics per instant, over the stored tags
// presented as candidates (CalSrc); an instant that comes back with n_tags = 0 takes no part.
// The result's covariance blocks are sigma^2 times the diagonal blocks of S^-1, S the undamped
// reduced matrix at the final state, sigma^2 = cost / (2 corners - 6 instants_used - free
// parameters); rows and columns of parameters that are not free are zero.
//
// The kernels (at_kernels.hip: k_cal_*) and the CPU twin (at_rigcal.cpp) instantiate these
// functions with a team (at_rigpose.h's, plus first() / stride() for loops spread over the
// team's threads) over the same CalBufs, device or host pointers.  at_fieldpose.h's rules hold:
// no contraction, only + - * / sqrt, every sum in one stated order.
#pragma once

#include "at_rigpose.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define AT_CAL_M __host__ __device__
#else
#define AT_CAL_M
#endif

namespace at {

constexpr int kCalMaxInstants = 4096;  // AT_RIGCAL_MAX_INSTANTS
constexpr int kCalIters = 16;
constexpr int kCalChunk = 32;
constexpr int kCalMaxChunks = kCalMaxInstants / kCalChunk;
constexpr int kCalMaxParams = 6 * kRigMaxCams;
constexpr int kCalCamSums = 90;  // U 21, g 6 | V 21, h 6 | W 36 (row k of the pose, column b of the camera)

// one camera's selected tags at one instant, ascending ids
struct CalCamObs {
  int32_t m;
  int32_t pad;
  int32_t ids[kFpMaxTags];
  double p[kFpMaxTags][8];
  double pose_R[kFpMaxTags][9];
  double pose_t[kFpMaxTags][3];
};
static_assert(sizeof(CalCamObs) == 2632, "CalCamObs: 2632 B per camera and instant");

struct CalPose { double R[9]; double t[3]; };  // a robot pose, or a camera's extrinsics

struct CalCtl {
  double lambda, cost, cost0;
  int32_t which;       // the current state is pose[which], ext[which]; the candidate the other
  int32_t accepted, rejected;
  int32_t factor_ok;   // the last reduced solve had a Cholesky factor
  int32_t corners, used, cov_valid, pad;
};

struct CalBufs {
  const CalCamObs* obs;  // [N][n_cams]
  RigRecord* rec;        // [N] the start
  int32_t* ntags;        // [N] the start's n_tags: 0 takes no part
  CalPose* pose[2];      // [N]
  CalPose* ext[2];       // [n_cams]
  double* inst;          // [N][27 + 36 n_cams]: U, g, W_c
  double* part;          // [N][E] the instant's part of the reduced system, E = M M + 2 M
  double* chunk;         // [chunks][E]
  double* dc;            // [M] the cameras' step
  double* instcost;      // [N]
  double* cov;           // [n_cams][36]
  CalCtl* ctl;
  FpLayout lay;
  double tag_size;
  double fx[kRigMaxCams], fy[kRigMaxCams], cx[kRigMaxCams], cy[kRigMaxCams];
  int32_t free_rot[kRigMaxCams], free_trans[kRigMaxCams];
  int N, n_cams;
  AT_CAL_M int M() const { return 6 * n_cams; }
  AT_CAL_M int E() const { return M() * M() + 2 * M(); }
  AT_CAL_M int inst_len() const { return 27 + 36 * n_cams; }
  AT_CAL_M int chunks() const { return (N + kCalChunk - 1) / kCalChunk; }
  AT_CAL_M bool is_free(int p) const { return (p % 6 < 3 ? free_rot[p / 6] : free_trans[p / 6]) != 0; }
  AT_CAL_M RigCam rigcam(int c, const CalPose& e) const {
    RigCam r = {fx[c], fy[c], cx[c], cy[c], {}, {}};
    for (int k = 0; k < 9; k++) r.ER[k] = e.R[k];
    for (int k = 0; k < 3; k++) r.Et[k] = e.t[k];
    return r;
  }
};

// the stored tags of one camera as fp_select's / rig_solve_instant's candidates
struct CalCamSrc {
  const CalCamObs* o;
  AT_CAL_M int n() const { return o->m; }
  AT_CAL_M int32_t id(int c) const { return o->ids[c]; }
  AT_CAL_M int32_t hamming(int) const { return 0; }
  AT_CAL_M float margin(int) const { return 0.0f; }
  AT_CAL_M const double* p(int c) const { return o->p[c]; }
  AT_CAL_M const double* pose_R(int c) const { return o->pose_R[c]; }
  AT_CAL_M const double* pose_t(int c) const { return o->pose_t[c]; }
};
struct CalSrc {
  const CalBufs* b;
  int i;
  AT_CAL_M CalCamSrc cam(int c) const { return {b->obs + (size_t)i * b->n_cams + c}; }
  AT_CAL_M RigCam rigcam(int c) const { return b->rigcam(c, b->ext[0][c]); }
};

struct CalShared {
  double cs[kRigMaxCams][kCalCamSums];  // each camera's sums
  double U[27];                         // U, g over the cameras
  double Y[kRigMaxCams][36];            // Y_c[k][b]
  double y[6];
  double r[6];
};
struct CalSolveShared {
  double A[kCalMaxParams][kCalMaxParams];  // the reduced matrix (upper triangle); then one row per covariance column
  double L[kCalMaxParams][kCalMaxParams];
  double rhs[kCalMaxParams], vd[kCalMaxParams], y[kCalMaxParams], x[kCalMaxParams];
  double cc[kCalMaxChunks];
  int32_t ct[kCalMaxChunks], cu[kCalMaxChunks];
};

// E' = E moved by d = (we, de); a part that is not free is copied
AT_FP_HD void cal_apply_ext(const CalPose& e, const double* d, bool free_rot, bool free_trans, CalPose* o) {
  double Rn[9], tn[3];
  rig_apply_step(e.R, e.t, d, Rn, tn);
  for (int k = 0; k < 9; k++) o->R[k] = free_rot ? Rn[k] : e.R[k];
  for (int k = 0; k < 3; k++) o->t[k] = free_trans ? tn[k] : e.t[k];
}

// the slot's residual rows for the pose (jpu, jpv) and for its camera (jcu, jcv), and (ru, rv)
AT_FP_HD void cal_slot_rows(const FpSlot& s, const RigCam& cam, const double* R, const double* t, bool free_rot,
                            bool free_trans, double* jpu, double* jpv, double* jcu, double* jcv, double* ru,
                            double* rv) {
  double Q[3], P[3];
  rig_point(cam, R, t, s.X, Q, P);
  const double xn = P[0] / P[2], yn = P[1] / P[2];
  *ru = (cam.fx * xn + cam.cx) - s.u;
  *rv = (cam.fy * yn + cam.cy) - s.v;
  const double A = cam.fx / P[2], B = -(cam.fx * xn) / P[2];
  const double C = cam.fy / P[2], D = -(cam.fy * yn) / P[2];
  const double dQ[3][6] = {{0.0, -Q[2], Q[1], -R[0], -R[3], -R[6]},
                           {Q[2], 0.0, -Q[0], -R[1], -R[4], -R[7]},
                           {-Q[1], Q[0], 0.0, -R[2], -R[5], -R[8]}};
  // dP/dwe = [P]x, dP/dde = -E_R^T
  const double dP[3][6] = {{0.0, -P[2], P[1], -cam.ER[0], -cam.ER[3], -cam.ER[6]},
                           {P[2], 0.0, -P[0], -cam.ER[1], -cam.ER[4], -cam.ER[7]},
                           {-P[1], P[0], 0.0, -cam.ER[2], -cam.ER[5], -cam.ER[8]}};
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const double m0 = (cam.ER[0] * dQ[0][c] + cam.ER[3] * dQ[1][c]) + cam.ER[6] * dQ[2][c];
    const double m1 = (cam.ER[1] * dQ[0][c] + cam.ER[4] * dQ[1][c]) + cam.ER[7] * dQ[2][c];
    const double m2 = (cam.ER[2] * dQ[0][c] + cam.ER[5] * dQ[1][c]) + cam.ER[8] * dQ[2][c];
    jpu[c] = A * m0 + B * m2;
    jpv[c] = C * m1 + D * m2;
    const bool fr = c < 3 ? free_rot : free_trans;
    jcu[c] = fr ? A * dP[0][c] + B * dP[2][c] : 0.0;
    jcv[c] = fr ? C * dP[1][c] + D * dP[2][c] : 0.0;
  }
}

// pass 0: U, g (27 values); 1: V, h (27); 2: W rows 0..2 (18); 3: W rows 3..5 (18)
template <int PASS>
AT_FP_HD void cal_slot_pass(bool valid, const double* jpu, const double* jpv, const double* jcu, const double* jcv,
                            double ru, double rv, double* o) {
  constexpr int N = PASS < 2 ? 27 : 18;
  if (!valid) {
#pragma unroll
    for (int k = 0; k < N; k++) o[k] = 0.0;
    return;
  }
  if constexpr (PASS < 2) {
    const double* ju = PASS ? jcu : jpu;
    const double* jv = PASS ? jcv : jpv;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
      for (int j = i; j < 6; j++) o[fp_tri(i, j)] = ju[i] * ju[j] + jv[i] * jv[j];
      o[21 + i] = ju[i] * ru + jv[i] * rv;
    }
  } else {
    constexpr int k0 = PASS == 2 ? 0 : 3;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int b = 0; b < 6; b++) o[k * 6 + b] = jpu[k0 + k] * jcu[b] + jpv[k0 + k] * jcv[b];
  }
}
// one pass over the slots of a held camera: its sums into row
template <int PASS, class T>
AT_FP_HD void cal_pass(const T& tm, const FpSlot* slots, const double (*j)[26], double* row) {
  constexpr int N = PASS < 2 ? 27 : 18;
  double v[T::NS][N];
#pragma unroll
  for (int s = 0; s < T::NS; s++)
    cal_slot_pass<PASS>(slots[s].valid, j[s], j[s] + 6, j[s] + 12, j[s] + 18, j[s][24], j[s][25], v[s]);
  tm.template wave_sums<N>(v, row);
}

// the slots of held camera k (index ci) at instant i: the stored tags are the selection
template <class T>
AT_FP_HD void cal_slots(const T& tm, const CalBufs& b, int i, int ci, FpSlot* slots) {
  const CalCamSrc cs = {b.obs + (size_t)i * b.n_cams + ci};
  uint32_t my_cand[T::NS], my_id[T::NS];
  const int m = cs.n();
#pragma unroll
  for (int s = 0; s < T::NS; s++) {
    const int j = tm.wave().slot(s) >> 2;
    my_cand[s] = j < m ? (uint32_t)j : 0u;
    my_id[s] = j < m ? (uint32_t)cs.id(j) : 0u;
  }
  fp_points(tm.wave(), cs, b.lay, b.tag_size, m, my_cand, my_id, slots);
}

// ---- start: rig_solve_instant under the initial extrinsics ----
template <class T>
AT_FP_HD void cal_start(const T& tm, RigShared& sh, const CalBufs& b, int i) {
  const CalSrc src = {&b, i};
  rig_solve_instant(tm, src, sh, b.lay, b.n_cams, b.tag_size, b.rec + i, (RigRecord*)nullptr);
  if (tm.leader()) {
    const RigRecord& r = b.rec[i];
    b.ntags[i] = r.n_tags;
    for (int k = 0; k < 9; k++) b.pose[0][i].R[k] = r.R[k];
    for (int k = 0; k < 3; k++) b.pose[0][i].t[k] = r.t[k];
  }
}

// ---- accumulate and reduce: instant i's part of the reduced system ----
template <class T>
AT_FP_HD void cal_accum(const T& tm, CalShared& sh, const CalBufs& b, int i, bool final) {
  const int M = b.M(), E = b.E(), nc = b.n_cams;
  double* part = b.part + (size_t)i * E;
  if (b.ntags[i] <= 0) {
    for (int e = tm.first(); e < E; e += tm.stride()) part[e] = 0.0;
    return;
  }
  const int which = b.ctl->which;
  const double lambda = final ? 0.0 : b.ctl->lambda;
  const CalPose pose = b.pose[which][i];
  for (int k = 0; k < T::NC; k++) {
    const int ci = tm.cam(k);
    if (ci >= nc) continue;
    FpSlot slots[T::NS];
    cal_slots(tm, b, i, ci, slots);
    const RigCam cam = b.rigcam(ci, b.ext[which][ci]);
    const bool fr = b.free_rot[ci] != 0, ft = b.free_trans[ci] != 0;
    double j[T::NS][26];  // jpu, jpv, jcu, jcv, ru, rv
#pragma unroll
    for (int s = 0; s < T::NS; s++) {
#pragma unroll
      for (int q = 0; q < 26; q++) j[s][q] = 0.0;
      if (slots[s].valid)
        cal_slot_rows(slots[s], cam, pose.R, pose.t, fr, ft, j[s], j[s] + 6, j[s] + 12, j[s] + 18, &j[s][24], &j[s][25]);
    }
    cal_pass<0>(tm, slots, j, sh.cs[ci]);
    cal_pass<1>(tm, slots, j, sh.cs[ci] + 27);
    cal_pass<2>(tm, slots, j, sh.cs[ci] + 54);
    cal_pass<3>(tm, slots, j, sh.cs[ci] + 72);
  }
  tm.barrier();
  for (int e = tm.first(); e < 27; e += tm.stride()) {
    double acc = sh.cs[0][e];
    for (int c = 1; c < nc; c++) acc = acc + sh.cs[c][e];
    sh.U[e] = acc;
  }
  tm.barrier();
  for (int col = tm.first(); col <= M; col += tm.stride()) {
    double rhs[6], x[6];
    const int c = col / 6, bb = col % 6;
    for (int k = 0; k < 6; k++) rhs[k] = col < M ? -sh.cs[c][54 + 6 * k + bb] : -sh.U[21 + k];
    fp_solve6(sh.U, rhs, lambda, x);
    for (int k = 0; k < 6; k++) {
      if (col < M) sh.Y[c][6 * k + bb] = x[k];
      else sh.y[k] = x[k];
    }
  }
  tm.barrier();
  for (int e = tm.first(); e < E; e += tm.stride()) {
    double val = 0.0;
    if (e < M * M) {
      const int r = e / M, s = e % M, c = r / 6, a = r % 6, c2 = s / 6, bb = s % 6;
      if (c <= c2) {
        double acc = sh.cs[c][54 + a] * sh.Y[c2][bb];
        for (int k = 1; k < 6; k++) acc = acc + sh.cs[c][54 + 6 * k + a] * sh.Y[c2][6 * k + bb];
        const double v0 = c == c2 ? sh.cs[c][27 + (a <= bb ? fp_tri(a, bb) : fp_tri(bb, a))] : 0.0;
        val = v0 - acc;
      }
    } else if (e < M * M + M) {
      const int p = e - M * M, c = p / 6, a = p % 6;
      double acc = sh.cs[c][54 + a] * sh.y[0];
      for (int k = 1; k < 6; k++) acc = acc + sh.cs[c][54 + 6 * k + a] * sh.y[k];
      val = sh.cs[c][27 + 21 + a] - acc;
    } else {
      const int p = e - M * M - M, c = p / 6, a = p % 6;
      val = sh.cs[c][27 + fp_tri(a, a)];
    }
    part[e] = val;
  }
  double* inst = b.inst + (size_t)i * b.inst_len();
  for (int e = tm.first(); e < b.inst_len(); e += tm.stride())
    inst[e] = e < 27 ? sh.U[e] : sh.cs[(e - 27) / 36][54 + (e - 27) % 36];
}

// ---- entry e of chunk ch: its instants in ascending order ----
AT_FP_HD void cal_chunk_entry(const CalBufs& b, int ch, int e) {
  const int E = b.E(), i0 = ch * kCalChunk, i1 = i0 + kCalChunk < b.N ? i0 + kCalChunk : b.N;
  double acc = b.part[(size_t)i0 * E + e];
  for (int i = i0 + 1; i < i1; i++) acc = acc + b.part[(size_t)i * E + e];
  b.chunk[(size_t)ch * E + e] = acc;
}

// ---- the reduced solve (one team).  final: the undamped matrix and its inverse's blocks ----
template <class T>
AT_FP_HD void cal_reduced(const T& tm, CalSolveShared& sh, const CalBufs& b, bool final) {
  const int M = b.M(), E = b.E(), nch = b.chunks();
  const double lambda = b.ctl->lambda;
  const int which = b.ctl->which;
  for (int e = tm.first(); e < E; e += tm.stride()) {
    double acc = b.chunk[e];
    for (int ch = 1; ch < nch; ch++) acc = acc + b.chunk[(size_t)ch * E + e];
    if (e < M * M) sh.A[e / M][e % M] = acc;
    else if (e < M * M + M) sh.rhs[e - M * M] = acc;
    else sh.vd[e - M * M - M] = acc;
  }
  tm.barrier();
  for (int e = tm.first(); e < M * M; e += tm.stride()) {
    const int r = e / M, s = e % M;
    if (r > s) continue;
    double a = sh.A[r][s];
    if (!b.is_free(r) || !b.is_free(s)) a = r == s ? 1.0 : 0.0;
    else if (r == s && !final) a = a + lambda * sh.vd[r];
    sh.A[r][s] = a;
  }
  tm.barrier();
  bool ok = true;
  for (int j = 0; j < M; j++) {
    double s = sh.A[j][j];
    for (int k = 0; k < j; k++) s = s - sh.L[j][k] * sh.L[j][k];
    if (!(s > 0.0)) ok = false;
    const double ljj = sqrt(s);
    for (int i = j + tm.first(); i < M; i += tm.stride()) {
      if (i == j) {
        sh.L[j][j] = ljj;
        continue;
      }
      double v = sh.A[j][i];
      for (int k = 0; k < j; k++) v = v - sh.L[i][k] * sh.L[j][k];
      sh.L[i][j] = v / ljj;
    }
    tm.barrier();
  }
  if (!final) {
    if (tm.leader()) {
      for (int i = 0; i < M; i++) {
        double v = b.is_free(i) ? -sh.rhs[i] : 0.0;
        for (int k = 0; k < i; k++) v = v - sh.L[i][k] * sh.y[k];
        sh.y[i] = v / sh.L[i][i];
      }
      for (int i = M - 1; i >= 0; i--) {
        double v = sh.y[i];
        for (int k = i + 1; k < M; k++) v = v - sh.L[k][i] * sh.x[k];
        sh.x[i] = v / sh.L[i][i];
      }
      for (int i = 0; i < M; i++) {
        const double d = ok && b.is_free(i) ? sh.x[i] : 0.0;
        sh.x[i] = d;
        b.dc[i] = d;
      }
      b.ctl->factor_ok = ok ? 1 : 0;
    }
    tm.barrier();
    for (int c = tm.first(); c < b.n_cams; c += tm.stride())
      cal_apply_ext(b.ext[which][c], sh.x + 6 * c, b.free_rot[c] != 0, b.free_trans[c] != 0, &b.ext[which ^ 1][c]);
    return;
  }
  // column p of S^-1 in row p of A: forward, then back in place
  int den = 2 * b.ctl->corners - 6 * b.ctl->used;
  for (int p = 0; p < M; p++) den -= b.is_free(p) ? 1 : 0;
  const bool valid = ok && den > 0;
  const double s2 = b.ctl->cost / (double)den;
  for (int p = tm.first(); p < M; p += tm.stride()) {
    double* w = sh.A[p];
    for (int i = 0; i < M; i++) {
      double v = i == p ? 1.0 : 0.0;
      for (int k = 0; k < i; k++) v = v - sh.L[i][k] * w[k];
      w[i] = v / sh.L[i][i];
    }
    for (int i = M - 1; i >= 0; i--) {
      double v = w[i];
      for (int k = i + 1; k < M; k++) v = v - sh.L[k][i] * w[k];
      w[i] = v / sh.L[i][i];
    }
    const int c = p / 6, a = p % 6;
    for (int bb = 0; bb < 6; bb++)
      b.cov[c * 36 + a * 6 + bb] = valid && b.is_free(p) && b.is_free(6 * c + bb) ? s2 * w[6 * c + bb] : 0.0;
  }
  if (tm.leader()) b.ctl->cov_valid = valid ? 1 : 0;
}

// ---- back substitution and the candidate's cost (step), or the current state's cost ----
template <class T>
AT_FP_HD void cal_back(const T& tm, CalShared& sh, const CalBufs& b, int i, bool step) {
  if (b.ntags[i] <= 0) {
    if (tm.leader()) b.instcost[i] = 0.0;
    return;
  }
  const int nc = b.n_cams;
  const int which = b.ctl->which, st = step ? which ^ 1 : which;
  CalPose pose = b.pose[which][i];
  if (step) {
    const double* inst = b.inst + (size_t)i * b.inst_len();
    for (int k = tm.first(); k < 6; k += tm.stride()) {
      double acc = inst[21 + k];
      for (int c = 0; c < nc; c++)
        for (int bb = 0; bb < 6; bb++) acc = acc + inst[27 + 36 * c + 6 * k + bb] * b.dc[6 * c + bb];
      sh.r[k] = acc;
    }
    tm.barrier();
    double U[21], d[6];
    for (int k = 0; k < 21; k++) U[k] = inst[k];
    const bool ok = fp_solve6(U, sh.r, b.ctl->lambda, d);
    if (!ok || !b.ctl->factor_ok)
      for (int k = 0; k < 6; k++) d[k] = 0.0;
    CalPose pn;
    rig_apply_step(pose.R, pose.t, d, pn.R, pn.t);
    pose = pn;
    if (tm.leader()) b.pose[st][i] = pn;
  }
  for (int k = 0; k < T::NC; k++) {
    const int ci = tm.cam(k);
    if (ci >= nc) continue;
    FpSlot slots[T::NS];
    cal_slots(tm, b, i, ci, slots);
    const RigCam cam = b.rigcam(ci, b.ext[st][ci]);
    double e[T::NS][1];
#pragma unroll
    for (int s = 0; s < T::NS; s++) e[s][0] = rig_slot_cost(slots[s], cam, pose.R, pose.t);
    tm.template wave_sums<1>(e, sh.cs[ci]);
  }
  tm.barrier();
  if (tm.leader()) {
    double acc = sh.cs[0][0];
    for (int c = 1; c < nc; c++) acc = acc + sh.cs[c][0];
    b.instcost[i] = acc;
  }
}

// ---- the total cost in chunk order, and what follows from it (one team) ----
// step: accept or reject the candidate; else: the start's cost and counts
template <class T>
AT_FP_HD void cal_decide(const T& tm, CalSolveShared& sh, const CalBufs& b, bool step) {
  const int nch = b.chunks();
  for (int ch = tm.first(); ch < nch; ch += tm.stride()) {
    const int i0 = ch * kCalChunk, i1 = i0 + kCalChunk < b.N ? i0 + kCalChunk : b.N;
    double acc = b.instcost[i0];
    int tags = b.ntags[i0], used = b.ntags[i0] > 0;
    for (int i = i0 + 1; i < i1; i++) {
      acc = acc + b.instcost[i];
      tags += b.ntags[i];
      used += b.ntags[i] > 0;
    }
    sh.cc[ch] = acc;
    sh.ct[ch] = tags;
    sh.cu[ch] = used;
  }
  tm.barrier();
  if (!tm.leader()) return;
  double cn = sh.cc[0];
  int tags = sh.ct[0], used = sh.cu[0];
  for (int ch = 1; ch < nch; ch++) {
    cn = cn + sh.cc[ch];
    tags += sh.ct[ch];
    used += sh.cu[ch];
  }
  CalCtl& c = *b.ctl;
  if (!step) {
    c.lambda = 1e-3;
    c.cost = c.cost0 = cn;
    c.which = 0;
    c.accepted = c.rejected = 0;
    c.factor_ok = 0;
    c.corners = 4 * tags;
    c.used = used;
    c.cov_valid = 0;
    return;
  }
  if (c.factor_ok && cn < c.cost) {
    c.which ^= 1;
    c.cost = cn;
    c.accepted++;
    c.lambda = c.lambda / 10.0;
    if (c.lambda < 1e-9) c.lambda = 1e-9;
  } else {
    c.rejected++;
    c.lambda = c.lambda * 10.0;
  }
}

// Every slot of every camera held by one host thread.
struct CalHostTeam : RigHostTeam {
  int first() const { return 0; }
  int stride() const { return 1; }
};

}  // namespace at

// ---- the calibrator's host side (at_rigcal.cpp; at_api.cpp adds the device buffers) ----
#include <vector>

#include "../../include/at_api.h"

namespace at {
struct CalGpu;  // at_api.cpp
}
struct at_rigcal {
  int n_cams;
  int max_hamming;
  double tag_size;
  at_rigcal_camera cams[at::kRigMaxCams];
  std::vector<int16_t> lut;
  std::vector<at::FpTag> tags;
  std::vector<at::CalCamObs> obs;  // [N][n_cams]
  int n;                           // stored instants
  bool obs_dirty;                  // the device copy of obs is stale
  // the last solve
  at_rigcal_result result;
  std::vector<at_rigcal_instant> instants;
  uint64_t ns;
  int profiling;
  at::CalGpu* gpu;
  void (*gpu_free)(at::CalGpu*);
};
namespace at {
// the parts of CalBufs that do not depend on where the buffers live
void cal_fill_bufs(const at_rigcal& c, CalBufs* b);
// the records of a finished solve from its final buffers (host copies)
void cal_finish(at_rigcal* c, const CalCtl& ctl, const CalPose* ext, const double* cov, const CalPose* pose,
                const double* instcost, const int32_t* ntags, at_rigcal_result* out);
}  // namespace at
