// at_camcal.h -- camera calibration: the intrinsics and distortion of one camera from N stored
// views of a board of tags, shared by host and device.
//
// A joint least-squares solve.  Unknowns: the board's pose in every view (x_cam = R x_board + t)
// and the entries of (fx, fy, cx, cy, k1, k2, p1, p2, k3) that free_mask selects (bit p frees
// parameter p in that order).  Cost: the summed squared error in pixels of every stored corner
// under the detector's own forward model (cc_distort):
//   P = R X + t,  x = Px / Pz,  y = Py / Pz,  r2 = x x + y y,
//   lin = 1 + k1 r2 + k2 r2^2 + k3 r2^3,
//   x'' = x lin + 2 p1 x y + p2 (r2 + 2 x x),  y'' = y lin + p1 (r2 + 2 y y) + 2 p2 x y,
//   u = fx x'' + cx,  v = fy y'' + cy;   Pz <= 0 costs HUGE_VAL.
// The corners must be raw pixels: record views with the detector's distortion set to zero.
//
// Start.  Each stored tag's homography H (tag [-1, 1]^2 -> pixels) under the start intrinsics gives
// cam_T_tag (cc_h_pose): a_k = K^-1 h_k, s = sqrt(|a_1| |a_2|) signed so that t_z > 0, r_1 = a_1 / s,
// r_2 = a_2 / s, r_3 = r_1 x r_2, t = (a_3 / s) tag_size / 2; cam_T_board = cam_T_tag
// (board_T_tag)^-1.  The candidate (ascending id) with the least cost over all the view's corners,
// the first among equals, is made orthonormal by fp_project_rotation; a view whose candidates all
// have a corner at Pz <= 0 takes no part (ntags = 0).
//
// Parameters: per view (w, dt) as fp_apply_step (R' = dR(w) R, t' = t + dt), so dP/dw = -[R X]x
// and dP/dt = I; the intrinsics step is additive.  A parameter that is not free has zero Jacobian
// columns, 1 on the diagonal and +0.0 on the right-hand side of the reduced system, and its value
// is copied.
//
// kCcIters Levenberg-Marquardt iterations, fixed, on the whole problem, by the Schur complement of
// the pose blocks.  With U, g the normal equations of a view's pose, V, h those of the intrinsics
// over that view's corners and W = Jp^T Ji (6 x 9), an iteration is
//   accumulate  (cc_accum, per view) the 135 sums over the view's 64 slots (the xor tree of
//               at_fieldpose.h) in five passes of 27; Y = (U + lambda diag U)^-1 W and
//               y = (U + lambda diag U)^-1 g column by column by fp_solve6; the view's part of the
//               reduced system: S[a][b] = V[a][b] - sum_k W[k][a] Y[k][b] (a <= b),
//               rhs[a] = h[a] - sum_k W[k][a] y[k], and the diagonal of V; k ascending;
//   sum         (cc_chunk_entry, cc_reduced) every entry over the views: ascending within chunks of
//               kCcChunk, then the chunk sums in ascending order; a view that takes no part adds +0.0;
//   solve       (cc_reduced, one team) lambda times the summed V diagonal on the free diagonals,
//               Cholesky column by column, each entry (a - sum_k L[i][k] L[j][k]) / L[j][j] with k
//               ascending, forward and back substitution; a pivot that is not positive is a failed
//               factor: every step is zero and the iteration counts as rejected;
//   back        (cc_back, per view) the pose step -(U + lambda diag U)^-1 (g + W dc), both steps
//               applied to the candidate copies, the candidate's cost;
//   decide      (cc_decide, one team) `cn < cost` takes the candidates (CalCtl::which flips) and
//               divides lambda by 10 (floor 1e-9), else lambda grows tenfold.  A corner at Pz <= 0
//               makes cn infinite, so the one comparison is the whole accept rule.
// The covariance is sigma^2 times the inverse of the undamped reduced matrix at the final state,
// sigma^2 = cost / (2 corners - 6 views_used - free parameters); rows and columns of parameters
// that are not free are zero.
//
// Focal guess (cc_focal_guess, host, at solve time): Zhang's two constraints per tag plane with
// the principal point c = (width / 2, height / 2) and zero skew.  For H' = T(-c) H with columns
// h1 = (x1, y1, z1), h2 = (x2, y2, z2), both divided by q = sqrt(sqrt(x1 x1 + y1 y1) sqrt(x2 x2 +
// y2 y2)) (the row scaling: pixel parts of unit size, so every tag weighs the same whatever the
// scale of its H), the rows (x1 x2, y1 y2 | -z1 z2) and (x1 x1 - x2 x2, y1 y1 - y2 y2 |
// -(z1 z1 - z2 z2)) are linear in (a, b) = (1 / fx^2, 1 / fy^2); their 2 x 2 normal equations are
// added over all stored tags, ascending by view then by id, and solved by Cramer's rule.
//
// The kernels (at_kernels.hip: k_cc_*) and the CPU twin (at_camcal.cpp) instantiate these
// functions with a team over the same CcBufs, device or host pointers.  at_fieldpose.h's rules
// hold: no contraction, only + - * / sqrt, every sum in one stated order.
#pragma once

#include "at_rigcal.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace at {

constexpr int kCcMaxViews = 4096;  // AT_CAMCAL_MAX_VIEWS
constexpr int kCcIters = 30;
constexpr int kCcChunk = 32;
constexpr int kCcMaxChunks = kCcMaxViews / kCcChunk;
constexpr int kCcP = 9;                       // intrinsics
constexpr int kCcE = kCcP * kCcP + 2 * kCcP;  // a view's part: S (81), rhs (9), diag V (9)
constexpr int kCcViewLen = 27 + 54;           // what cc_back reads again: U, g, W
constexpr int kCcSums = 135;                  // U 21, g 6 | V 45, h 9 | W 54 (row k of the pose, column b)
constexpr int kCcV = 27, kCcH = 72, kCcW = 81;

// one view's selected tags, ascending ids
struct CcObs {
  int32_t m;
  int32_t pad;
  int32_t ids[kFpMaxTags];
  double p[kFpMaxTags][8];
  double H[kFpMaxTags][9];
};
static_assert(sizeof(CcObs) == 2248, "CcObs: 2248 B per view");

struct CcCam { double v[kCcP]; };  // fx, fy, cx, cy, k1, k2, p1, p2, k3

struct CcBufs {
  const CcObs* obs;   // [N]
  int32_t* ntags;     // [N] the start's tag count: 0 takes no part
  CalPose* pose[2];   // [N]
  CcCam* cam[2];      // [1]
  double* view;       // [N][kCcViewLen]
  double* part;       // [N][kCcE]
  double* chunk;      // [chunks][kCcE]
  double* dc;         // [9] the intrinsics' step
  double* viewcost;   // [N]
  double* cov;        // [81]
  CalCtl* ctl;        // (instants -> views)
  FpLayout lay;
  double tag_size;
  int32_t free_mask;
  int N;
  AT_CAL_M int chunks() const { return (N + kCcChunk - 1) / kCcChunk; }
  AT_CAL_M bool is_free(int p) const { return ((free_mask >> p) & 1) != 0; }
};

struct CcSrc {
  const CcObs* o;
  AT_CAL_M const double* p(int c) const { return o->p[c]; }
};

struct CcShared {
  double cs[kCcSums];
  double Y[6][kCcP];
  double y[6];
  double r[6];
  double cand[kFpMaxTags];
};
struct CcSolveShared {
  double A[kCcP][kCcP];  // the reduced matrix (upper triangle); then one row per covariance column
  double L[kCcP][kCcP];
  double rhs[kCcP], vd[kCcP], y[kCcP], x[kCcP];
  double cc[kCcMaxChunks];
  int32_t ct[kCcMaxChunks], cu[kCcMaxChunks];
};

AT_FP_HD constexpr int cc_tri(int i, int j) { return i * kCcP - i * (i - 1) / 2 + (j - i); }

// the forward model from the normalised point on: (x'', y'')
AT_FP_HD void cc_distort(const double* c, double x, double y, double* xd, double* yd) {
  const double xx = x * x, yy = y * y, xy = x * y;
  const double r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2;
  const double lin = ((1.0 + c[4] * r2) + c[5] * r4) + c[8] * r6;
  *xd = (x * lin + 2.0 * c[6] * xy) + c[7] * (r2 + 2.0 * xx);
  *yd = (y * lin + c[6] * (r2 + 2.0 * yy)) + 2.0 * c[7] * xy;
}

// squared reprojection error of one slot under (R, t); HUGE_VAL with its Z not positive
AT_FP_HD double cc_slot_cost(const FpSlot& s, const double* c, const double* R, const double* t) {
  if (!s.valid) return 0.0;
  double Q[3];
  fp_rot(R, s.X, Q);
  const double Px = Q[0] + t[0], Py = Q[1] + t[1], Pz = Q[2] + t[2];
  if (!(Pz > 0.0)) return HUGE_VAL;
  double xd, yd;
  cc_distort(c, Px / Pz, Py / Pz, &xd, &yd);
  const double ru = (c[0] * xd + c[2]) - s.u;
  const double rv = (c[1] * yd + c[3]) - s.v;
  return ru * ru + rv * rv;
}

// the slot's two residual rows in j[32]: the pose's (jpu 0..5, jpv 6..11), the intrinsics'
// (jiu 12..20, jiv 21..29; 0 where not free) and (ru, rv) at 30, 31
AT_FP_HD void cc_slot_rows(const FpSlot& s, const double* c, int free_mask, const double* R, const double* t,
                           double* j) {
  double Q[3];
  fp_rot(R, s.X, Q);
  const double Px = Q[0] + t[0], Py = Q[1] + t[1], Pz = Q[2] + t[2];
  const double x = Px / Pz, y = Py / Pz;
  const double xx = x * x, yy = y * y, xy = x * y;
  const double r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2;
  const double lin = ((1.0 + c[4] * r2) + c[5] * r4) + c[8] * r6;
  const double xd = (x * lin + 2.0 * c[6] * xy) + c[7] * (r2 + 2.0 * xx);
  const double yd = (y * lin + c[6] * (r2 + 2.0 * yy)) + 2.0 * c[7] * xy;
  j[30] = (c[0] * xd + c[2]) - s.u;
  j[31] = (c[1] * yd + c[3]) - s.v;
  // d(x'', y'') / d(x, y); dl = d lin / d r2
  const double dl = (c[4] + 2.0 * c[5] * r2) + 3.0 * c[8] * r4;
  const double dxx = ((lin + 2.0 * xx * dl) + 2.0 * c[6] * y) + 6.0 * c[7] * x;
  const double dxy = (2.0 * xy * dl + 2.0 * c[6] * x) + 2.0 * c[7] * y;
  const double dyy = ((lin + 2.0 * yy * dl) + 6.0 * c[6] * y) + 2.0 * c[7] * x;
  // du/dP = (A0, A1, A2), dv/dP = (B0, B1, B2)
  const double A0 = c[0] * dxx / Pz, A1 = c[0] * dxy / Pz, A2 = -(A0 * x + A1 * y);
  const double B0 = c[1] * dxy / Pz, B1 = c[1] * dyy / Pz, B2 = -(B0 * x + B1 * y);
  // dP/dw = -[Q]x, dP/dt = I
  j[0] = A2 * Q[1] - A1 * Q[2];
  j[1] = A0 * Q[2] - A2 * Q[0];
  j[2] = A1 * Q[0] - A0 * Q[1];
  j[3] = A0;
  j[4] = A1;
  j[5] = A2;
  j[6] = B2 * Q[1] - B1 * Q[2];
  j[7] = B0 * Q[2] - B2 * Q[0];
  j[8] = B1 * Q[0] - B0 * Q[1];
  j[9] = B0;
  j[10] = B1;
  j[11] = B2;
  const double iu[kCcP] = {xd, 0.0, 1.0, 0.0, c[0] * (x * r2), c[0] * (x * r4), c[0] * (2.0 * xy),
                           c[0] * (r2 + 2.0 * xx), c[0] * (x * r6)};
  const double iv[kCcP] = {0.0, yd, 0.0, 1.0, c[1] * (y * r2), c[1] * (y * r4), c[1] * (r2 + 2.0 * yy),
                           c[1] * (2.0 * xy), c[1] * (y * r6)};
#pragma unroll
  for (int p = 0; p < kCcP; p++) {
    const bool fr = ((free_mask >> p) & 1) != 0;
    j[12 + p] = fr ? iu[p] : 0.0;
    j[21 + p] = fr ? iv[p] : 0.0;
  }
}

// 27 of the 135 sums per pass.  0: U, g; 1: V entries 0..26; 2: V entries 27..44, then h;
// 3: W rows 0..2; 4: W rows 3..5
template <int PASS>
AT_FP_HD void cc_slot_pass(bool valid, const double* j, double* o) {
  if (!valid) {
#pragma unroll
    for (int k = 0; k < 27; k++) o[k] = 0.0;
    return;
  }
  const double *jpu = j, *jpv = j + 6, *jiu = j + 12, *jiv = j + 21;
  const double ru = j[30], rv = j[31];
  if constexpr (PASS == 0) {
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
      for (int k = i; k < 6; k++) o[fp_tri(i, k)] = jpu[i] * jpu[k] + jpv[i] * jpv[k];
      o[21 + i] = jpu[i] * ru + jpv[i] * rv;
    }
  } else if constexpr (PASS == 1 || PASS == 2) {
    constexpr int base = PASS == 1 ? 0 : 27, end = PASS == 1 ? 27 : 45;
#pragma unroll
    for (int i = 0; i < kCcP; i++) {
#pragma unroll
      for (int k = i; k < kCcP; k++) {
        const int e = cc_tri(i, k);
        if (e >= base && e < end) o[e - base] = jiu[i] * jiu[k] + jiv[i] * jiv[k];
      }
      if constexpr (PASS == 2) o[18 + i] = jiu[i] * ru + jiv[i] * rv;
    }
  } else {
    constexpr int k0 = PASS == 3 ? 0 : 3;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int b = 0; b < kCcP; b++) o[k * kCcP + b] = jpu[k0 + k] * jiu[b] + jpv[k0 + k] * jiv[b];
  }
}
template <int PASS, class T>
AT_FP_HD void cc_pass(const T& tm, const FpSlot* slots, const double (*j)[32], double* row) {
  double v[T::NS][27];
#pragma unroll
  for (int s = 0; s < T::NS; s++) cc_slot_pass<PASS>(slots[s].valid, j[s], v[s]);
  tm.template wave_sums<27>(v, row);
}

// the slots of view i: the stored tags are the selection
template <class T>
AT_FP_HD void cc_slots(const T& tm, const CcBufs& b, int i, FpSlot* slots) {
  const CcObs* o = b.obs + i;
  const CcSrc cs = {o};
  uint32_t my_cand[T::NS], my_id[T::NS];
  const int m = o->m;
#pragma unroll
  for (int s = 0; s < T::NS; s++) {
    const int j = tm.wave().slot(s) >> 2;
    my_cand[s] = j < m ? (uint32_t)j : 0u;
    my_id[s] = j < m ? (uint32_t)o->ids[j] : 0u;
  }
  fp_points(tm.wave(), cs, b.lay, b.tag_size, m, my_cand, my_id, slots);
}

// cam_T_tag from the tag's homography under (fx, fy, cx, cy) = c[0..3]
AT_FP_HD void cc_h_pose(const double* H, const double* c, double hs, double* R, double* t) {
  double a[3][3];  // a[k] = K^-1 h_(k+1)
#pragma unroll
  for (int k = 0; k < 3; k++) {
    a[k][0] = (H[k] - c[2] * H[6 + k]) / c[0];
    a[k][1] = (H[3 + k] - c[3] * H[6 + k]) / c[1];
    a[k][2] = H[6 + k];
  }
  const double n1 = sqrt((a[0][0] * a[0][0] + a[0][1] * a[0][1]) + a[0][2] * a[0][2]);
  const double n2 = sqrt((a[1][0] * a[1][0] + a[1][1] * a[1][1]) + a[1][2] * a[1][2]);
  double s = sqrt(n1 * n2);
  if (a[2][2] < 0.0) s = -s;
  double r1[3], r2[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    r1[k] = a[0][k] / s;
    r2[k] = a[1][k] / s;
    t[k] = (a[2][k] / s) * hs;
  }
  const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    R[k * 3] = r1[k];
    R[k * 3 + 1] = r2[k];
    R[k * 3 + 2] = r3[k];
  }
}
// candidate j of a view: cam_T_board = cam_T_tag (board_T_tag)^-1
AT_FP_HD void cc_candidate(const CcBufs& b, const CcObs& o, int j, const double* c, double* R, double* t) {
  double Rt[9], tt[3], rt[3];
  cc_h_pose(o.H[j], c, b.tag_size / 2.0, Rt, tt);
  const FpTag& tg = b.lay.tags[b.lay.lut[o.ids[j]]];
  fp_mul_abt(Rt, tg.R, R);
  fp_rot(R, tg.t, rt);
  for (int k = 0; k < 3; k++) t[k] = tt[k] - rt[k];
}

// ---- start: the best single-tag board pose of view i under the start intrinsics ----
template <class T>
AT_FP_HD void cc_start(const T& tm, CcShared& sh, const CcBufs& b, int i) {
  const CcObs& o = b.obs[i];
  const int m = o.m;
  const CcCam cam = b.cam[0][0];
  FpSlot slots[T::NS];
  cc_slots(tm, b, i, slots);
  for (int j = 0; j < m; j++) {
    double Rj[9], tj[3];
    cc_candidate(b, o, j, cam.v, Rj, tj);
    double e[T::NS][1];
#pragma unroll
    for (int s = 0; s < T::NS; s++) e[s][0] = cc_slot_cost(slots[s], cam.v, Rj, tj);
    tm.template wave_sums<1>(e, sh.cand + j);
  }
  tm.barrier();
  if (!tm.leader()) return;
  double cost = HUGE_VAL;
  int best = -1;
  for (int j = 0; j < m; j++)
    if (sh.cand[j] < cost) {  // (a NaN or an infinite cost never wins; ties stay with the lower id)
      cost = sh.cand[j];
      best = j;
    }
  CalPose p = {};
  if (best >= 0) {
    cc_candidate(b, o, best, cam.v, p.R, p.t);
    fp_project_rotation(p.R);
  }
  b.ntags[i] = best >= 0 ? m : 0;
  b.pose[0][i] = p;
  b.pose[1][i] = p;
}

// ---- accumulate and reduce: view i's part of the reduced system ----
template <class T>
AT_FP_HD void cc_accum(const T& tm, CcShared& sh, const CcBufs& b, int i, bool final) {
  double* part = b.part + (size_t)i * kCcE;
  if (b.ntags[i] <= 0) {
    for (int e = tm.first(); e < kCcE; e += tm.stride()) part[e] = 0.0;
    return;
  }
  const int which = b.ctl->which;
  const double lambda = final ? 0.0 : b.ctl->lambda;
  const CalPose pose = b.pose[which][i];
  const CcCam cam = b.cam[which][0];
  {
    FpSlot slots[T::NS];
    cc_slots(tm, b, i, slots);
    double j[T::NS][32];
#pragma unroll
    for (int s = 0; s < T::NS; s++) {
#pragma unroll
      for (int q = 0; q < 32; q++) j[s][q] = 0.0;
      if (slots[s].valid) cc_slot_rows(slots[s], cam.v, b.free_mask, pose.R, pose.t, j[s]);
    }
    cc_pass<0>(tm, slots, j, sh.cs);
    cc_pass<1>(tm, slots, j, sh.cs + 27);
    cc_pass<2>(tm, slots, j, sh.cs + 54);
    cc_pass<3>(tm, slots, j, sh.cs + 81);
    cc_pass<4>(tm, slots, j, sh.cs + 108);
  }
  tm.barrier();
  for (int col = tm.first(); col <= kCcP; col += tm.stride()) {
    double rhs[6], x[6];
    for (int k = 0; k < 6; k++) rhs[k] = col < kCcP ? -sh.cs[kCcW + kCcP * k + col] : -sh.cs[21 + k];
    fp_solve6(sh.cs, rhs, lambda, x);
    for (int k = 0; k < 6; k++) {
      if (col < kCcP) sh.Y[k][col] = x[k];
      else sh.y[k] = x[k];
    }
  }
  tm.barrier();
  for (int e = tm.first(); e < kCcE; e += tm.stride()) {
    double val = 0.0;
    if (e < kCcP * kCcP) {
      const int r = e / kCcP, s = e % kCcP;
      if (r <= s) {
        double acc = sh.cs[kCcW + r] * sh.Y[0][s];
        for (int k = 1; k < 6; k++) acc = acc + sh.cs[kCcW + kCcP * k + r] * sh.Y[k][s];
        val = sh.cs[kCcV + cc_tri(r, s)] - acc;
      }
    } else if (e < kCcP * kCcP + kCcP) {
      const int a = e - kCcP * kCcP;
      double acc = sh.cs[kCcW + a] * sh.y[0];
      for (int k = 1; k < 6; k++) acc = acc + sh.cs[kCcW + kCcP * k + a] * sh.y[k];
      val = sh.cs[kCcH + a] - acc;
    } else {
      const int a = e - kCcP * kCcP - kCcP;
      val = sh.cs[kCcV + cc_tri(a, a)];
    }
    part[e] = val;
  }
  double* view = b.view + (size_t)i * kCcViewLen;
  for (int e = tm.first(); e < kCcViewLen; e += tm.stride()) view[e] = e < 27 ? sh.cs[e] : sh.cs[kCcW + (e - 27)];
}

// ---- entry e of chunk ch: its views in ascending order ----
AT_FP_HD void cc_chunk_entry(const CcBufs& b, int ch, int e) {
  const int i0 = ch * kCcChunk, i1 = i0 + kCcChunk < b.N ? i0 + kCcChunk : b.N;
  double acc = b.part[(size_t)i0 * kCcE + e];
  for (int i = i0 + 1; i < i1; i++) acc = acc + b.part[(size_t)i * kCcE + e];
  b.chunk[(size_t)ch * kCcE + e] = acc;
}

// ---- the reduced solve (one team).  final: the undamped matrix and its inverse ----
template <class T>
AT_FP_HD void cc_reduced(const T& tm, CcSolveShared& sh, const CcBufs& b, bool final) {
  constexpr int M = kCcP;
  const int nch = b.chunks();
  const double lambda = b.ctl->lambda;
  const int which = b.ctl->which;
  for (int e = tm.first(); e < kCcE; e += tm.stride()) {
    double acc = b.chunk[e];
    for (int ch = 1; ch < nch; ch++) acc = acc + b.chunk[(size_t)ch * kCcE + e];
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
      const CcCam cur = b.cam[which][0];
      CcCam next;
      for (int i = 0; i < M; i++) {
        const double d = ok && b.is_free(i) ? sh.x[i] : 0.0;
        b.dc[i] = d;
        next.v[i] = b.is_free(i) ? cur.v[i] + d : cur.v[i];
      }
      b.cam[which ^ 1][0] = next;
      b.ctl->factor_ok = ok ? 1 : 0;
    }
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
    for (int q = 0; q < M; q++) b.cov[p * M + q] = valid && b.is_free(p) && b.is_free(q) ? s2 * w[q] : 0.0;
  }
  if (tm.leader()) b.ctl->cov_valid = valid ? 1 : 0;
}

// ---- back substitution and the candidate's cost (step), or the current state's cost ----
template <class T>
AT_FP_HD void cc_back(const T& tm, CcShared& sh, const CcBufs& b, int i, bool step) {
  if (b.ntags[i] <= 0) {
    if (tm.leader()) b.viewcost[i] = 0.0;
    return;
  }
  const int which = b.ctl->which, st = step ? which ^ 1 : which;
  CalPose pose = b.pose[which][i];
  if (step) {
    const double* view = b.view + (size_t)i * kCcViewLen;
    for (int k = tm.first(); k < 6; k += tm.stride()) {
      double acc = view[21 + k];
      for (int q = 0; q < kCcP; q++) acc = acc + view[27 + kCcP * k + q] * b.dc[q];
      sh.r[k] = acc;
    }
    tm.barrier();
    double U[21], d[6];
    for (int k = 0; k < 21; k++) U[k] = view[k];
    const bool ok = fp_solve6(U, sh.r, b.ctl->lambda, d);
    if (!ok || !b.ctl->factor_ok)
      for (int k = 0; k < 6; k++) d[k] = 0.0;
    CalPose pn;
    fp_apply_step(pose.R, pose.t, d, pn.R, pn.t);
    pose = pn;
    if (tm.leader()) b.pose[st][i] = pn;
  }
  const CcCam cam = b.cam[st][0];
  FpSlot slots[T::NS];
  cc_slots(tm, b, i, slots);
  double e[T::NS][1];
#pragma unroll
  for (int s = 0; s < T::NS; s++) e[s][0] = cc_slot_cost(slots[s], cam.v, pose.R, pose.t);
  tm.template wave_sums<1>(e, sh.cs);
  tm.barrier();
  if (tm.leader()) b.viewcost[i] = sh.cs[0];
}

// ---- the total cost in chunk order, and what follows from it (one team) ----
// step: accept or reject the candidate; else: the start's cost and counts
template <class T>
AT_FP_HD void cc_decide(const T& tm, CcSolveShared& sh, const CcBufs& b, bool step) {
  const int nch = b.chunks();
  for (int ch = tm.first(); ch < nch; ch += tm.stride()) {
    const int i0 = ch * kCcChunk, i1 = i0 + kCcChunk < b.N ? i0 + kCcChunk : b.N;
    double acc = b.viewcost[i0];
    int tags = b.ntags[i0], used = b.ntags[i0] > 0;
    for (int i = i0 + 1; i < i1; i++) {
      acc = acc + b.viewcost[i];
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

}  // namespace at

// ---- the calibrator's host side (at_camcal.cpp; at_api.cpp adds the device buffers) ----
namespace at {
struct CcGpu;  // at_api.cpp
}
struct at_camcal {
  at_camcal_config cfg;
  int max_hamming;
  double tag_size;
  std::vector<int16_t> lut;
  std::vector<at::FpTag> tags;
  std::vector<at::CcObs> obs;
  int n;           // stored views
  bool obs_dirty;  // the device copy of obs is stale
  // the last solve
  at_camcal_result result;
  std::vector<at_camcal_view> views;
  uint64_t ns;
  int profiling;
  at::CcGpu* gpu;
  void (*gpu_free)(at::CcGpu*);
};
namespace at {
// the start intrinsics of a solve: cfg.init, or the focal guess; AT_E_INVALID when the guess fails
int cc_start_camera(const at_camcal& c, CcCam* out);
// the records of a finished solve from its final buffers (host copies)
void cc_finish(at_camcal* c, const CalCtl& ctl, const CcCam& cam, const double* cov, const CalPose* pose,
               const double* viewcost, const int32_t* ntags, at_camcal_result* out);
}  // namespace at
