// at_fieldmap.h -- field map: where the tags of a field stand, from N recorded views of them,
// shared by host and device.
//
// A joint least-squares solve (bundle adjustment) over a map of 1..kFmMaxTags tags.  Unknowns: the
// camera pose of every view that takes part (x_cam = R x_field + t) and, per placed tag, the
// rotation (free_rot) and / or translation (free_trans) of x_field = R_j x_tag + t_j.  Cost: the
// summed squared error in pixels of every stored corner of every placed tag,
//   X = R_j c + t_j,  P = R X + t,  u = fx Px / Pz + cx,  v = fy Py / Pz + cy
// against at_detection.p, c the corner (-+s/2, +-s/2, 0) of at_fieldpose.h's fp_points and
// fx .. cy the view's own (views of several calibrated cameras may be mixed); Pz <= 0 costs
// HUGE_VAL, so the one comparison `cn < cost` is the whole accept rule.
//
// Parameters: per view (w, dt) as fp_apply_step (R' = dR(w) R, t' = t + dt), so dP/dw = -[R X]x
// and dP/dt = I; per tag (w_j, d_j) as rig_apply_step (R_j' = R_j dR(w_j), t_j' = t_j + d_j), so
// with G = R R_j: dP/dw_j = -G [c]x and dP/dd_j = R.  A tag parameter that is not free -- its flag
// is 0, the tag is not placed, or no stored view holds the tag -- has zero Jacobian columns, row
// and column zero, 1 on the diagonal and +0.0 on the right-hand side of the reduced system, and
// the rotation / translation it belongs to is copied, not multiplied: it comes back bit for bit.
//
// Placing (host, fm_place in at_fieldmap.cpp, before either route runs; its outcome is input to
// both).  A tag given with known = 1 is placed where the caller put it.  The others are placed in
// rounds until a round places nothing; a round visits the unplaced tags by ascending id, and a tag
// placed in a round counts as placed for the tags after it.  For an unplaced tag T, every stored
// view that holds T and at least one placed tag has a camera pose by the field pose's start rule
// over its placed tags (each placed tag's own pose as a camera pose, R_j = pose_R R_tag^T,
// t_j = pose_t - R_j t_tag; the one with the least summed squared reprojection error over the
// corners of the view's placed tags, none behind the camera; ties: the lower id; made orthonormal
// by fp_project_rotation) and from it one candidate (cam_T_field)^-1 cam_T_tag, made orthonormal
// the same way.  T gets the candidate with the least summed squared reprojection error of T's
// corners over all such views (a corner at Pz <= 0: infinite); ties go to the lower view.  A tag
// that no chain of views reaches is not placed: placed = 0, zeros in its record, and its
// observations take no part on either route.  R0, t0 of the result are these start poses.
//
// The start of a view is fp_solve_frame over the placed tags' start poses (the field pose's whole
// solve: k_fm_start); a view that comes back with n_tags = 0 takes no part.
//
// kFmIters Levenberg-Marquardt iterations, fixed, on the whole problem, by the Schur complement of
// the views' pose blocks.  With U, g the normal equations of a view's pose, V_j, h_j those of tag j
// over its four corners in that view and W_j = Jp^T Jt (6 x 6, row k of the pose), an iteration is
//   accumulate  (fm_accum, per view, one slot per corner) U, g as the 64-slot xor tree of
//               at_fieldpose.h; the 63 sums of a tag over its quad of slots as
//               (c0 + c2) + (c1 + c3) -- the two last steps of that tree; Y_j =
//               (U + lambda diag U)^-1 W_j and y = (U + lambda diag U)^-1 g column by column by
//               fp_solve6.  The view keeps U, g, y and per tag slot V_j, h_j, W_j, Y_j
//               (kFmViewLen doubles: 12.9 KB, whatever the size of the map); its two tables,
//               slot -> map index (read here and in back) and map index -> slot (read in
//               reduce), -1: none, are written once, by fm_start.  fp_solve6's verdict is not
//               looked at here: a view whose damped U has no Cholesky factor (a pivot that is
//               not positive) keeps the columns fp_solve6 leaves, which hold NaN (a negative
//               pivot) or infinities (a zero one); they spoil the entries of its tags in the
//               reduced system, whose factor then fails on a NaN pivot (not positive), so that
//               the iteration is rejected with every step zero and lambda tenfold, and fm_back
//               gives that view a zero pose step; the tests hold no such view, and whatever the
//               values, both routes run the same operations on them;
//   reduce      (fm_chunk_entry, fm_total) the reduced system of size M = 6 n_tags is never
//               formed per view.  For every pair of map tags J <= K the 36 entries
//               S[6J+a][6K+b] = sum over the views that hold both of
//               ([J == K] V_J[a][b] - sum_k W_J[k][a] Y_K[k][b]), k ascending; rhs[6J+a] = sum of
//               (h_J[a] - sum_k W_J[k][a] y[k]); vd[6J+a] = sum of V_J[a][a].  Every sum starts at
//               +0.0 and runs over the views ascending within chunks of kFmChunk, then over the
//               chunk sums ascending.  A view that takes no part, or that does not hold both tags
//               (placed), is passed over: it adds nothing, not even +0.0;
//   solve       (fm_solve, one team) lambda times vd on the free diagonals; Cholesky column by
//               column, each entry (a - sum_k L[i][k] L[j][k]) / L[j][j] with k ascending;
//               forward substitution with k ascending, back substitution with k descending (both
//               column-oriented: v[i] -= L[i][k] y[k] for every i at once); a pivot that is not
//               positive is a failed factor: every step is zero and the iteration counts as
//               rejected.  The tags' candidates are written here;
//   back        (fm_back, per view) the pose step -(U + lambda diag U)^-1 (g + sum_j W_j d_j), j
//               over the view's slots ascending, applied to the candidate copy; the candidate's
//               cost;
//   decide      (fm_decide, one team) `cn < cost` takes the candidates (CalCtl::which flips) and
//               divides lambda by 10 (floor 1e-9), else lambda grows tenfold.
// The covariance of tag J is sigma^2 times the J-th 6 x 6 diagonal block of S^-1, S the undamped
// reduced matrix at the final state (6 columns of the inverse per tag, each by a forward and a
// back substitution), order (w_j, d_j), sigma^2 = cost / (2 corners - 6 views_used - free
// parameters); rows and columns of parameters that are not free are zero; cov_valid = 0 (and
// zeros) without a factor or with a denominator that is not positive.
//
// A part of the map that hangs together through views but holds no fixed tag (a component without
// an anchor) is not refused: its tags move together with its views at no cost, so the damped
// iterations still lower the cost inside it, where it ends up against the anchored part is
// whatever the start gave, and the undamped final matrix is singular up to rounding: cov_valid is
// whatever its Cholesky factor says (none in the tests' case: cov_valid = 0 and zeros) and, with a
// factor, the variances of that component mean nothing.  Both routes run the same operations on it
// and return equal records.
//
// The kernels (at_kernels.hip: k_fm_*) and the CPU twin (at_fieldmap.cpp) instantiate these
// functions with a team (at_rigcal.h's, plus quad() for the sum over a tag's four slots) over the
// same FmBufs, device or host pointers.  at_fieldpose.h's rules hold: no contraction, only
// + - * / sqrt, every sum in one stated order.
#pragma once

#include "at_rigcal.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace at {

constexpr int kFmMaxTags = 32;     // AT_FIELDMAP_MAX_TAGS
constexpr int kFmMaxViews = 4096;  // AT_FIELDMAP_MAX_VIEWS
// LM iterations, chosen on the CPU with the twin.  The exact-corner case of
// tests/test_field_map_host.py (6 tags, 12 views, free tags 3 degrees / 30 mm off) is within 1e-9
// of the truth after 5 iterations (worst entry 8.7e-11) and at its rounding floor (rms 7e-14 px,
// worst entry 5e-15) after 6; from there on steps are rejected or gain nothing.  16, the rig
// calibration's count, leaves ten for starts further off (a tag placed by a chain of views begins
// 0.1 m off in the tests) and for rejected steps.
constexpr int kFmIters = 16;
constexpr int kFmChunk = 32;
constexpr int kFmMaxChunks = kFmMaxViews / kFmChunk;
constexpr int kFmMaxParams = 6 * kFmMaxTags;
constexpr int kFmTagLen = 99;                               // V 21, h 6, W 36, Y 36
constexpr int kFmHead = 33;                                 // U 21, g 6, y 6
constexpr int kFmViewLen = kFmHead + kFpMaxTags * kFmTagLen;  // 1617 doubles per view
constexpr int kFmV = 0, kFmH = 21, kFmW = 27, kFmY = 63;
static_assert(kFmViewLen * sizeof(double) + (kFpMaxTags + kFmMaxTags) * sizeof(int32_t) < 65536,
              "a view's scratch stays under 64 KB");

// one view's selected map tags, ascending ids, and its camera
struct FmObs {
  int32_t m;
  int32_t dropped;           // eligible candidates beyond the 16 lowest ids
  int32_t ids[kFpMaxTags];
  int32_t idx[kFpMaxTags];   // the tag's index in the map
  double p[kFpMaxTags][8];
  double pose_R[kFpMaxTags][9];
  double pose_t[kFpMaxTags][3];
  double fx, fy, cx, cy;
};
static_assert(sizeof(FmObs) == 2728, "FmObs: 2728 B per view");

struct FmBufs {
  const FmObs* obs;   // [N]
  FpRecord* rec;      // [N] the start
  int32_t* ntags;     // [N] the start's n_tags: 0 takes no part
  CalPose* pose[2];   // [N]
  CalPose* tag[2];    // [T]
  double* view;       // [N][kFmViewLen]
  int32_t* tab;       // [N][kFpMaxTags] slot -> map index, -1: the slot takes no part
  int32_t* inv;       // [N][kFmMaxTags] map index -> slot, -1: not in the view
  double* chunk;      // [chunks][E]
  double* S;          // [E] the sums over the chunks
  double* A;          // [M][M] one row per covariance column (the final pass)
  double* dc;         // [M] the tags' step
  double* viewcost;   // [N]
  double* cov;        // [T][36]
  CalCtl* ctl;        // (instants -> views)
  FpLayout lay;       // the placed tags' start poses (an id that is not placed: -1)
  double tag_size;
  int8_t placed[kFmMaxTags], free_rot[kFmMaxTags], free_trans[kFmMaxTags];  // free_*: in effect
  int N, T;
  AT_CAL_M int M() const { return 6 * T; }
  AT_CAL_M int pairs() const { return T * (T + 1) / 2; }
  AT_CAL_M int pair(int J, int K) const { return J * T - J * (J - 1) / 2 + (K - J); }  // J <= K
  AT_CAL_M int E() const { return 36 * pairs() + 12 * T; }
  AT_CAL_M int chunks() const { return (N + kFmChunk - 1) / kFmChunk; }
  AT_CAL_M bool is_free(int p) const { return (p % 6 < 3 ? free_rot[p / 6] : free_trans[p / 6]) != 0; }
  // the map index of a view's slot j, -1: beyond its tags or not placed
  AT_CAL_M int slot_tag(const FmObs& o, int j) const { return j < o.m && placed[o.idx[j]] ? o.idx[j] : -1; }
};

// the stored tags of a view as fp_solve_frame's candidates
struct FmSrc {
  const FmObs* o;
  AT_CAL_M int n() const { return o->m; }
  AT_CAL_M int32_t id(int c) const { return o->ids[c]; }
  AT_CAL_M int32_t hamming(int) const { return 0; }
  AT_CAL_M float margin(int) const { return 0.0f; }
  AT_CAL_M const double* p(int c) const { return o->p[c]; }
  AT_CAL_M const double* pose_R(int c) const { return o->pose_R[c]; }
  AT_CAL_M const double* pose_t(int c) const { return o->pose_t[c]; }
};

struct FmShared {
  double U[kRigSums];             // U 21, g 6
  double W[kFpMaxTags][36];       // W_j[k][b]
  double y[6];
  double r[6];
  double c[kRigSums];
};
struct FmSolveShared {
  double rhs[kFmMaxParams], vd[kFmMaxParams], v[kFmMaxParams], y[kFmMaxParams], x[kFmMaxParams];
  double d[kFmMaxParams];  // the factor's diagonal
  double cc[kFmMaxChunks];
  int32_t ct[kFmMaxChunks], cu[kFmMaxChunks];
};

// one corner slot: its corner in the tag frame, its pixel and its tag's map index
struct FmSlot {
  double sx, sy;
  double u, v;
  int tag;
  bool valid;
};

// slot 4j + c of view o: corner c of stored tag j, valid when the tag is placed
template <class T>
AT_FP_HD void fm_slots(const T& tm, const FmBufs& b, const FmObs& o, FmSlot* slots) {
  const double hs = b.tag_size / 2.0;
#pragma unroll
  for (int s = 0; s < T::NS; s++) {
    const int sl = tm.wave().slot(s), j = sl >> 2, c = sl & 3;
    FmSlot& q = slots[s];
    q.tag = b.slot_tag(o, j);
    q.valid = q.tag >= 0;
    q.sx = (c == 0 || c == 3) ? -hs : hs;  // estimate_tag_pose's corners (fp_points)
    q.sy = c < 2 ? hs : -hs;
    q.u = q.valid ? o.p[j][c * 2] : 0.0;
    q.v = q.valid ? o.p[j][c * 2 + 1] : 0.0;
    if (!q.valid) q.tag = 0;
  }
}

// X = R_j c + t_j (fp_points' arithmetic), Q = R X, P = Q + t
AT_FP_HD void fm_point(const FmSlot& s, const CalPose& tg, const double* R, const double* t, double* Q, double* P) {
  double X[3];
#pragma unroll
  for (int k = 0; k < 3; k++) X[k] = (tg.R[k * 3] * s.sx + tg.R[k * 3 + 1] * s.sy) + tg.t[k];
  fp_rot(R, X, Q);
#pragma unroll
  for (int k = 0; k < 3; k++) P[k] = Q[k] + t[k];
}

// squared reprojection error of one slot; HUGE_VAL with its Z not positive
AT_FP_HD double fm_slot_cost(const FmSlot& s, const FmObs& o, const CalPose& tg, const double* R, const double* t) {
  if (!s.valid) return 0.0;
  double Q[3], P[3];
  fm_point(s, tg, R, t, Q, P);
  if (!(P[2] > 0.0)) return HUGE_VAL;
  const double ru = (o.fx * (P[0] / P[2]) + o.cx) - s.u;
  const double rv = (o.fy * (P[1] / P[2]) + o.cy) - s.v;
  return ru * ru + rv * rv;
}

// the slot's residual rows in j[26]: the pose's (jpu 0..5, jpv 6..11), its tag's (jtu 12..17,
// jtv 18..23; 0 where not free) and (ru, rv) at 24, 25
AT_FP_HD void fm_slot_rows(const FmSlot& s, const FmObs& o, const CalPose& tg, const double* R, const double* t,
                           bool free_rot, bool free_trans, double* j) {
  double Q[3], P[3];
  fm_point(s, tg, R, t, Q, P);
  const double xn = P[0] / P[2], yn = P[1] / P[2];
  j[24] = (o.fx * xn + o.cx) - s.u;
  j[25] = (o.fy * yn + o.cy) - s.v;
  // du/dP = (A, 0, B), dv/dP = (0, C, D); dP/dw = -[Q]x, dP/dt = I (fp_slot_normal)
  const double A = o.fx / P[2], B = -(o.fx * xn) / P[2];
  const double C = o.fy / P[2], D = -(o.fy * yn) / P[2];
  j[0] = B * Q[1];
  j[1] = A * Q[2] - B * Q[0];
  j[2] = -(A * Q[1]);
  j[3] = A;
  j[4] = 0.0;
  j[5] = B;
  j[6] = D * Q[1] - C * Q[2];
  j[7] = -(D * Q[0]);
  j[8] = C * Q[0];
  j[9] = 0.0;
  j[10] = C;
  j[11] = D;
  // G = R R_j; dP/dw_j = -G [c]x = (sy G2, -sx G2, sx G1 - sy G0) by columns G0, G1, G2; dP/dd_j = R
  double G[9];
  fp_mul_ab(R, tg.R, G);
  double dP[3][6];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    dP[r][0] = s.sy * G[r * 3 + 2];
    dP[r][1] = -(s.sx * G[r * 3 + 2]);
    dP[r][2] = s.sx * G[r * 3 + 1] - s.sy * G[r * 3];
    dP[r][3] = R[r * 3];
    dP[r][4] = R[r * 3 + 1];
    dP[r][5] = R[r * 3 + 2];
  }
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const bool fr = c < 3 ? free_rot : free_trans;
    j[12 + c] = fr ? A * dP[0][c] + B * dP[2][c] : 0.0;
    j[18 + c] = fr ? C * dP[1][c] + D * dP[2][c] : 0.0;
  }
}

// ---- start: fp_solve_frame over the placed tags' start poses ----
template <class T>
AT_FP_HD void fm_start(const T& tm, const FmBufs& b, int i) {
  const FmObs& o = b.obs[i];
  const FmSrc src = {&o};
  const FpCam cam = {o.fx, o.fy, o.cx, o.cy};
  fp_solve_frame(tm.wave(), src, b.lay, cam, b.tag_size, b.rec + i, (FpRecord*)nullptr);
  if (tm.leader()) {
    const FpRecord& r = b.rec[i];
    b.ntags[i] = r.n_tags;
    CalPose p;
    for (int k = 0; k < 9; k++) p.R[k] = r.R[k];
    for (int k = 0; k < 3; k++) p.t[k] = r.t[k];
    b.pose[0][i] = p;
    b.pose[1][i] = p;
  }
  // the view's two tables, once per solve: they depend on the stored view, on which tags are
  // placed and on whether the view takes part, none of which changes afterwards
  tm.barrier();
  const bool part = b.ntags[i] > 0;
  for (int j = tm.first(); j < kFpMaxTags; j += tm.stride()) b.tab[(size_t)i * kFpMaxTags + j] = part ? b.slot_tag(o, j) : -1;
  for (int J = tm.first(); J < kFmMaxTags; J += tm.stride()) {
    int s = -1;
    for (int j = 0; j < kFpMaxTags; j++)
      if (part && b.slot_tag(o, j) == J) s = j;
    b.inv[(size_t)i * kFmMaxTags + J] = s;
  }
}

// ---- accumulate: what view i keeps for the reduced system ----
template <class T>
AT_FP_HD void fm_accum(const T& tm, FmShared& sh, const FmBufs& b, int i, bool final) {
  const FmObs& o = b.obs[i];
  if (b.ntags[i] <= 0) return;
  const int32_t* tab = b.tab + (size_t)i * kFpMaxTags;
  double* view = b.view + (size_t)i * kFmViewLen;
  const int which = b.ctl->which;
  const double lambda = final ? 0.0 : b.ctl->lambda;
  const CalPose pose = b.pose[which][i];
  {
    FmSlot slots[T::NS];
    fm_slots(tm, b, o, slots);
    double j[T::NS][26];
#pragma unroll
    for (int s = 0; s < T::NS; s++) {
#pragma unroll
      for (int q = 0; q < 26; q++) j[s][q] = 0.0;
      const int tg = slots[s].tag;
      if (slots[s].valid)
        fm_slot_rows(slots[s], o, b.tag[which][tg], pose.R, pose.t, b.free_rot[tg] != 0, b.free_trans[tg] != 0, j[s]);
    }
    {  // U, g over the 64 slots
      double v[T::NS][27];
#pragma unroll
      for (int s = 0; s < T::NS; s++)
        cal_slot_pass<0>(slots[s].valid, j[s], j[s] + 6, j[s] + 12, j[s] + 18, j[s][24], j[s][25], v[s]);
      tm.template wave_sums<27>(v, sh.U);
    }
    // a tag's sums over its quad: value e of kFmTagLen's first 63
    auto put = [&](int e, const double* val) {
      double q[T::NS];
      tm.quad(val, q);
#pragma unroll
      for (int s = 0; s < T::NS; s++) {
        const int sl = tm.wave().slot(s);
        if ((sl & 3) == 0 && slots[s].valid) {
          view[kFmHead + (sl >> 2) * kFmTagLen + e] = q[s];
          if (e >= kFmW) sh.W[sl >> 2][e - kFmW] = q[s];
        }
      }
    };
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int c = a; c < 6; c++) {
        double val[T::NS];
#pragma unroll
        for (int s = 0; s < T::NS; s++) val[s] = j[s][12 + a] * j[s][12 + c] + j[s][18 + a] * j[s][18 + c];
        put(kFmV + fp_tri(a, c), val);
      }
      double val[T::NS];
#pragma unroll
      for (int s = 0; s < T::NS; s++) val[s] = j[s][12 + a] * j[s][24] + j[s][18 + a] * j[s][25];
      put(kFmH + a, val);
    }
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
      for (int c = 0; c < 6; c++) {
        double val[T::NS];
#pragma unroll
        for (int s = 0; s < T::NS; s++) val[s] = j[s][k] * j[s][12 + c] + j[s][6 + k] * j[s][18 + c];
        put(kFmW + 6 * k + c, val);
      }
  }
  tm.barrier();
  for (int e = tm.first(); e < 27; e += tm.stride()) view[e] = sh.U[e];
  for (int col = tm.first(); col <= 6 * kFpMaxTags; col += tm.stride()) {
    const int jj = col / 6, bb = col % 6;
    const bool isy = col == 6 * kFpMaxTags;
    if (!isy && tab[jj] < 0) continue;
    double rhs[6], x[6];
    for (int k = 0; k < 6; k++) rhs[k] = isy ? -sh.U[21 + k] : -sh.W[jj][6 * k + bb];
    fp_solve6(sh.U, rhs, lambda, x);
    for (int k = 0; k < 6; k++) {
      if (isy) view[27 + k] = x[k];
      else view[kFmHead + jj * kFmTagLen + kFmY + 6 * k + bb] = x[k];
    }
  }
}

// ---- entry e of item `item` of chunk ch: its views in ascending order ----
// items 0 .. pairs-1: the pair (J, K), e = 6 a + b; then one item per tag, e < 6: rhs, e < 12: vd
AT_FP_HD void fm_chunk_entry(const FmBufs& b, int ch, int item, int e) {
  const int np = b.pairs();
  const int i0 = ch * kFmChunk, i1 = i0 + kFmChunk < b.N ? i0 + kFmChunk : b.N;
  double acc = 0.0;
  if (item < np) {
    int J = 0, rest = item;
    while (rest >= b.T - J) {
      rest -= b.T - J;
      J++;
    }
    const int K = J + rest, a = e / 6, bb = e % 6;
    const int tri = a <= bb ? fp_tri(a, bb) : fp_tri(bb, a);
    for (int i = i0; i < i1; i++) {
      const int sj = b.inv[(size_t)i * kFmMaxTags + J], sk = b.inv[(size_t)i * kFmMaxTags + K];
      if (sj < 0 || sk < 0) continue;
      const double* vw = b.view + (size_t)i * kFmViewLen + kFmHead;
      const double* Wj = vw + sj * kFmTagLen + kFmW;
      const double* Yk = vw + sk * kFmTagLen + kFmY;
      double t = Wj[a] * Yk[bb];
      for (int k = 1; k < 6; k++) t = t + Wj[6 * k + a] * Yk[6 * k + bb];
      const double v0 = J == K ? vw[sj * kFmTagLen + kFmV + tri] : 0.0;
      acc = acc + (v0 - t);
    }
    b.chunk[(size_t)ch * b.E() + 36 * item + e] = acc;
    return;
  }
  const int J = item - np, a = e % 6;
  for (int i = i0; i < i1; i++) {
    const int sj = b.inv[(size_t)i * kFmMaxTags + J];
    if (sj < 0) continue;
    const double* vh = b.view + (size_t)i * kFmViewLen;
    const double* tj = vh + kFmHead + sj * kFmTagLen;
    if (e < 6) {
      double t = tj[kFmW + a] * vh[27];
      for (int k = 1; k < 6; k++) t = t + tj[kFmW + 6 * k + a] * vh[27 + k];
      acc = acc + (tj[kFmH + a] - t);
    } else {
      acc = acc + tj[kFmV + fp_tri(a, a)];
    }
  }
  b.chunk[(size_t)ch * b.E() + 36 * np + 12 * J + e] = acc;
}

// ---- entry e over the chunks, ascending ----
AT_FP_HD void fm_total(const FmBufs& b, int e) {
  const int E = b.E(), nch = b.chunks();
  double acc = 0.0;
  for (int ch = 0; ch < nch; ch++) acc = acc + b.chunk[(size_t)ch * E + e];
  b.S[e] = acc;
}

// ---- the reduced solve (one team).  final: the undamped matrix and its inverse's blocks ----
// P: the packed lower triangle, M (M + 1) / 2 doubles, entry (i, j <= i) at i (i + 1) / 2 + j.  It
// holds the reduced matrix (entry (i, j) is row j, column i of its upper triangle) and is
// overwritten in place, below the diagonal, by the factor: L[i][j] takes the place of the entry it
// is computed from, by the thread that read it.  The factor's diagonal goes to sh.d, so the
// matrix's own diagonal, which every thread reads at the start of a column, is never written.
template <class T>
AT_FP_HD void fm_solve(const T& tm, FmSolveShared& sh, const FmBufs& b, double* P, bool final) {
  const int M = b.M(), np = b.pairs();
  const double lambda = b.ctl->lambda;
  const int which = b.ctl->which;
  auto at = [](int i, int j) { return (size_t)i * (i + 1) / 2 + j; };
  for (int p = tm.first(); p < M; p += tm.stride()) {
    sh.rhs[p] = b.S[36 * np + 12 * (p / 6) + p % 6];
    sh.vd[p] = b.S[36 * np + 12 * (p / 6) + 6 + p % 6];
  }
  tm.barrier();
  for (int e = tm.first(); e < M * M; e += tm.stride()) {
    const int r = e / M, s = e % M;
    if (r > s) continue;
    double a = b.S[36 * b.pair(r / 6, s / 6) + 6 * (r % 6) + s % 6];
    if (!b.is_free(r) || !b.is_free(s)) a = r == s ? 1.0 : 0.0;
    else if (r == s && !final) a = a + lambda * sh.vd[r];
    P[at(s, r)] = a;
  }
  tm.barrier();
  bool ok = true;
  for (int j = 0; j < M; j++) {
    double s = P[at(j, j)];
    for (int k = 0; k < j; k++) s = s - P[at(j, k)] * P[at(j, k)];
    if (!(s > 0.0)) ok = false;
    const double ljj = sqrt(s);
    for (int i = j + tm.first(); i < M; i += tm.stride()) {
      if (i == j) {
        sh.d[j] = ljj;
        continue;
      }
      double v = P[at(i, j)];
      for (int k = 0; k < j; k++) v = v - P[at(i, k)] * P[at(j, k)];
      P[at(i, j)] = v / ljj;
    }
    tm.barrier();
  }
  if (!final) {
    for (int i = tm.first(); i < M; i += tm.stride()) sh.v[i] = b.is_free(i) ? -sh.rhs[i] : 0.0;
    tm.barrier();
    for (int k = 0; k < M; k++) {
      const double yk = sh.v[k] / sh.d[k];
      if (tm.leader()) sh.y[k] = yk;
      for (int i = k + 1 + tm.first(); i < M; i += tm.stride()) sh.v[i] = sh.v[i] - P[at(i, k)] * yk;
      tm.barrier();
    }
    for (int i = tm.first(); i < M; i += tm.stride()) sh.v[i] = sh.y[i];
    tm.barrier();
    for (int k = M - 1; k >= 0; k--) {
      const double xk = sh.v[k] / sh.d[k];
      if (tm.leader()) sh.x[k] = xk;
      for (int i = tm.first(); i < k; i += tm.stride()) sh.v[i] = sh.v[i] - P[at(k, i)] * xk;
      tm.barrier();
    }
    for (int i = tm.first(); i < M; i += tm.stride()) {
      const double d = ok && b.is_free(i) ? sh.x[i] : 0.0;
      sh.v[i] = d;
      b.dc[i] = d;
    }
    if (tm.leader()) b.ctl->factor_ok = ok ? 1 : 0;
    tm.barrier();
    for (int c = tm.first(); c < b.T; c += tm.stride())
      cal_apply_ext(b.tag[which][c], sh.v + 6 * c, b.free_rot[c] != 0, b.free_trans[c] != 0, &b.tag[which ^ 1][c]);
    return;
  }
  // column p of S^-1 in row p of A: forward (k ascending), then back (k descending) down to the
  // first row of p's block
  int den = 2 * b.ctl->corners - 6 * b.ctl->used;
  for (int p = 0; p < M; p++) den -= b.is_free(p) ? 1 : 0;
  const bool valid = ok && den > 0;
  const double s2 = b.ctl->cost / (double)den;
  for (int p = tm.first(); p < M; p += tm.stride()) {
    const int c = p / 6, a = p % 6;
    double* w = b.A + (size_t)p * M;
    if (valid && b.is_free(p)) {
      for (int i = 0; i < M; i++) w[i] = i == p ? 1.0 : 0.0;
      for (int k = p; k < M; k++) {  // (rows above p stay +0.0)
        const double yk = w[k] / sh.d[k];
        w[k] = yk;
        for (int i = k + 1; i < M; i++) w[i] = w[i] - P[at(i, k)] * yk;
      }
      for (int k = M - 1; k >= 6 * c; k--) {
        const double xk = w[k] / sh.d[k];
        w[k] = xk;
        for (int i = 6 * c; i < k; i++) w[i] = w[i] - P[at(k, i)] * xk;
      }
    }
    for (int bb = 0; bb < 6; bb++)
      b.cov[c * 36 + a * 6 + bb] = valid && b.is_free(p) && b.is_free(6 * c + bb) ? s2 * w[6 * c + bb] : 0.0;
  }
  if (tm.leader()) b.ctl->cov_valid = valid ? 1 : 0;
}

// ---- back substitution and the candidate's cost (step), or the current state's cost ----
template <class T>
AT_FP_HD void fm_back(const T& tm, FmShared& sh, const FmBufs& b, int i, bool step) {
  if (b.ntags[i] <= 0) {
    if (tm.leader()) b.viewcost[i] = 0.0;
    return;
  }
  const FmObs& o = b.obs[i];
  const int which = b.ctl->which, st = step ? which ^ 1 : which;
  CalPose pose = b.pose[which][i];
  if (step) {
    const double* view = b.view + (size_t)i * kFmViewLen;
    for (int k = tm.first(); k < 6; k += tm.stride()) {
      double acc = view[21 + k];
      for (int j = 0; j < kFpMaxTags; j++) {
        const int J = b.tab[(size_t)i * kFpMaxTags + j];
        if (J < 0) continue;
        const double* W = view + kFmHead + j * kFmTagLen + kFmW;
        for (int bb = 0; bb < 6; bb++) acc = acc + W[6 * k + bb] * b.dc[6 * J + bb];
      }
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
  FmSlot slots[T::NS];
  fm_slots(tm, b, o, slots);
  double e[T::NS][1];
#pragma unroll
  for (int s = 0; s < T::NS; s++) e[s][0] = fm_slot_cost(slots[s], o, b.tag[st][slots[s].tag], pose.R, pose.t);
  tm.template wave_sums<1>(e, sh.c);
  tm.barrier();
  if (tm.leader()) b.viewcost[i] = sh.c[0];
}

// ---- the total cost in chunk order, and what follows from it (one team) ----
// step: accept or reject the candidate; else: the start's cost and counts
template <class T>
AT_FP_HD void fm_decide(const T& tm, FmSolveShared& sh, const FmBufs& b, bool step) {
  const int nch = b.chunks();
  for (int ch = tm.first(); ch < nch; ch += tm.stride()) {
    const int i0 = ch * kFmChunk, i1 = i0 + kFmChunk < b.N ? i0 + kFmChunk : b.N;
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

// Every slot of the view held by one host thread.
struct FmHostTeam : CalHostTeam {
  void quad(const double* v, double* o) const {
    for (int j = 0; j < kFpMaxTags; j++) {
      const double q = (v[4 * j] + v[4 * j + 2]) + (v[4 * j + 1] + v[4 * j + 3]);
      for (int c = 0; c < 4; c++) o[4 * j + c] = q;
    }
  }
};

}  // namespace at

// ---- the mapper's host side (at_fieldmap.cpp; at_api.cpp adds the device buffers) ----
namespace at {
struct FmGpu;  // at_api.cpp
}
struct at_fieldmap {
  int n_tags;
  int max_hamming;
  double tag_size;
  at_fieldmap_tag tags[at::kFmMaxTags];
  std::vector<int16_t> lut;        // id -> map index, every tag of the map (the selection of a view)
  std::vector<at::FmObs> obs;
  int n;           // stored views
  bool obs_dirty;  // the device copy of obs is stale
  // the last solve
  at_fieldmap_result result;
  std::vector<at_fieldmap_tag_result> tag_results;
  std::vector<at_fieldmap_view> views;
  uint64_t ns;
  int profiling;
  at::FmGpu* gpu;
  void (*gpu_free)(at::FmGpu*);
};
namespace at {
// What both routes start from: the placed tags' start poses (start[T]), the layout over them
// (lut[kFpMaxIds], lay_tags[T]), and the parts of FmBufs that do not depend on where the buffers
// live (placed, the free flags in effect, the sizes).  seen[T]: stored views that hold the tag.
void fm_prepare(const at_fieldmap& m, FmBufs* b, CalPose* start, int16_t* lut, FpTag* lay_tags, int32_t* seen);
// the records of a finished solve from its final buffers (host copies)
void fm_finish(at_fieldmap* m, const FmBufs& b, const CalCtl& ctl, const CalPose* start, const int32_t* seen,
               const CalPose* tag, const double* cov, const CalPose* pose, const double* viewcost,
               const int32_t* ntags, at_fieldmap_result* out);
}  // namespace at
