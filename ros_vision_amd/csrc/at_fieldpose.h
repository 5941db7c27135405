// at_fieldpose.h -- one camera pose per frame from every layout tag in it, shared by
// host and device.
//
// The frame's detections whose ids a field layout knows (x_field = R_tag x_tag + t_tag)
// give 4 point correspondences each; the camera pose x_cam = R x_field + t is the
// Levenberg-Marquardt minimum of the summed squared reprojection error in pixels,
// started from the best single-tag pose (k_pose's).  The whole algorithm -- selection
// key, points, start, every arithmetic operation of the refinement -- lives here once:
// the kernel (at_kernels.hip: k_field, one wave per frame, one lane per corner) and the
// CPU twin (at_fieldpose.cpp: at_field_pose_host) instantiate fp_solve_frame with a
// "wave" that tells how the 64 corner slots are spread over threads (FpHostWave: one
// thread holds all 64; the kernel's: one slot per lane) and how a value crosses them.
//
// Host and device take the same accept / reject decisions because every double
// operation is the same IEEE operation in the same order:
//   * no contraction (the pragma below; at_pose.h allows it, this header does not);
//   * only + - * / sqrt, all correctly rounded on both sides; no trigonometry;
//   * every sum over the corners runs over 64 slots (unused ones hold +0.0) as the
//     butterfly v[i] += v[i ^ off], off = 32, 16, .. 1: a + b == b + a bit for bit, so
//     every lane ends with the value of the tree (i, i + 32), (i, i + 16), ... which
//     the host evaluates directly.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define AT_FP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define AT_FP_HD static inline
#endif

namespace at {

constexpr int kFpMaxTags = 16;    // AT_FIELD_MAX_TAGS
constexpr int kFpSlots = 64;      // 4 corners x kFpMaxTags: one wave
constexpr int kFpMaxIds = 1024;   // ids a layout may name: [0, kMaxCodes)
constexpr int kFpIters = 12;      // LM iterations, fixed (no early exit)
constexpr int kFpMaxCand = 65536; // candidates scanned per frame (the key holds 16 slot bits)

struct FpCam { double fx, fy, cx, cy; };
struct FpTag { double R[9]; double t[3]; };  // x_field = R x_tag + t
struct FpLayout {
  const int16_t* lut;   // [kFpMaxIds] id -> index into tags, -1: not in the layout
  const FpTag* tags;
  int max_hamming;
};

// at_field_pose and the two counters at_field_stats sums
struct FpRecord {
  int32_t n_tags;
  int32_t ids[kFpMaxTags];
  double R[9];
  double t[3];
  double rms_px;
  int32_t steps_taken;
  int32_t rejected;   // LM steps not taken (cost did not fall, a point behind the camera, no Cholesky factor)
  int32_t dropped;    // eligible candidates with an id beyond the 16 lowest
  int32_t pad;
};
static_assert(sizeof(FpRecord) == 192, "FpRecord: 192 B per frame");

// ---- selection ------------------------------------------------------------------
// One key per eligible candidate; ascending key order is ascending id, then lowest
// hamming, then greatest decision margin, then lowest slot.  The selection is the first
// key of each of the 16 lowest ids.
constexpr uint64_t kFpNoKey = ~0ull;
AT_FP_HD uint64_t fp_key(const FpLayout& lay, int32_t id, int32_t hamming, float margin, uint32_t slot) {
  if (id < 0 || id >= kFpMaxIds || lay.lut[id] < 0 || hamming < 0 || hamming > lay.max_hamming) return kFpNoKey;
  const uint32_t b = __builtin_bit_cast(uint32_t, margin);
  const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // monotonic in the float's order
  const uint64_t h = (uint64_t)(hamming > 15 ? 15 : hamming);
  return ((uint64_t)id << 52) | (h << 48) | ((uint64_t)(~asc) << 16) | (uint64_t)(slot & 0xffffu);
}

// ---- small dense helpers ---------------------------------------------------------
// c = a b^T, 3x3 row-major, each entry (p + q) + r
AT_FP_HD void fp_mul_abt(const double* a, const double* b, double* c) {
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++)
      c[r * 3 + k] = (a[r * 3] * b[k * 3] + a[r * 3 + 1] * b[k * 3 + 1]) + a[r * 3 + 2] * b[k * 3 + 2];
}
// c = a b
AT_FP_HD void fp_mul_ab(const double* a, const double* b, double* c) {
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++)
      c[r * 3 + k] = (a[r * 3] * b[k] + a[r * 3 + 1] * b[3 + k]) + a[r * 3 + 2] * b[6 + k];
}
// y = a x (no translation)
AT_FP_HD void fp_rot(const double* a, const double* x, double* y) {
  for (int r = 0; r < 3; r++) y[r] = (a[r * 3] * x[0] + a[r * 3 + 1] * x[1]) + a[r * 3 + 2] * x[2];
}

// rotation matrix of the unit quaternion (q0; q1, q2, q3)
AT_FP_HD void fp_quat_to_R(double q0, double q1, double q2, double q3, double* R) {
  const double xx = q1 * q1, yy = q2 * q2, zz = q3 * q3;
  const double xy = q1 * q2, xz = q1 * q3, yz = q2 * q3;
  const double wx = q0 * q1, wy = q0 * q2, wz = q0 * q3;
  R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
  R[3] = 2.0 * (xy + wz);       R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
  R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = 1.0 - 2.0 * (xx + yy);
}

// The rotation nearest in quaternion terms to an almost-orthonormal R (the start is
// pose_R R_tag^T, and a layout's R is only held to 1e-6): largest-pivot quaternion
// extraction, normalised, and back.
AT_FP_HD void fp_project_rotation(double* R) {
  const double tr = (R[0] + R[4]) + R[8];
  double q0, q1, q2, q3;
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q0 = 0.25 * s; q1 = (R[7] - R[5]) / s; q2 = (R[2] - R[6]) / s; q3 = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0;
    q0 = (R[7] - R[5]) / s; q1 = 0.25 * s; q2 = (R[1] + R[3]) / s; q3 = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0;
    q0 = (R[2] - R[6]) / s; q1 = (R[1] + R[3]) / s; q2 = 0.25 * s; q3 = (R[5] + R[7]) / s;
  } else {
    const double s = sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0;
    q0 = (R[3] - R[1]) / s; q1 = (R[2] + R[6]) / s; q2 = (R[5] + R[7]) / s; q3 = 0.25 * s;
  }
  const double n = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
  fp_quat_to_R(q0 / n, q1 / n, q2 / n, q3 / n, R);
}

// R' = dR(w) R with dR from q = (1, w / 2) normalised; t' = t + dt.  d = (w, dt).
AT_FP_HD void fp_apply_step(const double* R, const double* t, const double* d, double* Rn, double* tn) {
  const double h0 = 0.5 * d[0], h1 = 0.5 * d[1], h2 = 0.5 * d[2];
  const double n = sqrt(1.0 + ((h0 * h0 + h1 * h1) + h2 * h2));
  double dR[9];
  fp_quat_to_R(1.0 / n, h0 / n, h1 / n, h2 / n, dR);
  fp_mul_ab(dR, R, Rn);
  for (int k = 0; k < 3; k++) tn[k] = t[k] + d[3 + k];
}

// (A + lambda diag(A)) x = -g by Cholesky; A's upper triangle in a[21] (row i, column
// j >= i at fp_tri(i, j)).  false: a pivot is not positive (or not a number).
AT_FP_HD constexpr int fp_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }
AT_FP_HD bool fp_solve6(const double* a, const double* g, double lambda, double* x) {
  double L[6][6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double s = a[fp_tri(j, j)] + lambda * a[fp_tri(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k];
    if (!(s > 0.0)) ok = false;
    const double ljj = sqrt(s);
    L[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double v = a[fp_tri(j, i)];
#pragma unroll
      for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
      L[i][j] = v / ljj;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double v = -g[i];
#pragma unroll
    for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) v = v - L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
  return ok;
}

// one corner slot: its point in the field frame and its pixel
struct FpSlot {
  double X[3];
  double u, v;
  bool valid;
};

// squared reprojection error of one slot under (R, t); *behind: its Z is not positive
AT_FP_HD double fp_slot_cost(const FpSlot& s, const FpCam& cam, const double* R, const double* t, bool* behind) {
  *behind = false;
  if (!s.valid) return 0.0;
  double Q[3];
  fp_rot(R, s.X, Q);
  const double Px = Q[0] + t[0], Py = Q[1] + t[1], Pz = Q[2] + t[2];
  *behind = !(Pz > 0.0);
  const double ru = (cam.fx * (Px / Pz) + cam.cx) - s.u;
  const double rv = (cam.fy * (Py / Pz) + cam.cy) - s.v;
  return ru * ru + rv * rv;
}

// the slot's two residual rows: its 21 J^T J products (upper triangle) and 6 J^T r
AT_FP_HD void fp_slot_normal(const FpSlot& s, const FpCam& cam, const double* R, const double* t, double* a,
                             double* g) {
  if (!s.valid) {
#pragma unroll
    for (int k = 0; k < 21; k++) a[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) g[k] = 0.0;
    return;
  }
  double Q[3];
  fp_rot(R, s.X, Q);
  const double Px = Q[0] + t[0], Py = Q[1] + t[1], Pz = Q[2] + t[2];
  const double xn = Px / Pz, yn = Py / Pz;
  const double ru = (cam.fx * xn + cam.cx) - s.u;
  const double rv = (cam.fy * yn + cam.cy) - s.v;
  // du/dP = (A, 0, B), dv/dP = (0, C, D); dP/dw = -[Q]x, dP/dt = I
  const double A = cam.fx / Pz, B = -(cam.fx * xn) / Pz;
  const double C = cam.fy / Pz, D = -(cam.fy * yn) / Pz;
  const double ju[6] = {B * Q[1], A * Q[2] - B * Q[0], -(A * Q[1]), A, 0.0, B};
  const double jv[6] = {D * Q[1] - C * Q[2], -(D * Q[0]), C * Q[0], 0.0, C, D};
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = i; j < 6; j++) a[fp_tri(i, j)] = ju[i] * ju[j] + jv[i] * jv[j];
    g[i] = ju[i] * ru + jv[i] * rv;
  }
}

// The 64 slots held by one host thread.
struct FpHostWave {
  static constexpr int NS = kFpSlots;
  int slot(int s) const { return s; }
  bool leader() const { return true; }
  double sum(const double* v) const {
    double a[kFpSlots];
    for (int i = 0; i < kFpSlots; i++) a[i] = v[i];
    for (int off = kFpSlots / 2; off >= 1; off >>= 1)
      for (int i = 0; i < off; i++) a[i] = a[i] + a[i + off];
    return a[0];
  }
  bool any(const bool* f) const {
    bool r = false;
    for (int i = 0; i < kFpSlots; i++) r = r || f[i];
    return r;
  }
  uint64_t min(const uint64_t* v) const {
    uint64_t r = v[0];
    for (int i = 1; i < kFpSlots; i++) r = v[i] < r ? v[i] : r;
    return r;
  }
  uint32_t from_slot(const uint32_t* v, int slot) const { return v[slot]; }
};

// cost of all slots under (R, t): infinite with a point at Z <= 0
template <class W>
AT_FP_HD double fp_cost(const W& w, const FpSlot* slots, const FpCam& cam, const double* R, const double* t,
                        bool* behind) {
  double e[W::NS];
  bool b[W::NS];
#pragma unroll
  for (int s = 0; s < W::NS; s++) e[s] = fp_slot_cost(slots[s], cam, R, t, &b[s]);
  *behind = w.any(b);
  return w.sum(e);
}

// ---- select: the best candidate of each of the 16 lowest layout ids ----
// Slot 4j + c ends with the candidate (my_cand) and id (my_id) of the j-th selected tag; *m_out
// tags were selected, *dropped_out eligible candidates had an id beyond them.  (k_rig and its
// twin run this once per camera: at_rigpose.h.)
template <class W, class Src>
AT_FP_HD void fp_select(const W& w, const Src& src, const FpLayout& lay, uint32_t* my_cand, uint32_t* my_id,
                        int* m_out, int* dropped_out) {
  const int n = src.n() < kFpMaxCand ? src.n() : kFpMaxCand;
#pragma unroll
  for (int s = 0; s < W::NS; s++) my_cand[s] = my_id[s] = 0;
  // (a slot's first candidate, the only one in a frame of up to 64, is read once; the rounds
  // reread the records only beyond it)
  uint64_t first[W::NS];
#pragma unroll
  for (int s = 0; s < W::NS; s++) {
    const int c = w.slot(s);
    first[s] = c < n ? fp_key(lay, src.id(c), src.hamming(c), src.margin(c), (uint32_t)c) : kFpNoKey;
  }
  uint64_t floor_key = 0;
  int m = 0, dropped = 0;
  for (int j = 0; j <= kFpMaxTags; j++) {
    uint64_t loc[W::NS];
    double cnt[W::NS];
#pragma unroll
    for (int s = 0; s < W::NS; s++) {
      loc[s] = kFpNoKey;
      cnt[s] = 0.0;
      for (int c = w.slot(s); c < n; c += kFpSlots) {
        const uint64_t k = c < kFpSlots ? first[s]
                                        : fp_key(lay, src.id(c), src.hamming(c), src.margin(c), (uint32_t)c);
        if (k == kFpNoKey || k < floor_key) continue;
        cnt[s] = cnt[s] + 1.0;
        if (k < loc[s]) loc[s] = k;
      }
    }
    const uint64_t best = w.min(loc);
    if (j == kFpMaxTags || best == kFpNoKey) {
      dropped = (int)w.sum(cnt);  // what is left beyond the 16th id was dropped by the cap
      break;
    }
#pragma unroll
    for (int s = 0; s < W::NS; s++)
      if ((w.slot(s) >> 2) == j) {
        my_cand[s] = (uint32_t)(best & 0xffffu);
        my_id[s] = (uint32_t)(best >> 52);
      }
    m++;
    floor_key = ((best >> 52) + 1) << 52;
  }
  *m_out = m;
  *dropped_out = dropped;
}

// ---- points: each slot's corner in the field frame and its pixel ----
template <class W, class Src>
AT_FP_HD void fp_points(const W& w, const Src& src, const FpLayout& lay, double tag_size, int m,
                        const uint32_t* my_cand, const uint32_t* my_id, FpSlot* slots) {
  const double hs = tag_size / 2.0;
#pragma unroll
  for (int s = 0; s < W::NS; s++) {
    const int sl = w.slot(s), j = sl >> 2, c = sl & 3;
    FpSlot& q = slots[s];
    q.valid = j < m;
    q.X[0] = q.X[1] = q.X[2] = q.u = q.v = 0.0;
    if (q.valid) {
      const FpTag& tg = lay.tags[lay.lut[my_id[s]]];
      const double sx = (c == 0 || c == 3) ? -hs : hs, sy = c < 2 ? hs : -hs;  // estimate_tag_pose's corners
      for (int k = 0; k < 3; k++) q.X[k] = (tg.R[k * 3] * sx + tg.R[k * 3 + 1] * sy) + tg.t[k];
      const double* p = src.p((int)my_cand[s]);
      q.u = p[c * 2];
      q.v = p[c * 2 + 1];
    }
  }
}

// Src: the frame's candidates -- n(), id(c), hamming(c), margin(c), p(c) (8 doubles:
// the four corners' pixels), pose_R(c) (9), pose_t(c) (3).
// Every thread of the wave ends with the same record; the leader stores it to out (and
// out2 when given).
template <class W, class Src>
AT_FP_HD void fp_solve_frame(const W& w, const Src& src, const FpLayout& lay, const FpCam& cam, double tag_size,
                             FpRecord* out, FpRecord* out2) {
  uint32_t my_cand[W::NS], my_id[W::NS];
  int m, dropped;
  fp_select(w, src, lay, my_cand, my_id, &m, &dropped);
  FpSlot slots[W::NS];
  fp_points(w, src, lay, tag_size, m, my_cand, my_id, slots);

  // ---- start: the single-tag pose with the least total error ----
  double R[9], t[3];
  double cost = HUGE_VAL;
  bool found = false;
  for (int j = 0; j < m; j++) {
    const int c = (int)w.from_slot(my_cand, 4 * j);
    const FpTag& tg = lay.tags[lay.lut[w.from_slot(my_id, 4 * j)]];
    double Rj[9], tj[3], rt[3];
    fp_mul_abt(src.pose_R(c), tg.R, Rj);
    fp_rot(Rj, tg.t, rt);
    const double* pt = src.pose_t(c);
    for (int k = 0; k < 3; k++) tj[k] = pt[k] - rt[k];
    bool behind;
    const double cj = fp_cost(w, slots, cam, Rj, tj, &behind);
    if (!behind && cj < cost) {  // (a NaN never wins; ties stay with the lower id)
      cost = cj;
      found = true;
      for (int k = 0; k < 9; k++) R[k] = Rj[k];
      for (int k = 0; k < 3; k++) t[k] = tj[k];
    }
  }
  if (!found) {  // no layout tag in the frame, or none whose pose puts every point in front
    if (w.leader()) {
      FpRecord z = {};
      z.dropped = dropped;
      *out = z;
      if (out2) *out2 = z;
    }
    return;
  }
  fp_project_rotation(R);
  {
    bool behind;
    const double c0 = fp_cost(w, slots, cam, R, t, &behind);
    if (!behind && c0 == c0) cost = c0;  // (else: the start's own cost bounds the first step)
  }

  // ---- refine: kFpIters Levenberg-Marquardt iterations on the pixel residuals ----
  double lambda = 1e-3;
  int steps = 0, rejected = 0;
  for (int it = 0; it < kFpIters; it++) {
    double a[21], g[6];
    {
      double pa[W::NS][21], pg[W::NS][6];
#pragma unroll
      for (int s = 0; s < W::NS; s++) fp_slot_normal(slots[s], cam, R, t, pa[s], pg[s]);
#pragma unroll
      for (int k = 0; k < 21; k++) {
        double col[W::NS];
#pragma unroll
        for (int s = 0; s < W::NS; s++) col[s] = pa[s][k];
        a[k] = w.sum(col);
      }
#pragma unroll
      for (int k = 0; k < 6; k++) {
        double col[W::NS];
#pragma unroll
        for (int s = 0; s < W::NS; s++) col[s] = pg[s][k];
        g[k] = w.sum(col);
      }
    }
    double d[6], Rn[9], tn[3];
    bool take = fp_solve6(a, g, lambda, d);
    double cn = HUGE_VAL;
    if (take) {
      fp_apply_step(R, t, d, Rn, tn);
      bool behind;
      cn = fp_cost(w, slots, cam, Rn, tn, &behind);
      take = !behind && cn < cost;
    }
    if (take) {
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
  const double rms = sqrt(cost / (double)(4 * m));

  // ---- the record ----
  for (int j = 0; j < kFpMaxTags; j++) {
    const int32_t id = j < m ? (int32_t)w.from_slot(my_id, 4 * j) : 0;
    if (w.leader()) {
      out->ids[j] = id;
      if (out2) out2->ids[j] = id;
    }
  }
  if (w.leader()) {
    for (int k = 0; k < 2; k++) {
      FpRecord* o = k ? out2 : out;
      if (!o) continue;
      o->n_tags = m;
      for (int i = 0; i < 9; i++) o->R[i] = R[i];
      for (int i = 0; i < 3; i++) o->t[i] = t[i];
      o->rms_px = rms;
      o->steps_taken = steps;
      o->rejected = rejected;
      o->dropped = dropped;
      o->pad = 0;
    }
  }
}

}  // namespace at
