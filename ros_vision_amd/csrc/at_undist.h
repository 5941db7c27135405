// at_undist.h -- ideal corners: the lens distortion undone before the pose solves, shared by
// host and device.
//
// Every pose solve of this project projects through a pinhole.  A pinhole projection compared
// with the *ideal* pixel is the same model as the distorting projection compared with the raw
// pixel, the ideal pixel being the raw one mapped through the exact inverse of the forward
// model (k_decode's redistort, at_camcal.h's cc_distort):
//   x'' = x lin + 2 p1 x y + p2 (r2 + 2 x^2),  y'' = y lin + p1 (r2 + 2 y^2) + 2 p2 x y,
//   lin = 1 + k1 r2 + k2 r2^2 + k3 r2^3,       u = fx x'' + cx,  v = fy y'' + cy.
// und_point inverts it; und_detection turns a detection's corners into ideal corners and
// recomputes its homography and centre from them.  The kernels (at_kernels.hip: the head of
// k_pose and of the pose wave of k_decode, k_und_points) and the CPU twins (at_undist.cpp:
// at_ideal_detections_host, at_undistort_points_host) share this text, under at_fieldpose.h's
// rules: no contraction, only + - * / and comparisons, a fixed operation order -- so device
// and host agree bit for bit.
//
// (k_decode's own `undistort` is not this inverse: it carries the reference's p2 term and a
// data-dependent loop, and serves the edge-line fit only.)
#pragma once

#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define AT_UND_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define AT_UND_HD static inline
#endif

namespace at {

constexpr int kUndIters = 8;        // Newton steps, fixed (no early exit); four reach the rounding floor
constexpr double kUndTolPx = 1e-6;  // the result's forward image lies this close to the raw pixel, per axis

// at_camera's fields in at_camera's order
struct UndCam { double fx, fy, cx, cy, k1, k2, p1, p2, k3; };

// The ideal record of one candidate slot: the detection's H, c and p from ideal corners, and its
// id, or the raw values with id = -1 when a corner is not invertible.
struct UndRecord {
  double H[9];
  double c[2];
  double p[4][2];
  int32_t id;
  int32_t pad;
};
static_assert(sizeof(UndRecord) == 160, "UndRecord: 160 B per candidate slot");

// no distortion at all: the stage is a copy
AT_UND_HD bool und_identity(const UndCam& c) {
  return c.k1 == 0.0 && c.k2 == 0.0 && c.p1 == 0.0 && c.p2 == 0.0 && c.k3 == 0.0;
}

// the forward model on a normalised point, with its Jacobian (J[0] = dx''/dx, J[1] = dx''/dy =
// dy''/dx, J[2] = dy''/dy: it is symmetric)
AT_UND_HD void und_forward(const UndCam& c, double x, double y, double* xd, double* yd, double* J) {
  const double xx = x * x, yy = y * y, xy = x * y;
  const double r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2;
  const double lin = ((1.0 + c.k1 * r2) + c.k2 * r4) + c.k3 * r6;
  const double dl = (c.k1 + 2.0 * c.k2 * r2) + 3.0 * c.k3 * r4;  // d lin / d r2
  *xd = (x * lin + 2.0 * c.p1 * xy) + c.p2 * (r2 + 2.0 * xx);
  *yd = (y * lin + c.p1 * (r2 + 2.0 * yy)) + 2.0 * c.p2 * xy;
  J[0] = ((lin + 2.0 * xx * dl) + 2.0 * c.p1 * y) + 6.0 * c.p2 * x;
  J[1] = (2.0 * xy * dl + 2.0 * c.p1 * x) + 2.0 * c.p2 * y;
  J[2] = ((lin + 2.0 * yy * dl) + 6.0 * c.p1 * y) + 2.0 * c.p2 * x;
}

// The ideal pixel (*ou, *ov) of the raw pixel (u, v): kUndIters Newton steps from the raw
// normalised point.  false -- the point is not invertible, (*ou, *ov) = (u, v) -- when the
// Jacobian's determinant is not > 0 at an iterate or at the result (the model has folded over),
// or the result's forward image is not within kUndTolPx of (u, v) on each axis; a NaN fails both.
// The ideal pixel is the raw one plus fx (x - x0): without distortion it is the raw pixel itself.
AT_UND_HD bool und_point(const UndCam& c, double u, double v, double* ou, double* ov) {
  const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
  double x = x0, y = y0;
  bool ok = true;
  for (int it = 0; it < kUndIters; it++) {
    double xd, yd, J[3];
    und_forward(c, x, y, &xd, &yd, J);
    const double det = J[0] * J[2] - J[1] * J[1];
    if (!(det > 0.0)) ok = false;
    const double rx = xd - x0, ry = yd - y0;
    x = x - (J[2] * rx - J[1] * ry) / det;
    y = y - (J[0] * ry - J[1] * rx) / det;
  }
  double xd, yd, J[3];
  und_forward(c, x, y, &xd, &yd, J);
  const double det = J[0] * J[2] - J[1] * J[1];
  if (!(det > 0.0)) ok = false;
  const double eu = (xd * c.fx + c.cx) - u, ev = (yd * c.fy + c.cy) - v;
  if (!(eu <= kUndTolPx && eu >= -kUndTolPx)) ok = false;
  if (!(ev <= kUndTolPx && ev >= -kUndTolPx)) ok = false;
  *ou = ok ? u + c.fx * (x - x0) : u;
  *ov = ok ? v + c.fy * (y - y0) : v;
  return ok;
}

// tag coordinates of corner i of a detection record (at_detection.p[i] = H (tx, ty))
AT_UND_HD double und_tx(int i) { return (i == 1 || i == 2) ? 1.0 : -1.0; }
AT_UND_HD double und_ty(int i) { return i < 2 ? 1.0 : -1.0; }

// rows 2i and 2i + 1 of the 8 x 9 system of corner i at pixel (px, py)
AT_UND_HD void und_rows(int i, double px, double py, double* r0, double* r1) {
  const double tx = und_tx(i), ty = und_ty(i);
  r0[0] = tx; r0[1] = ty; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0;
  r0[6] = -tx * px; r0[7] = -ty * px; r0[8] = px;
  r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = tx; r1[4] = ty; r1[5] = 1.0;
  r1[6] = -tx * py; r1[7] = -ty * py; r1[8] = py;
}

// H with H (tx, ty)_i = p[i], by homography_compute2's elimination (apriltag 3.x
// common/homography.c): per column the pivot is the first row holding the strict maximum of
// |A[row][col]|, a maximum under 1e-10 (or no number) is singular (-1).  A: 72 doubles of
// workspace.  This serial form is the definition; the kernels spread the same per-element
// sequence of operations over lanes (homography_wave, und_homography_quad).
AT_UND_HD int und_homography(const double (*p)[2], double* A, double* H) {
  for (int i = 0; i < 4; i++) und_rows(i, p[i][0], p[i][1], A + (2 * i) * 9, A + (2 * i + 1) * 9);
  for (int col = 0; col < 8; col++) {
    double max_val = 0.0;
    int max_idx = -1;
    for (int row = col; row < 8; row++) {
      const double a = A[row * 9 + col];
      const double v = a < 0.0 ? -a : a;
      if (v > max_val) { max_val = v; max_idx = row; }
    }
    if (!(max_val >= 1e-10)) return -1;
    if (max_idx != col)
      for (int i = col; i < 9; i++) {
        const double t = A[col * 9 + i];
        A[col * 9 + i] = A[max_idx * 9 + i];
        A[max_idx * 9 + i] = t;
      }
    for (int i = col + 1; i < 8; i++) {
      const double f = A[i * 9 + col] / A[col * 9 + col];
      for (int j = col + 1; j < 9; j++) A[i * 9 + j] = A[i * 9 + j] - f * A[col * 9 + j];
    }
  }
  for (int col = 7; col >= 0; col--) {
    double sum = 0.0;
    for (int i = col + 1; i < 8; i++) sum = sum + A[col * 9 + i] * A[i * 9 + 8];
    A[col * 9 + 8] = (A[col * 9 + 8] - sum) / A[col * 9 + col];
  }
  for (int k = 0; k < 8; k++) H[k] = A[k * 9 + 8];
  H[8] = 1.0;
  return 0;
}

// the centre: the image of (0, 0) under H
AT_UND_HD void und_centre(const double* H, double* c) {
  c[0] = H[2] / H[8];
  c[1] = H[5] / H[8];
}

// The ideal record of a raw detection (its H, c, p and id).  Without distortion a copy; with a
// corner that is not invertible, or a singular system, the raw values with id = -1.  A: 72
// doubles of workspace.
AT_UND_HD void und_detection(const UndCam& cam, const double* H, const double* c, const double (*p)[2], int32_t id,
                             double* A, UndRecord* out) {
  bool ok = true;
  double q[4][2];
  const bool ident = und_identity(cam);
  if (!ident) {
    for (int i = 0; i < 4; i++)
      if (!und_point(cam, p[i][0], p[i][1], &q[i][0], &q[i][1])) ok = false;
    if (ok && und_homography(q, A, out->H) != 0) ok = false;
  }
  if (ident || !ok) {
    for (int k = 0; k < 9; k++) out->H[k] = H[k];
    out->c[0] = c[0];
    out->c[1] = c[1];
    for (int i = 0; i < 4; i++) { out->p[i][0] = p[i][0]; out->p[i][1] = p[i][1]; }
    out->id = ident ? id : -1;
  } else {
    und_centre(out->H, out->c);
    for (int i = 0; i < 4; i++) { out->p[i][0] = q[i][0]; out->p[i][1] = q[i][1]; }
    out->id = id;
  }
  out->pad = 0;
}

}  // namespace at
