// undistort_host_check.cpp -- at_undistort_points_host / at_ideal_detections_host driven
// stand-alone, for a build with -fsanitize=address,undefined (tests/test_undistort_host.py builds
// and runs it).  Every array is a heap buffer of exactly the size the call may touch.  Prints
// "ok <points checked> <detections made ideal> <not invertible> <calls refused>".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/at_api.h"

// two 1280 x 800 lenses with round coefficients: one like the deployed cam11 (regular over the whole
// frame), one like cam14, whose k3 folds the model over at the frame's corners
static const at_camera kCam11 = {895.0, 894.0, 647.5, 409.0, 0.006, 0.039, -0.006, -0.0006, -0.146};
static const at_camera kCam14 = {900.0, 900.0, 665.0, 405.0, 0.023, 0.13, 0.0009, 0.0021, -0.395};
static const at_camera kNone = {900.0, 900.0, 640.0, 400.0, 0, 0, 0, 0, 0};

static int fail(const char* what) {
  printf("FAILED: %s\n", what);
  return 1;
}

static void forward(const at_camera& c, double u, double v, double* ru, double* rv) {
  const double x = (u - c.cx) / c.fx, y = (v - c.cy) / c.fy;
  const double r2 = x * x + y * y;
  const double lin = 1 + c.k1 * r2 + c.k2 * r2 * r2 + c.k3 * r2 * r2 * r2;
  *ru = c.fx * (x * lin + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x)) + c.cx;
  *rv = c.fy * (y * lin + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y) + c.cy;
}

// a 16-px grid of a 1280 x 800 frame: every point of cam11 comes back ok and maps forward onto
// itself; without distortion every point comes back itself
static int points(int* checked) {
  const int nx = 80, ny = 50, n = nx * ny;
  double* xy = (double*)malloc(sizeof(double) * 2 * (size_t)n);
  double* out = (double*)malloc(sizeof(double) * 2 * (size_t)n);
  uint8_t* ok = (uint8_t*)malloc((size_t)n);
  if (!xy || !out || !ok) return fail("malloc");
  for (int i = 0; i < n; i++) {
    xy[2 * i] = 16.0 * (i % nx);
    xy[2 * i + 1] = 16.0 * (i / nx);
  }
  int bad = 0;
  if (at_undistort_points_host(&kCam11, xy, n, out, ok) != n) bad = fail("at_undistort_points_host");
  for (int i = 0; !bad && i < n; i++) {
    double ru, rv;
    forward(kCam11, out[2 * i], out[2 * i + 1], &ru, &rv);
    if (!ok[i] || !(fabs(ru - xy[2 * i]) <= 1e-9) || !(fabs(rv - xy[2 * i + 1]) <= 1e-9)) bad = fail("cam11 point");
  }
  if (!bad && at_undistort_points_host(&kNone, xy, n, out, ok) != n) bad = fail("no distortion");
  if (!bad && memcmp(xy, out, sizeof(double) * 2 * (size_t)n) != 0) bad = fail("no distortion: not a copy");
  // cam14: the frame's corner is flagged and comes back raw; NaN and infinity are flagged
  double* q = (double*)malloc(sizeof(double) * 8);
  const double in[8] = {0.0, 0.0, 640.0, 400.0, NAN, 5.0, 7.0, INFINITY};
  memcpy(q, in, sizeof(in));
  if (!bad && at_undistort_points_host(&kCam14, q, 4, out, ok) != 4) bad = fail("cam14");
  if (!bad && (ok[0] || !ok[1] || ok[2] || ok[3] || out[0] != 0.0 || out[1] != 0.0)) bad = fail("cam14 flags");
  if (!bad && at_undistort_points_host(&kCam14, q, 0, nullptr, nullptr) != 0) bad = fail("n = 0");
  free(q);
  free(xy);
  free(out);
  free(ok);
  *checked = 2 * n + 4;
  return bad;
}

// detections of cam14 marching from the centre to the corner of the frame: the ideal H maps
// (+-1, +-1) onto the ideal corners, and the ones that reach the fold come back raw with id = -1
static int detections(int* ideal, int* flagged) {
  const int n = 12;
  at_detection* d = (at_detection*)malloc(sizeof(at_detection) * (size_t)n);
  at_detection* o = (at_detection*)malloc(sizeof(at_detection) * (size_t)n);
  if (!d || !o) return fail("malloc");
  memset(d, 0, sizeof(at_detection) * (size_t)n);
  const double tx[4] = {-1, 1, 1, -1}, ty[4] = {1, 1, -1, -1};
  for (int k = 0; k < n; k++) {
    const double cx = 640.0 - 52.0 * k, cy = 400.0 - 32.0 * k, h = 30.0;
    d[k].id = k;
    d[k].hamming = k & 1;
    d[k].decision_margin = 40.0f + (float)k;
    const double H[9] = {h, 0, cx, 0, -h, cy, 0, 0, 1};
    memcpy(d[k].H, H, sizeof(H));
    d[k].c[0] = cx;
    d[k].c[1] = cy;
    for (int i = 0; i < 4; i++) {
      d[k].p[i][0] = cx + h * tx[i];
      d[k].p[i][1] = cy - h * ty[i];
    }
  }
  int bad = 0;
  if (at_ideal_detections_host(&kCam14, d, n, o) != n) bad = fail("at_ideal_detections_host");
  for (int k = 0; !bad && k < n; k++) {
    if (o[k].hamming != d[k].hamming || o[k].decision_margin != d[k].decision_margin) bad = fail("carried fields");
    if (o[k].id == -1) {
      if (memcmp(o[k].H, d[k].H, sizeof(d[k].H)) || memcmp(o[k].p, d[k].p, sizeof(d[k].p)) ||
          memcmp(o[k].c, d[k].c, sizeof(d[k].c)))
        bad = fail("a flagged detection is not raw");
      ++*flagged;
      continue;
    }
    if (o[k].id != k) bad = fail("id");
    for (int i = 0; !bad && i < 4; i++) {
      const double* H = o[k].H;
      const double z = H[6] * tx[i] + H[7] * ty[i] + H[8];
      const double x = (H[0] * tx[i] + H[1] * ty[i] + H[2]) / z, y = (H[3] * tx[i] + H[4] * ty[i] + H[5]) / z;
      if (!(fabs(x - o[k].p[i][0]) <= 1e-9) || !(fabs(y - o[k].p[i][1]) <= 1e-9)) bad = fail("H does not map onto p");
      double ru, rv;
      forward(kCam14, o[k].p[i][0], o[k].p[i][1], &ru, &rv);
      if (!(fabs(ru - d[k].p[i][0]) <= 1e-6) || !(fabs(rv - d[k].p[i][1]) <= 1e-6)) bad = fail("p is not the inverse image");
    }
    ++*ideal;
  }
  // without distortion: a copy, in place
  if (!bad && at_ideal_detections_host(&kNone, d, n, d) != n) bad = fail("in place");
  free(d);
  free(o);
  return bad;
}

static int refusals(int* refused) {
  double xy[2] = {1, 2}, out[2];
  uint8_t ok;
  at_detection d, o;
  memset(&d, 0, sizeof(d));
  at_camera zero = kCam11;
  zero.fx = 0;
  *refused += at_undistort_points_host(nullptr, xy, 1, out, &ok) == AT_E_INVALID;
  *refused += at_undistort_points_host(&zero, xy, 1, out, &ok) == AT_E_INVALID;
  *refused += at_undistort_points_host(&kCam11, nullptr, 1, out, &ok) == AT_E_INVALID;
  *refused += at_undistort_points_host(&kCam11, xy, 1, nullptr, &ok) == AT_E_INVALID;
  *refused += at_undistort_points_host(&kCam11, xy, 1, out, nullptr) == AT_E_INVALID;
  *refused += at_undistort_points_host(&kCam11, xy, -1, out, &ok) == AT_E_INVALID;
  *refused += at_ideal_detections_host(nullptr, &d, 1, &o) == AT_E_INVALID;
  *refused += at_ideal_detections_host(&kCam11, nullptr, 1, &o) == AT_E_INVALID;
  *refused += at_ideal_detections_host(&kCam11, &d, 1, nullptr) == AT_E_INVALID;
  *refused += at_ideal_detections_host(&kCam11, &d, -1, &o) == AT_E_INVALID;
  return 0;
}

int main() {
  int checked = 0, ideal = 0, flagged = 0, refused = 0;
  if (points(&checked) || detections(&ideal, &flagged) || refusals(&refused)) return 1;
  printf("ok %d %d %d %d\n", checked, ideal, flagged, refused);
  return (refused == 10 && ideal > 0 && flagged > 0 && ideal + flagged == 12) ? 0 : 1;
}
