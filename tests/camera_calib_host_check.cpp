// camera_calib_host_check.cpp -- the camera calibrator's host side driven stand-alone, for a build
// with -fsanitize=address,undefined (tests/test_camera_calib_host.py builds and runs it): create
// and its refusals, add from heap buffers of exactly the size the call may touch (a frame without
// a board tag, an empty frame from a NULL array), at_camcal_solve_host with and without the focal
// guess, the view records, clear and destroy.  Prints "ok <views stored> <frames not stored>
// <calls refused>".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/at_api.h"

static const double kTag = 0.1, kPitch = 0.14;
static const int kRows = 3, kCols = 4, kViews = 35;
static const at_camera kTrue = {610.0, 605.0, 331.0, 236.0, 0.05, -0.08, 0.001, -0.002, 0.02};

static void rot(double rx, double ry, double rz, double* R) {  // Rz Ry Rx
  const double cx = cos(rx), sx = sin(rx), cy = cos(ry), sy = sin(ry), cz = cos(rz), sz = sin(rz);
  const double M[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                       sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                       -sy,     cy * sx,                cy * cx};
  memcpy(R, M, sizeof(M));
}

static int fail(const char* what) {
  printf("FAILED: %s\n", what);
  return 1;
}

static void project(const at_camera& c, const double* R, const double* t, const double* X, double* uv) {
  double P[3];
  for (int r = 0; r < 3; r++) P[r] = R[r * 3] * X[0] + R[r * 3 + 1] * X[1] + R[r * 3 + 2] * X[2] + t[r];
  const double x = P[0] / P[2], y = P[1] / P[2], r2 = x * x + y * y;
  const double lin = 1 + c.k1 * r2 + c.k2 * r2 * r2 + c.k3 * r2 * r2 * r2;
  uv[0] = c.fx * (x * lin + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x)) + c.cx;
  uv[1] = c.fy * (y * lin + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y) + c.cy;
}

// the map of (-1, 1), (1, 1), (1, -1), (-1, -1) onto p by Gaussian elimination with pivoting
static void homography(const double p[4][2], double* H) {
  static const double sx[4] = {-1, 1, 1, -1}, sy[4] = {1, 1, -1, -1};
  double A[8][9];
  for (int k = 0; k < 4; k++) {
    const double u = p[k][0], v = p[k][1];
    const double r0[9] = {sx[k], sy[k], 1, 0, 0, 0, -u * sx[k], -u * sy[k], u};
    const double r1[9] = {0, 0, 0, sx[k], sy[k], 1, -v * sx[k], -v * sy[k], v};
    memcpy(A[2 * k], r0, sizeof(r0));
    memcpy(A[2 * k + 1], r1, sizeof(r1));
  }
  for (int c = 0; c < 8; c++) {
    int piv = c;
    for (int r = c + 1; r < 8; r++)
      if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
    for (int k = 0; k < 9; k++) {
      const double tmp = A[c][k];
      A[c][k] = A[piv][k];
      A[piv][k] = tmp;
    }
    for (int r = 0; r < 8; r++) {
      if (r == c) continue;
      const double f = A[r][c] / A[c][c];
      for (int k = c; k < 9; k++) A[r][k] -= f * A[c][k];
    }
  }
  for (int k = 0; k < 8; k++) H[k] = A[k][8] / A[k][k];
  H[8] = 1.0;
}

// One view of the board at pose number s: the tags with index < n_seen, exact corners, plus one
// detection of an id the board does not have.  Returns at_camcal_add's value.
static int add_view(at_camcal* cal, const std::vector<at_field_tag>& board, int s, int n_seen) {
  double R[9];
  rot(0.35 * sin(1.3 * s), 0.4 * cos(0.9 * s), 0.1 * s, R);
  const double centre[3] = {1.5 * kPitch, kPitch, 0.0};
  double t[3] = {0.02 * sin(0.7 * s), 0.015 * cos(1.1 * s), 0.85 + 0.01 * (s % 5)};
  for (int r = 0; r < 3; r++) t[r] -= R[r * 3] * centre[0] + R[r * 3 + 1] * centre[1] + R[r * 3 + 2] * centre[2];
  const int n = n_seen + 1;
  at_detection* dets = (at_detection*)malloc(sizeof(at_detection) * (size_t)n);  // exactly n records
  if (!dets) return -100;
  memset(dets, 0, sizeof(at_detection) * (size_t)n);
  static const double sx[4] = {-1, 1, 1, -1}, sy[4] = {1, 1, -1, -1};
  for (int k = 0; k < n; k++) {
    const at_field_tag& g = board[(size_t)(k < n_seen ? k : 0)];
    at_detection& d = dets[k];
    d.id = k < n_seen ? g.id : 900;
    d.hamming = 0;
    d.decision_margin = 50.0f + (float)k;
    for (int c = 0; c < 4; c++) {
      const double X[3] = {g.t[0] + sx[c] * kTag / 2, g.t[1] + sy[c] * kTag / 2, 0.0};
      project(kTrue, R, t, X, d.p[c]);
    }
    homography(d.p, d.H);
    d.c[0] = d.H[2];
    d.c[1] = d.H[5];
  }
  const int rc = at_camcal_add(cal, dets, n);
  free(dets);
  return rc;
}

int main() {
  std::vector<at_field_tag> board((size_t)(kRows * kCols));
  for (int r = 0; r < kRows; r++)
    for (int c = 0; c < kCols; c++) {
      at_field_tag& g = board[(size_t)(r * kCols + c)];
      memset(&g, 0, sizeof(g));
      g.id = 10 + r * kCols + c;
      g.R[0] = g.R[4] = g.R[8] = 1.0;
      g.t[0] = c * kPitch;
      g.t[1] = r * kPitch;
    }
  at_camcal_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.width = 640;
  cfg.height = 480;
  cfg.init = kTrue;
  cfg.init.fx *= 1.1;
  cfg.init.fy *= 0.9;
  cfg.init.cx += 15;
  cfg.init.k1 = cfg.init.k2 = cfg.init.p1 = cfg.init.p2 = cfg.init.k3 = 0.0;
  cfg.free_mask = 511;
  cfg.guess = 0;

  int refused = 0;
  at_camcal* cal = nullptr;
  {  // the refusals of create
    at_camcal_config bad = cfg;
    bad.free_mask = 512;
    refused += at_camcal_create(&bad, board.data(), (int)board.size(), 0, kTag, &cal) == AT_E_INVALID;
    bad = cfg;
    bad.free_mask = -1;
    refused += at_camcal_create(&bad, board.data(), (int)board.size(), 0, kTag, &cal) == AT_E_INVALID;
    bad = cfg;
    bad.width = 0;
    refused += at_camcal_create(&bad, board.data(), (int)board.size(), 0, kTag, &cal) == AT_E_INVALID;
    bad = cfg;
    bad.init.fy = 0.0;
    refused += at_camcal_create(&bad, board.data(), (int)board.size(), 0, kTag, &cal) == AT_E_INVALID;
    refused += at_camcal_create(&cfg, board.data(), (int)board.size(), 0, 0.0, &cal) == AT_E_INVALID;
    refused += at_camcal_create(&cfg, board.data(), (int)board.size(), -1, kTag, &cal) == AT_E_INVALID;
    std::vector<at_field_tag> twice = board;
    twice[1].id = twice[0].id;
    refused += at_camcal_create(&cfg, twice.data(), (int)twice.size(), 0, kTag, &cal) == AT_E_INVALID;
    refused += at_camcal_create(&cfg, board.data(), 0, 0, kTag, &cal) == AT_E_INVALID;
    if (cal) return fail("a refused create left a handle");
  }
  if (at_camcal_create(&cfg, board.data(), (int)board.size(), 1, kTag, &cal) != AT_OK) return fail("create");
  at_camcal_result res;
  refused += at_camcal_solve_host(cal, &res) == AT_E_INVALID;  // no stored view

  int stored = 0, not_stored = 0;
  for (int s = 0; s < kViews; s++) {
    const int rc = add_view(cal, board, s, s == 7 ? 0 : 4 + s % 9);  // view 7: only the foreign id
    if (rc == 1) stored++;
    else if (rc == 0) not_stored++;
    else return fail("add");
  }
  {
    const int rc = at_camcal_add(cal, nullptr, 0);  // an empty frame
    if (rc != 0) return fail("empty add");
    not_stored++;
  }
  if (at_camcal_count(cal) != stored) return fail("count");
  if (at_camcal_solve_host(cal, &res) != AT_OK) return fail("solve_host");
  if (res.views_used != stored || !res.cov_valid || !(res.rms_after < 1e-6) || !(res.rms_before > 1.0))
    return fail("result");
  const double* got = &res.cam.fx;
  const double* want = &kTrue.fx;
  for (int k = 0; k < 9; k++)
    if (!(fabs(got[k] - want[k]) <= 1e-6 * (k < 4 ? 1000.0 : 1.0))) return fail("camera");
  {
    const int n = at_camcal_views(cal, nullptr, 0);
    if (n != stored) return fail("views count");
    at_camcal_view* v = (at_camcal_view*)malloc(sizeof(at_camcal_view) * (size_t)n);  // exactly n records
    if (!v || at_camcal_views(cal, v, n) != n) return fail("views");
    for (int i = 0; i < n; i++)
      if (!v[i].used || v[i].n_tags < 4 || !(v[i].rms_px < 1e-6) || !(v[i].t[2] > 0)) return fail("view record");
    free(v);
  }
  uint64_t st[5];
  if (at_camcal_stats(cal, st, 5) != 5 || st[0] != (uint64_t)stored || st[4] != 0) return fail("stats");
  if (at_camcal_clear(cal) != AT_OK || at_camcal_count(cal) != 0) return fail("clear");
  refused += at_camcal_solve_host(cal, &res) == AT_E_INVALID;
  at_camcal_destroy(cal);

  // no initial camera: the focal guess, the four pinhole values free, exact pinhole corners
  cfg.guess = 1;
  cfg.free_mask = 15;
  memset(&cfg.init, 0, sizeof(cfg.init));
  if (at_camcal_create(&cfg, board.data(), (int)board.size(), 0, kTag, &cal) != AT_OK) return fail("create (guess)");
  for (int s = 0; s < 6; s++)
    if (add_view(cal, board, s, 12) != 1) return fail("add (guess)");
  if (at_camcal_solve_host(cal, &res) != AT_OK || res.views_used != 6) return fail("solve_host (guess)");
  if (!(res.rms_after < res.rms_before) || res.cam.k1 != 0.0 || res.cam.k3 != 0.0) return fail("result (guess)");
  at_camcal_destroy(cal);
  at_camcal_destroy(nullptr);

  printf("ok %d %d %d\n", stored, not_stored, refused);
  return 0;
}
