// field_pose_host_check.cpp -- at_field_pose_host / at_robot_in_field driven stand-alone, for a
// build with -fsanitize=address,undefined (tests/test_field_pose_host.py builds and runs it).
// Every array is a heap buffer of exactly the size the call may touch.  Prints
// "ok <scenes solved> <layouts refused>".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/at_api.h"

static const double kTag = 0.1651;
static const at_camera kCam = {905.495617, 907.909470, 609.916016, 352.682645, 0, 0, 0, 0, 0};

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

// n tags on the wall z = 0 (every third turned a little about y), ids 3 k + 2 shuffled, seen from
// (R, t); the poses are the true ones turned by 0.04 rad about x.  `extra` more candidates follow:
// copies with a worse hamming and spoiled corners, and ids of no layout.
static int scene(int n, int extra, int* solved) {
  double R[9], t[3];
  rot(0.1, -0.15, 0.05, R);
  const double C[3] = {0.2, -0.1, -3.0};
  for (int r = 0; r < 3; r++) t[r] = -(R[r * 3] * C[0] + R[r * 3 + 1] * C[1] + R[r * 3 + 2] * C[2]);
  std::vector<at_field_tag> tags((size_t)n);
  for (int k = 0; k < n; k++) {
    at_field_tag& g = tags[(size_t)k];
    g.id = 3 * ((k * 7) % n) + 2;
    rot(0, (k % 3 == 2) ? 0.5 : 0.0, 0, g.R);
    g.t[0] = -1.0 + 0.25 * (k % 9);
    g.t[1] = -0.2 + 0.4 * (k / 9);
    g.t[2] = (k % 3 == 2) ? -0.2 : 0.0;
  }
  const int nd = n + extra;
  at_detection* dets = (at_detection*)malloc(sizeof(at_detection) * (size_t)nd);
  at_pose* poses = (at_pose*)malloc(sizeof(at_pose) * (size_t)nd);
  if (!dets || !poses) return fail("malloc");
  memset(dets, 0, sizeof(at_detection) * (size_t)nd);
  memset(poses, 0, sizeof(at_pose) * (size_t)nd);
  double dR[9];
  rot(0.04, 0, 0, dR);
  for (int k = 0; k < nd; k++) {
    const at_field_tag& g = tags[(size_t)(k % n)];
    at_detection& d = dets[k];
    at_pose& p = poses[k];
    const bool copy = k >= n;
    d.id = p.id = copy && (k & 1) ? 1000 + k % 20 : g.id;   // (1000..1019: in no layout)
    d.hamming = copy ? 1 : 0;
    d.decision_margin = 50.0f + (float)k;
    const double sx[4] = {-1, 1, 1, -1}, sy[4] = {1, 1, -1, -1};
    double Rtc[9], ttc[3];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) Rtc[r * 3 + c] = R[r * 3] * g.R[c] + R[r * 3 + 1] * g.R[3 + c] + R[r * 3 + 2] * g.R[6 + c];
      ttc[r] = R[r * 3] * g.t[0] + R[r * 3 + 1] * g.t[1] + R[r * 3 + 2] * g.t[2] + t[r];
    }
    for (int i = 0; i < 4; i++) {
      const double x = sx[i] * kTag / 2, y = sy[i] * kTag / 2;
      const double P[3] = {Rtc[0] * x + Rtc[1] * y + ttc[0], Rtc[3] * x + Rtc[4] * y + ttc[1],
                           Rtc[6] * x + Rtc[7] * y + ttc[2]};
      d.p[i][0] = kCam.fx * P[0] / P[2] + kCam.cx + (copy ? 30.0 : 0.0);
      d.p[i][1] = kCam.fy * P[1] / P[2] + kCam.cy;
    }
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) p.R[r * 3 + c] = dR[r * 3] * Rtc[c] + dR[r * 3 + 1] * Rtc[3 + c] + dR[r * 3 + 2] * Rtc[6 + c];
    memcpy(p.t, ttc, sizeof(ttc));
  }
  at_field_pose* out = (at_field_pose*)malloc(sizeof(at_field_pose));
  int rc = at_field_pose_host(dets, poses, nd, tags.data(), n, 2, &kCam, kTag, out);
  int bad = 0;
  if (rc != AT_OK) bad = fail("at_field_pose_host");
  const int want = n < AT_FIELD_MAX_TAGS ? n : AT_FIELD_MAX_TAGS;
  if (!bad && out->n_tags != want) bad = fail("n_tags");
  for (int j = 0; !bad && j < want; j++)
    if (out->ids[j] != 3 * j + 2) bad = fail("ids");
  for (int k = 0; !bad && k < 9; k++)
    if (!(fabs(out->R[k] - R[k]) <= 1e-9)) bad = fail("R");
  for (int k = 0; !bad && k < 3; k++)
    if (!(fabs(out->t[k] - t[k]) <= 1e-9)) bad = fail("t");
  if (!bad && !(out->rms_px < 1e-9)) bad = fail("rms_px");
  if (!bad) {
    double* Rr = (double*)malloc(9 * sizeof(double));
    double* tr = (double*)malloc(3 * sizeof(double));
    if (at_robot_in_field(out, nullptr, nullptr, Rr, tr) != AT_OK) bad = fail("at_robot_in_field");
    for (int k = 0; !bad && k < 3; k++)
      if (!(fabs(tr[k] - C[k]) <= 1e-9)) bad = fail("camera centre");
    free(Rr);
    free(tr);
  }
  free(out);
  free(dets);
  free(poses);
  if (!bad) ++*solved;
  return bad;
}

static int refusals(int* refused) {
  at_field_tag* tags = (at_field_tag*)malloc(2 * sizeof(at_field_tag));
  at_field_pose out;
  memset(tags, 0, 2 * sizeof(at_field_tag));
  for (int k = 0; k < 2; k++) {
    tags[k].id = k;
    tags[k].R[0] = tags[k].R[4] = tags[k].R[8] = 1;
  }
  auto call = [&](int n, int mh, double size) {
    return at_field_pose_host(nullptr, nullptr, 0, tags, n, mh, &kCam, size, &out);
  };
  int bad = 0;
  if (call(2, 0, kTag) != AT_OK || out.n_tags != 0) bad = fail("a valid layout, no candidates");
  if (call(0, 0, kTag) != AT_OK) bad = fail("an empty layout");
  *refused += call(2, 0, 0.0) == AT_E_INVALID;
  *refused += call(2, -1, kTag) == AT_E_INVALID;
  tags[1].id = 0;
  *refused += call(2, 0, kTag) == AT_E_INVALID;
  tags[1].id = 1024;
  *refused += call(2, 0, kTag) == AT_E_INVALID;
  tags[1].id = -1;
  *refused += call(2, 0, kTag) == AT_E_INVALID;
  tags[1].id = 1;
  tags[1].R[1] = 3e-6;
  *refused += call(2, 0, kTag) == AT_E_INVALID;
  tags[1].R[1] = 0;
  tags[1].R[8] = -1;
  *refused += call(2, 0, kTag) == AT_E_INVALID;
  tags[1].R[8] = 1;
  *refused += at_field_pose_host(nullptr, nullptr, 0, tags, 2, 0, &kCam, kTag, nullptr) == AT_E_INVALID;
  if (call(2, 0, kTag) != AT_OK) bad = fail("the layout restored");
  free(tags);
  return bad;
}

int main() {
  int solved = 0, refused = 0;
  if (scene(1, 0, &solved) || scene(3, 0, &solved) || scene(17, 0, &solved) || scene(5, 195, &solved)) return 1;
  if (refusals(&refused)) return 1;
  printf("ok %d %d\n", solved, refused);
  return refused == 8 ? 0 : 1;
}
