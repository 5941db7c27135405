// rig_calib_host_check.cpp -- the rig calibrator's host side driven stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_rig_calib_host.py builds and runs it): create and its
// refusals, add from heap buffers of exactly the size the call may touch (a camera that sees
// nothing passes NULL arrays), at_rigcal_solve_host, the records, clear and destroy.  Prints
// "ok <instants stored> <instants refused> <calls refused>".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/at_api.h"

static const double kTag = 0.1651;

static void rot(double rx, double ry, double rz, double* R) {  // Rz Ry Rx
  const double cx = cos(rx), sx = sin(rx), cy = cos(ry), sy = sin(ry), cz = cos(rz), sz = sin(rz);
  const double M[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                       sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                       -sy,     cy * sx,                cy * cx};
  memcpy(R, M, sizeof(M));
}
static void mul(const double* a, const double* b, double* c) {
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) c[r * 3 + k] = a[r * 3] * b[k] + a[r * 3 + 1] * b[3 + k] + a[r * 3 + 2] * b[6 + k];
}
static void tr(const double* a, double* c) {
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) c[r * 3 + k] = a[k * 3 + r];
}
static void app(const double* a, const double* x, double* y) {
  for (int r = 0; r < 3; r++) y[r] = a[r * 3] * x[0] + a[r * 3 + 1] * x[1] + a[r * 3 + 2] * x[2];
}

static int fail(const char* what) {
  printf("FAILED: %s\n", what);
  return 1;
}

static const int kTags = 12, kCams = 3;

// 12 tags on and near the wall z = 0; camera i sees the tags k with k % 3 == i or k % 3 == 0.
static void layout(std::vector<at_field_tag>* tags) {
  tags->resize((size_t)kTags);
  for (int k = 0; k < kTags; k++) {
    at_field_tag& g = (*tags)[(size_t)k];
    g.id = 5 * k + 1;
    rot(0, (k % 3 == 2) ? 0.4 : 0.0, 0, g.R);
    g.t[0] = -1.1 + 0.2 * k;
    g.t[1] = -0.15 + 0.3 * (k % 2);
    g.t[2] = (k % 3 == 2) ? -0.15 : 0.0;
  }
}

static void true_mount(int i, at_rig_extrinsics* e) {
  rot(0.01 * i, 0.03 * (i - 1), 0.0, e->R);
  e->t[0] = 0.05 * i - 0.1;
  e->t[1] = 0.02;
  e->t[2] = 0.01 * i;
}

// One instant of the robot at pose number s, exact corners, the tags' own poses turned by 0.04 rad;
// the cameras >= n_seeing see nothing.  Returns at_rigcal_add's value.
static int add_instant(at_rigcal* cal, const std::vector<at_field_tag>& tags, const at_camera* intr, int s,
                       int n_seeing) {
  double Rr[9], RrT[9], dR[9];
  rot(0.03 + 0.01 * s, -0.05 + 0.008 * s, 0.02 - 0.005 * s, Rr);
  tr(Rr, RrT);
  rot(0.04, 0, 0, dR);
  const double tr_[3] = {0.1 - 0.03 * s, -0.05 + 0.02 * s, -3.0 + 0.05 * s};
  at_rigcal_frame* fr = (at_rigcal_frame*)malloc(sizeof(at_rigcal_frame) * (size_t)kCams);
  memset(fr, 0, sizeof(at_rigcal_frame) * (size_t)kCams);
  std::vector<at_detection*> dbuf((size_t)kCams, nullptr);
  std::vector<at_pose*> pbuf((size_t)kCams, nullptr);
  for (int i = 0; i < n_seeing; i++) {
    at_rig_extrinsics e;
    true_mount(i, &e);
    int n = 0;
    for (int k = 0; k < kTags; k++) n += k % 3 == i || k % 3 == 0;
    fr[i].n = n;
    dbuf[(size_t)i] = (at_detection*)malloc(sizeof(at_detection) * (size_t)n);
    pbuf[(size_t)i] = (at_pose*)malloc(sizeof(at_pose) * (size_t)n);
    memset(dbuf[(size_t)i], 0, sizeof(at_detection) * (size_t)n);
    memset(pbuf[(size_t)i], 0, sizeof(at_pose) * (size_t)n);
    fr[i].dets = dbuf[(size_t)i];
    fr[i].poses = pbuf[(size_t)i];
    // x_cam = Rc x_field + tc with Rc = E_R^T Rr^T, tc = -E_R^T (Rr^T tr + E_t)
    double ERT[9], Rc[9], v[3], w[3], tc[3];
    tr(e.R, ERT);
    mul(ERT, RrT, Rc);
    app(RrT, tr_, v);
    for (int r = 0; r < 3; r++) v[r] += e.t[r];
    app(ERT, v, w);
    for (int r = 0; r < 3; r++) tc[r] = -w[r];
    int q = 0;
    for (int k = 0; k < kTags; k++) {
      if (!(k % 3 == i || k % 3 == 0)) continue;
      const at_field_tag& g = tags[(size_t)k];
      at_detection& d = dbuf[(size_t)i][q];
      at_pose& p = pbuf[(size_t)i][q];
      q++;
      d.id = p.id = g.id;
      d.decision_margin = 60.0f;
      double Rtc[9], ttc[3];
      mul(Rc, g.R, Rtc);
      app(Rc, g.t, ttc);
      for (int r = 0; r < 3; r++) ttc[r] += tc[r];
      const double sx[4] = {-1, 1, 1, -1}, sy[4] = {1, 1, -1, -1};
      for (int c = 0; c < 4; c++) {
        const double x = sx[c] * kTag / 2, y = sy[c] * kTag / 2;
        const double P[3] = {Rtc[0] * x + Rtc[1] * y + ttc[0], Rtc[3] * x + Rtc[4] * y + ttc[1],
                             Rtc[6] * x + Rtc[7] * y + ttc[2]};
        d.p[c][0] = intr[i].fx * P[0] / P[2] + intr[i].cx;
        d.p[c][1] = intr[i].fy * P[1] / P[2] + intr[i].cy;
      }
      mul(dR, Rtc, p.R);
      memcpy(p.t, ttc, sizeof(ttc));
    }
  }
  const int rc = at_rigcal_add(cal, fr);
  for (int i = 0; i < kCams; i++) {
    free(dbuf[(size_t)i]);
    free(pbuf[(size_t)i]);
  }
  free(fr);
  return rc;
}

int main() {
  std::vector<at_field_tag> tags;
  layout(&tags);
  at_camera intr[kCams];
  memset(intr, 0, sizeof(intr));
  at_rigcal_camera* cams = (at_rigcal_camera*)malloc(sizeof(at_rigcal_camera) * (size_t)kCams);
  memset(cams, 0, sizeof(at_rigcal_camera) * (size_t)kCams);
  for (int i = 0; i < kCams; i++) {
    intr[i].fx = 900.0 + 10 * i;
    intr[i].fy = 905.0 - 5 * i;
    intr[i].cx = 640.0 + i;
    intr[i].cy = 360.0 - i;
    cams[i].cam = intr[i];
    true_mount(i, &cams[i].extr);
    if (i) {  // the free cameras start 0.03 rad and 2 cm off
      double d[9], m[9];
      rot(0.02, -0.03, 0.01, d);
      mul(cams[i].extr.R, d, m);
      memcpy(cams[i].extr.R, m, sizeof(m));
      cams[i].extr.t[0] += 0.02;
    }
    cams[i].free_rot = i > 0;
    cams[i].free_trans = i == 1;
  }
  // camera 2 is free_rot only: it keeps its true translation
  cams[2].extr.t[0] -= 0.02;

  int refused = 0;
  at_rigcal* cal = nullptr;
  refused += at_rigcal_create(cams, 1, tags.data(), kTags, 0, kTag, &cal) == AT_E_INVALID;
  refused += at_rigcal_create(cams, kCams, tags.data(), 0, 0, kTag, &cal) == AT_E_INVALID;
  refused += at_rigcal_create(cams, kCams, tags.data(), kTags, 0, 0.0, &cal) == AT_E_INVALID;
  cams[0].free_rot = 1;
  refused += at_rigcal_create(cams, kCams, tags.data(), kTags, 0, kTag, &cal) == AT_E_INVALID;
  cams[0].free_rot = 0;
  if (cal) return fail("a refused create wrote a handle");
  if (at_rigcal_create(cams, kCams, tags.data(), kTags, 0, kTag, &cal) != AT_OK) return fail("create");
  at_rigcal_result res;
  refused += at_rigcal_solve_host(cal, &res) == AT_E_INVALID;  // nothing stored

  int kept = 0, dropped = 0;
  for (int s = 0; s < 35; s++) {
    const int rc = add_instant(cal, tags, intr, s, s == 4 ? 1 : s % 7 == 5 ? 2 : 3);
    if (rc < 0) return fail("add");
    kept += rc == 1;
    dropped += rc == 0;
  }
  if (at_rigcal_count(cal) != kept || kept != 34 || dropped != 1) return fail("count");
  if (at_rigcal_solve_host(cal, &res) != AT_OK) return fail("solve_host");
  if (res.instants_used != kept || res.instants_skipped != 0 || res.accepted < 1 || !res.cov_valid) return fail("result");
  if (!(res.rms_after < 1e-9) || !(res.rms_before > 0.1)) return fail("rms");
  for (int i = 0; i < kCams; i++) {
    at_rig_extrinsics e;
    true_mount(i, &e);
    for (int k = 0; k < 9; k++)
      if (fabs(res.cams[i].R[k] - e.R[k]) > 1e-9) return fail("R");
    for (int k = 0; k < 3; k++)
      if (fabs(res.cams[i].t[k] - e.t[k]) > 1e-9) return fail("t");
  }
  at_rigcal_instant* inst = (at_rigcal_instant*)malloc(sizeof(at_rigcal_instant) * (size_t)kept);
  if (at_rigcal_instants(cal, inst, kept) != kept) return fail("instants");
  for (int i = 0; i < kept; i++)
    if (!inst[i].used || inst[i].n_tags < 8 || !(inst[i].rms_px < 1e-9)) return fail("instant record");
  free(inst);
  uint64_t st[5];
  if (at_rigcal_stats(cal, st, 5) != 5 || st[0] != (uint64_t)kept || st[4] != 0) return fail("stats");
  if (at_rigcal_clear(cal) != AT_OK || at_rigcal_count(cal) != 0) return fail("clear");
  refused += at_rigcal_solve_host(cal, &res) == AT_E_INVALID;
  at_rigcal_destroy(cal);
  at_rigcal_destroy(nullptr);
  free(cams);
  printf("ok %d %d %d\n", kept, dropped, refused);
  return 0;
}
