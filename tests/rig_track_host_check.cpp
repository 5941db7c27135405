// rig_track_host_check.cpp -- the rig tracker's host side driven stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_rig_track_host.py builds and runs it): create and its
// refusals, pushes from heap buffers of exactly the size the call may touch (a camera that sees
// nothing passes NULL arrays; two instants see nothing at all), a slide past the window,
// at_rigtrack_solve_host on exact corners and exact odometry, the records, a chain restart, a
// window without a tag, clear and destroy.  Prints "ok <window count> <instants with tags> <calls refused>".
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

static const int kTags = 12, kCams = 2, kWindow = 6;

// 12 tags on and near the wall z = 0; camera i sees the tags k with k % 3 == i or k % 3 == 2.
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

static void mount(int i, at_rig_extrinsics* e) {
  rot(0.01 * i, 0.03 * (i - 1), 0.0, e->R);
  e->t[0] = 0.05 * i - 0.1;
  e->t[1] = 0.02;
  e->t[2] = 0.01 * i;
}

static void robot(int s, double* R, double* t) {
  rot(0.03 + 0.01 * s, -0.05 + 0.008 * s, 0.02 - 0.005 * s, R);
  t[0] = 0.1 - 0.03 * s;
  t[1] = -0.05 + 0.02 * s;
  t[2] = -3.0 + 0.05 * s;
}

// One instant of the robot at pose number s, exact corners, the tags' own poses turned by 0.04 rad;
// the cameras >= n_seeing see nothing; the exact odometry from pose s - 1 when with_odom.
static int push_instant(at_rigtrack* trk, const std::vector<at_field_tag>& tags, const at_camera* intr, int s,
                        int n_seeing, bool with_odom) {
  double Rr[9], RrT[9], dR[9], tr_[3];
  robot(s, Rr, tr_);
  tr(Rr, RrT);
  rot(0.04, 0, 0, dR);
  at_rigcal_frame* fr = (at_rigcal_frame*)malloc(sizeof(at_rigcal_frame) * (size_t)kCams);
  memset(fr, 0, sizeof(at_rigcal_frame) * (size_t)kCams);
  std::vector<at_detection*> dbuf((size_t)kCams, nullptr);
  std::vector<at_pose*> pbuf((size_t)kCams, nullptr);
  for (int i = 0; i < n_seeing; i++) {
    at_rig_extrinsics e;
    mount(i, &e);
    int n = 0;
    for (int k = 0; k < kTags; k++) n += k % 3 == i || k % 3 == 2;
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
      if (!(k % 3 == i || k % 3 == 2)) continue;
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
  at_rigtrack_odom* od = nullptr;
  if (with_odom) {  // x_prev = R x_now + t: R = Rp^T Rr, t = Rp^T (tr - tp)
    od = (at_rigtrack_odom*)malloc(sizeof(at_rigtrack_odom));
    double Rp[9], tp[3], RpT[9], d[3];
    robot(s - 1, Rp, tp);
    tr(Rp, RpT);
    mul(RpT, Rr, od->R);
    for (int r = 0; r < 3; r++) d[r] = tr_[r] - tp[r];
    app(RpT, d, od->t);
    od->sigma_rot = 0.004;
    od->sigma_trans = 0.003;
  }
  const int rc = at_rigtrack_push(trk, 10.0 + s, fr, od);
  for (int i = 0; i < kCams; i++) {
    free(dbuf[(size_t)i]);
    free(pbuf[(size_t)i]);
  }
  free(od);
  free(fr);
  return rc;
}

int main() {
  std::vector<at_field_tag> tags;
  layout(&tags);
  at_camera intr[kCams];
  memset(intr, 0, sizeof(intr));
  at_rigtrack_camera* cams = (at_rigtrack_camera*)malloc(sizeof(at_rigtrack_camera) * (size_t)kCams);
  memset(cams, 0, sizeof(at_rigtrack_camera) * (size_t)kCams);
  for (int i = 0; i < kCams; i++) {
    intr[i].fx = 900.0 + 10 * i;
    intr[i].fy = 905.0 - 5 * i;
    intr[i].cx = 640.0 + i;
    intr[i].cy = 360.0 - i;
    cams[i].cam = intr[i];
    mount(i, &cams[i].extr);
  }

  int refused = 0;
  at_rigtrack* trk = nullptr;
  refused += at_rigtrack_create(cams, 0, tags.data(), kTags, 0, kTag, 0.5, kWindow, 6, &trk) == AT_E_INVALID;
  refused += at_rigtrack_create(cams, kCams, tags.data(), 0, 0, kTag, 0.5, kWindow, 6, &trk) == AT_E_INVALID;
  refused += at_rigtrack_create(cams, kCams, tags.data(), kTags, 0, kTag, 0.0, kWindow, 6, &trk) == AT_E_INVALID;
  refused += at_rigtrack_create(cams, kCams, tags.data(), kTags, 0, kTag, 0.5, 1, 6, &trk) == AT_E_INVALID;
  refused += at_rigtrack_create(cams, kCams, tags.data(), kTags, 0, kTag, 0.5, 65, 6, &trk) == AT_E_INVALID;
  refused += at_rigtrack_create(cams, kCams, tags.data(), kTags, 0, kTag, 0.5, kWindow, 17, &trk) == AT_E_INVALID;
  if (trk) return fail("a refused create wrote a handle");
  if (at_rigtrack_create(cams, kCams, tags.data(), kTags, 0, kTag, 0.5, kWindow, 6, &trk) != AT_OK) return fail("create");
  at_rigtrack_result res;
  refused += at_rigtrack_solve_host(trk, &res) == AT_E_INVALID;  // nothing stored

  // nine instants through a window of six: 3..8 stay; 5 and 8 (the latest) see nothing, 6 one camera
  for (int s = 0; s < 9; s++) {
    const int rc = push_instant(trk, tags, intr, s, (s == 5 || s == 8) ? 0 : s == 6 ? 1 : 2, s > 0);
    if (rc != (s + 1 < kWindow ? s + 1 : kWindow)) return fail("push");
  }
  if (at_rigtrack_count(trk) != kWindow) return fail("count");
  if (at_rigtrack_solve_host(trk, &res) != AT_OK) return fail("solve_host");
  if (res.n != kWindow || res.with_tags != 4 || !res.cov_valid || res.stamp != 18.0) return fail("result");
  // (an instant with tags starts from its converged rig pose: only the instants without tags start off)
  if (!(res.rms_after < 1e-9) || !(res.cost_after < 1e-12) || !(res.cost_after <= res.cost_before)) {
    printf("rms %g -> %g, cost %g -> %g\n", res.rms_before, res.rms_after, res.cost_before, res.cost_after);
    return fail("rms");
  }
  at_rigtrack_instant* inst = (at_rigtrack_instant*)malloc(sizeof(at_rigtrack_instant) * (size_t)kWindow);
  if (at_rigtrack_instants(trk, inst, kWindow) != kWindow) return fail("instants");
  int with_tags = 0;
  for (int k = 0; k < kWindow; k++) {
    double R[9], t[3];
    robot(3 + k, R, t);
    for (int q = 0; q < 9; q++)
      if (fabs(inst[k].R[q] - R[q]) > 1e-9) return fail("R");
    for (int q = 0; q < 3; q++)
      if (fabs(inst[k].t[q] - t[q]) > 1e-9) return fail("t");
    if (inst[k].stamp != 13.0 + k || (inst[k].n_tags == 0) != (k == 2 || k == 5)) return fail("instant record");
    with_tags += inst[k].n_tags > 0;
  }
  free(inst);
  uint64_t st[8];
  if (at_rigtrack_stats(trk, st, 8) != 8 || st[0] != (uint64_t)kWindow || st[4] != 0) return fail("stats");

  // refused pushes change nothing
  at_rigcal_frame bad[kCams];
  memset(bad, 0, sizeof(bad));
  bad[0].n = -1;
  refused += at_rigtrack_push(trk, 0.0, bad, nullptr) == AT_E_INVALID;
  bad[0].n = 2;  // arrays missing
  refused += at_rigtrack_push(trk, 0.0, bad, nullptr) == AT_E_INVALID;
  bad[0].n = 0;
  at_rigtrack_odom od;
  memset(&od, 0, sizeof(od));
  od.R[0] = od.R[4] = od.R[8] = 1.0;
  od.sigma_rot = 0.0;
  od.sigma_trans = 0.01;
  refused += at_rigtrack_push(trk, 0.0, bad, &od) == AT_E_INVALID;
  od.sigma_rot = 0.01;
  od.R[8] = -1.0;
  refused += at_rigtrack_push(trk, 0.0, bad, &od) == AT_E_INVALID;
  if (at_rigtrack_count(trk) != kWindow) return fail("a refused push changed the window");

  // odometry lost: a new chain of one tagless instant, which cannot be solved; then one with tags
  if (push_instant(trk, tags, intr, 9, 0, false) != 1) return fail("restart");
  refused += at_rigtrack_solve_host(trk, &res) == AT_E_INVALID;
  if (push_instant(trk, tags, intr, 10, 2, true) != 2) return fail("push after restart");
  if (at_rigtrack_solve_host(trk, &res) != AT_OK || res.n != 2 || res.with_tags != 1) return fail("solve after restart");
  if (at_rigtrack_clear(trk) != AT_OK || at_rigtrack_count(trk) != 0) return fail("clear");
  refused += at_rigtrack_solve_host(trk, &res) == AT_E_INVALID;
  at_rigtrack_destroy(trk);
  at_rigtrack_destroy(nullptr);
  free(cams);
  printf("ok %d %d %d\n", kWindow, with_tags, refused);
  return 0;
}
