// rig_robust_host_check.cpp -- at_rig_pose_robust_host driven stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_rig_robust_host.py builds and runs it).  Every array is
// a heap buffer of exactly the size the call may touch.  Prints
// "ok <instants solved> <calls refused>".
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

// The robot at (Rr, tr_) 3 m in front of nt tags on a grid of the wall z = 0; camera i of n_cams,
// mounted with a turn about y and an offset of its own, sees the tags k with owner[k] == i, exact
// corners, poses the true ones turned by 0.04 rad about x.  The layout the solver is told has the
// tags with bad[k] moved by 0.3 m along x.  Expects exactly those views dropped (want_starved: none
// dropped, starved set) and, where something was dropped, the true robot pose to 1e-6.
static int instant(int n_cams, int nt, const int* owner, const bool* bad, int min_keep, bool want_starved,
                   int* solved) {
  double Rr[9], RrT[9];
  rot(0.03, -0.05, 0.02, Rr);
  tr(Rr, RrT);
  const double tr_[3] = {0.1, -0.05, -3.0};
  std::vector<at_field_tag> tags((size_t)nt), told((size_t)nt);
  for (int k = 0; k < nt; k++) {
    at_field_tag& g = tags[(size_t)k];
    g.id = 3 * k + 1;
    rot(0, (k % 3 == 2) ? 0.4 : 0.0, 0, g.R);
    g.t[0] = -1.2 + 0.3 * (k % 9);
    g.t[1] = -1.0 + 0.25 * (k / 9);
    g.t[2] = (k % 3 == 2) ? -0.15 : 0.0;
    told[(size_t)k] = g;
    if (bad[k]) told[(size_t)k].t[0] += 0.3;
  }
  at_rig_host_cam* cams = (at_rig_host_cam*)malloc(sizeof(at_rig_host_cam) * (size_t)n_cams);
  at_camera* intr = (at_camera*)malloc(sizeof(at_camera) * (size_t)n_cams);
  std::vector<at_detection*> dbuf((size_t)n_cams, nullptr);
  std::vector<at_pose*> pbuf((size_t)n_cams, nullptr);
  memset(cams, 0, sizeof(at_rig_host_cam) * (size_t)n_cams);
  memset(intr, 0, sizeof(at_camera) * (size_t)n_cams);
  double dR[9];
  rot(0.04, 0, 0, dR);
  int want_tags = 0, want_bad = 0;
  for (int i = 0; i < n_cams; i++) {
    intr[i].fx = 900.0 + 10 * i;
    intr[i].fy = 905.0 - 5 * i;
    intr[i].cx = 640.0 + i;
    intr[i].cy = 360.0 - i;
    at_rig_host_cam& c = cams[i];
    c.cam = &intr[i];
    rot(0.01 * i, 0.03 * (i - n_cams / 2), 0.0, c.extr.R);
    c.extr.t[0] = 0.05 * i - 0.1;
    c.extr.t[1] = 0.02;
    c.extr.t[2] = 0.01 * i;
    int n = 0;
    for (int k = 0; k < nt; k++) n += owner[k] == i;
    c.n = n;
    want_tags += n;
    if (!n) continue;
    dbuf[(size_t)i] = (at_detection*)malloc(sizeof(at_detection) * (size_t)n);
    pbuf[(size_t)i] = (at_pose*)malloc(sizeof(at_pose) * (size_t)n);
    memset(dbuf[(size_t)i], 0, sizeof(at_detection) * (size_t)n);
    memset(pbuf[(size_t)i], 0, sizeof(at_pose) * (size_t)n);
    c.dets = dbuf[(size_t)i];
    c.poses = pbuf[(size_t)i];
    double ERT[9], Rc[9], v[3], w[3], tc[3];
    tr(c.extr.R, ERT);
    mul(ERT, RrT, Rc);
    app(RrT, tr_, v);
    for (int r = 0; r < 3; r++) v[r] += c.extr.t[r];
    app(ERT, v, w);
    for (int r = 0; r < 3; r++) tc[r] = -w[r];
    int q = 0;
    for (int k = 0; k < nt; k++) {
      if (owner[k] != i) continue;
      want_bad += bad[k];
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
      for (int e = 0; e < 4; e++) {
        const double x = sx[e] * kTag / 2, y = sy[e] * kTag / 2;
        const double P[3] = {Rtc[0] * x + Rtc[1] * y + ttc[0], Rtc[3] * x + Rtc[4] * y + ttc[1],
                             Rtc[6] * x + Rtc[7] * y + ttc[2]};
        d.p[e][0] = intr[i].fx * P[0] / P[2] + intr[i].cx;
        d.p[e][1] = intr[i].fy * P[1] / P[2] + intr[i].cy;
      }
      mul(dR, Rtc, p.R);
      memcpy(p.t, ttc, sizeof(ttc));
    }
  }
  at_rig_pose* out = (at_rig_pose*)malloc(sizeof(at_rig_pose));
  at_rig_robust_info* info = (at_rig_robust_info*)malloc(sizeof(at_rig_robust_info));
  at_rig_robust_config* cfg = (at_rig_robust_config*)malloc(sizeof(at_rig_robust_config));
  memset(out, 0xff, sizeof(*out));
  memset(info, 0xff, sizeof(*info));
  cfg->huber_px = 2.0;
  cfg->reject_px = 6.0;
  cfg->max_rounds = 3;
  cfg->min_keep = min_keep;
  int bad_ = 0;
  if (at_rig_pose_robust_host(cams, n_cams, told.data(), nt, 0, kTag, cfg, out, info) != AT_OK)
    bad_ = fail("at_rig_pose_robust_host");
  if (!bad_ && out->n_tags != want_tags) bad_ = fail("n_tags");
  if (!bad_ && info->pad != 0) bad_ = fail("pad");
  if (!bad_ && want_starved) {
    if (!info->starved || info->n_rejected != 0 || info->n_kept != want_tags) bad_ = fail("starved");
  } else if (!bad_) {
    if (info->starved || info->n_rejected != want_bad || info->n_kept != want_tags - want_bad) bad_ = fail("counts");
    for (int i = 0; !bad_ && i < AT_RIG_MAX_CAMS; i++) {
      uint32_t want = 0;
      int q = 0;
      for (int k = 0; i < n_cams && k < nt; k++)
        if (owner[k] == i) want |= (uint32_t)(bad[k] ? 1u : 0u) << q++;
      if (info->rejected_mask[i] != want) bad_ = fail("rejected_mask");
      for (int j = 0; !bad_ && j < AT_FIELD_MAX_TAGS; j++) {
        const double v = info->tag_rms_px[i][j];
        const bool used = i < n_cams && j < cams[i].n;
        if (!used && v != 0.0) bad_ = fail("tag_rms_px beyond tags_per_cam");
        if (used && ((want >> j) & 1u) != (uint32_t)(v > 6.0)) bad_ = fail("tag_rms_px");
      }
    }
    for (int k = 0; !bad_ && k < 9; k++)
      if (!(fabs(out->R[k] - Rr[k]) <= 1e-6)) bad_ = fail("R");
    for (int k = 0; !bad_ && k < 3; k++)
      if (!(fabs(out->t[k] - tr_[k]) <= 1e-6)) bad_ = fail("t");
    if (!bad_ && !out->cov_valid) bad_ = fail("cov_valid");
  }
  free(cfg);
  free(info);
  free(out);
  for (int i = 0; i < n_cams; i++) {
    free(dbuf[(size_t)i]);
    free(pbuf[(size_t)i]);
  }
  free(intr);
  free(cams);
  if (!bad_) ++*solved;
  return bad_;
}

static int refusals(int* refused) {
  at_field_tag* tags = (at_field_tag*)malloc(sizeof(at_field_tag));
  at_rig_host_cam* cam = (at_rig_host_cam*)malloc(sizeof(at_rig_host_cam));
  at_camera intr = {900, 900, 640, 360, 0, 0, 0, 0, 0};
  at_rig_pose out;
  at_rig_robust_info info;
  at_rig_robust_config cfg = {2.0, 6.0, 3, 2};
  memset(tags, 0, sizeof(*tags));
  memset(cam, 0, sizeof(*cam));
  tags->R[0] = tags->R[4] = tags->R[8] = 1;
  cam->extr.R[0] = cam->extr.R[4] = cam->extr.R[8] = 1;
  cam->cam = &intr;
  int bad = 0;
  if (at_rig_pose_robust_host(cam, 1, tags, 1, 0, kTag, &cfg, &out, &info) != AT_OK || out.n_tags != 0 ||
      info.n_kept != 0)
    bad = fail("a valid call");
  *refused += at_rig_pose_robust_host(cam, 1, tags, 1, 0, kTag, nullptr, &out, &info) == AT_E_INVALID;
  *refused += at_rig_pose_robust_host(cam, 1, tags, 1, 0, kTag, &cfg, &out, nullptr) == AT_E_INVALID;
  *refused += at_rig_pose_robust_host(cam, 1, tags, 1, 0, kTag, &cfg, nullptr, &info) == AT_E_INVALID;
  at_rig_robust_config c = cfg;
  c.huber_px = 0.0;
  *refused += at_rig_pose_robust_host(cam, 1, tags, 1, 0, kTag, &c, &out, &info) == AT_E_INVALID;
  c = cfg;
  c.reject_px = NAN;
  *refused += at_rig_pose_robust_host(cam, 1, tags, 1, 0, kTag, &c, &out, &info) == AT_E_INVALID;
  c = cfg;
  c.max_rounds = 4;
  *refused += at_rig_pose_robust_host(cam, 1, tags, 1, 0, kTag, &c, &out, &info) == AT_E_INVALID;
  c = cfg;
  c.min_keep = 0;
  *refused += at_rig_pose_robust_host(cam, 1, tags, 1, 0, kTag, &c, &out, &info) == AT_E_INVALID;
  *refused += at_rig_pose_robust_host(cam, 9, tags, 1, 0, kTag, &cfg, &out, &info) == AT_E_INVALID;
  cam->cam = nullptr;
  *refused += at_rig_pose_robust_host(cam, 1, tags, 1, 0, kTag, &cfg, &out, &info) == AT_E_INVALID;
  free(cam);
  free(tags);
  return bad;
}

int main() {
  int solved = 0, refused = 0;
  {  // three cameras, the middle one sees nothing (n = 0, NULL arrays); one bad tag in camera 2
    const int owner[8] = {0, 0, 0, 0, 2, 2, 2, 2};
    const bool bad[8] = {false, false, false, false, false, true, false, false};
    if (instant(3, 8, owner, bad, 2, false, &solved)) return 1;
  }
  {  // camera 1's only tag is bad: the rejection leaves it without a kept slot
    const int owner[7] = {0, 0, 0, 1, 2, 2, 2};
    const bool bad[7] = {false, false, false, true, false, false, false};
    if (instant(3, 7, owner, bad, 2, false, &solved)) return 1;
  }
  {  // 8 cameras of 16 tags each, one bad tag in every second camera
    int owner[128];
    bool bad[128];
    for (int k = 0; k < 128; k++) {
      owner[k] = k / 16;
      bad[k] = (k / 16) % 2 == 1 && k % 16 == (k / 16);
    }
    if (instant(8, 128, owner, bad, 2, false, &solved)) return 1;
  }
  {  // one camera, two tags, one bad, min_keep 2: starved
    const int owner[2] = {0, 0};
    const bool bad[2] = {false, true};
    if (instant(1, 2, owner, bad, 2, true, &solved)) return 1;
  }
  if (refusals(&refused)) return 1;
  printf("ok %d %d\n", solved, refused);
  return refused == 9 ? 0 : 1;
}
