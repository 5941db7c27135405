// field_map_host_check.cpp -- the field mapper's host side driven stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_field_map_host.py builds and runs it): create and its
// refusals, add from heap buffers of exactly the size the call may touch (a view of 17 tags, a
// view of one, an empty view from NULL arrays), the placing of a tag without a start,
// at_fieldmap_solve_host, the records, clear and destroy.  Prints
// "ok <views stored> <views refused> <calls refused> <tags placed>".
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
static void app(const double* a, const double* x, double* y) {
  for (int r = 0; r < 3; r++) y[r] = a[r * 3] * x[0] + a[r * 3 + 1] * x[1] + a[r * 3 + 2] * x[2];
}

static int fail(const char* what) {
  printf("FAILED: %s\n", what);
  return 1;
}

static const int kTags = 20;

// 20 tags in 5 columns on and near the wall z = 0; the last one is seen by no view
static void truth(std::vector<at_field_tag>* tags) {
  tags->resize((size_t)kTags);
  for (int k = 0; k < kTags; k++) {
    at_field_tag& g = (*tags)[(size_t)k];
    g.id = 7 * k + 2;
    rot(0, (k % 3 == 2) ? 0.4 : 0.0, 0, g.R);
    g.t[0] = -0.9 + 0.45 * (k % 5);
    g.t[1] = -0.5 + 0.33 * (k / 5);
    g.t[2] = (k % 3 == 2) ? -0.15 : 0.0;
  }
}

// View number s of the tags first .. first + n - 1, exact corners, the tags' own poses turned by
// 0.04 rad.  Returns at_fieldmap_add's value.
static int add_view(at_fieldmap* m, const std::vector<at_field_tag>& tags, const at_camera* cam, int s, int first, int n) {
  double Rc[9], dR[9];
  rot(0.03 + 0.01 * s, -0.05 + 0.008 * s, 0.02 - 0.005 * s, Rc);
  rot(0.04, 0, 0, dR);
  const double tc[3] = {0.1 - 0.03 * s, -0.05 + 0.02 * s, 3.0 + 0.05 * s};
  at_detection* d = n ? (at_detection*)malloc(sizeof(at_detection) * (size_t)n) : nullptr;
  at_pose* p = n ? (at_pose*)malloc(sizeof(at_pose) * (size_t)n) : nullptr;
  if (n) {
    memset(d, 0, sizeof(at_detection) * (size_t)n);
    memset(p, 0, sizeof(at_pose) * (size_t)n);
  }
  for (int q = 0; q < n; q++) {
    const at_field_tag& g = tags[(size_t)(first + q)];
    d[q].id = p[q].id = g.id;
    d[q].decision_margin = 60.0f;
    double Rtc[9], ttc[3];
    mul(Rc, g.R, Rtc);
    app(Rc, g.t, ttc);
    for (int r = 0; r < 3; r++) ttc[r] += tc[r];
    const double sx[4] = {-1, 1, 1, -1}, sy[4] = {1, 1, -1, -1};
    for (int c = 0; c < 4; c++) {
      const double x = sx[c] * kTag / 2, y = sy[c] * kTag / 2;
      const double P[3] = {Rtc[0] * x + Rtc[1] * y + ttc[0], Rtc[3] * x + Rtc[4] * y + ttc[1],
                           Rtc[6] * x + Rtc[7] * y + ttc[2]};
      d[q].p[c][0] = cam->fx * P[0] / P[2] + cam->cx;
      d[q].p[c][1] = cam->fy * P[1] / P[2] + cam->cy;
    }
    mul(dR, Rtc, p[q].R);
    memcpy(p[q].t, ttc, sizeof(ttc));
  }
  const int rc = at_fieldmap_add(m, d, p, n, cam);
  free(d);
  free(p);
  return rc;
}

int main() {
  std::vector<at_field_tag> tags;
  truth(&tags);
  at_camera cam;
  memset(&cam, 0, sizeof(cam));
  cam.fx = 900.0;
  cam.fy = 905.0;
  cam.cx = 640.0;
  cam.cy = 360.0;
  // tag 0 is the anchor, tags 3 and 19 have no start (19 is in no view: it stays unplaced), tag 5
  // is free_rot only; the others start 0.03 rad and 2 cm off
  at_fieldmap_tag* mt = (at_fieldmap_tag*)malloc(sizeof(at_fieldmap_tag) * (size_t)kTags);
  memset(mt, 0, sizeof(at_fieldmap_tag) * (size_t)kTags);
  for (int k = 0; k < kTags; k++) {
    mt[k].tag = tags[(size_t)k];
    mt[k].known = k != 3 && k != kTags - 1;
    mt[k].free_rot = k > 0;
    mt[k].free_trans = k > 0 && k != 5;
    if (!mt[k].known) {
      memset(mt[k].tag.R, 0, sizeof(mt[k].tag.R));  // (not read)
      continue;
    }
    if (k > 0) {
      double d[9], r[9];
      rot(0.02, -0.03, 0.01, d);
      mul(tags[(size_t)k].R, d, r);
      memcpy(mt[k].tag.R, r, sizeof(r));
      if (k != 5) mt[k].tag.t[0] += 0.02;
    }
  }

  int refused = 0;
  at_fieldmap* m = nullptr;
  refused += at_fieldmap_create(mt, 0, 0, kTag, &m) == AT_E_INVALID;
  refused += at_fieldmap_create(mt, 33, 0, kTag, &m) == AT_E_INVALID;
  refused += at_fieldmap_create(mt, kTags, -1, kTag, &m) == AT_E_INVALID;
  refused += at_fieldmap_create(mt, kTags, 0, 0.0, &m) == AT_E_INVALID;
  mt[0].free_rot = 1;
  refused += at_fieldmap_create(mt, kTags, 0, kTag, &m) == AT_E_INVALID;  // no anchor
  mt[0].free_rot = 0;
  if (m) return fail("a refused create wrote a handle");
  if (at_fieldmap_create(mt, kTags, 0, kTag, &m) != AT_OK) return fail("create");
  at_fieldmap_result res;
  refused += at_fieldmap_solve_host(m, &res) == AT_E_INVALID;  // nothing stored

  int kept = 0, dropped = 0;
  for (int s = 0; s < 35; s++) {
    // windows of 6 tags over tags 0 .. 18; view 4 holds one tag, view 9 none, view 20 holds 17
    const int n = s == 4 ? 1 : s == 9 ? 0 : s == 20 ? 17 : 6;
    const int rc = add_view(m, tags, &cam, s, n == 17 ? 0 : s % 14, n);
    if (rc < 0) return fail("add");
    kept += rc == 1;
    dropped += rc == 0;
  }
  if (at_fieldmap_count(m) != kept || kept != 33 || dropped != 2) return fail("count");
  if (at_fieldmap_solve_host(m, &res) != AT_OK) return fail("solve_host");
  if (res.views_used != kept || res.views_skipped != 0 || res.accepted < 1 || !res.cov_valid) return fail("result");
  if (res.n_tags != kTags || res.n_placed != kTags - 1) return fail("placed");
  if (!(res.rms_after < 1e-9) || !(res.rms_before > 0.1)) return fail("rms");
  at_fieldmap_tag_result* tr = (at_fieldmap_tag_result*)malloc(sizeof(at_fieldmap_tag_result) * (size_t)kTags);
  if (at_fieldmap_tags(m, tr, kTags) != kTags) return fail("tags");
  for (int k = 0; k < kTags; k++) {
    if (tr[k].id != tags[(size_t)k].id) return fail("tag id");
    if (k == kTags - 1) {
      if (tr[k].placed || tr[k].views || tr[k].R[0] != 0.0) return fail("unplaced tag");
      continue;
    }
    if (!tr[k].placed || tr[k].views < 1) return fail("tag record");
    for (int q = 0; q < 9; q++)
      if (fabs(tr[k].R[q] - tags[(size_t)k].R[q]) > 1e-9) return fail("R");
    for (int q = 0; q < 3; q++)
      if (fabs(tr[k].t[q] - tags[(size_t)k].t[q]) > 1e-9) return fail("t");
  }
  if (memcmp(tr[5].t, mt[5].tag.t, sizeof(tr[5].t)) != 0) return fail("a fixed translation moved");
  free(tr);
  at_fieldmap_view* vw = (at_fieldmap_view*)malloc(sizeof(at_fieldmap_view) * (size_t)kept);
  if (at_fieldmap_views(m, vw, kept) != kept) return fail("views");
  for (int i = 0; i < kept; i++)
    if (!vw[i].used || vw[i].n_tags < 6 || !(vw[i].rms_px < 1e-9)) return fail("view record");
  free(vw);
  uint64_t st[6];
  if (at_fieldmap_stats(m, st, 6) != 6 || st[0] != (uint64_t)kept || st[4] != 0 || st[5] != 1) return fail("stats");
  if (at_fieldmap_clear(m) != AT_OK || at_fieldmap_count(m) != 0) return fail("clear");
  refused += at_fieldmap_solve_host(m, &res) == AT_E_INVALID;
  at_fieldmap_destroy(m);
  at_fieldmap_destroy(nullptr);
  free(mt);
  printf("ok %d %d %d %d\n", kept, dropped, refused, kTags - 1);
  return 0;
}
