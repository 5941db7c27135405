// at_camcal.cpp -- the camera calibrator's host side: creation and its refusals, the stored views
// (fp_select when one is added), the focal guess, at_camcal_solve_host -- the CPU twin of the
// k_cc_* kernels over the arithmetic of at_camcal.h -- and the records of a finished solve.
// Host only (no HIP): at_camcal_solve and the device buffers are at_api.cpp's.
#include "at_camcal.h"

#include <string.h>

#include <cmath>
#include <memory>
#include <new>

namespace at {

static_assert(kCcMaxViews == AT_CAMCAL_MAX_VIEWS, "at_camcal.h carries the ABI's view cap");
static_assert(sizeof(CcCam) == sizeof(at_camera), "CcCam is at_camera as an array");

// (at_fieldpose.cpp)
int fp_build_layout(const at_field_tag* tags, int n, int16_t* lut, std::vector<FpTag>* out);

namespace {
struct HostDetSrc {
  const at_detection* dets;
  int count;
  int n() const { return count; }
  int32_t id(int c) const { return dets[c].id; }
  int32_t hamming(int c) const { return dets[c].hamming; }
  float margin(int c) const { return dets[c].decision_margin; }
};

// Zhang's constraints with the principal point held at (cx, cy): at_camcal.h's header comment
bool cc_focal_guess(const std::vector<CcObs>& obs, int n, double cx, double cy, double* fx, double* fy) {
  double n00 = 0.0, n01 = 0.0, n11 = 0.0, b0 = 0.0, b1 = 0.0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < obs[i].m; j++) {
      const double* H = obs[i].H[j];
      double x1 = H[0] - cx * H[6], y1 = H[3] - cy * H[6], z1 = H[6];
      double x2 = H[1] - cx * H[7], y2 = H[4] - cy * H[7], z2 = H[7];
      const double q = sqrt(sqrt(x1 * x1 + y1 * y1) * sqrt(x2 * x2 + y2 * y2));
      x1 = x1 / q; y1 = y1 / q; z1 = z1 / q;
      x2 = x2 / q; y2 = y2 / q; z2 = z2 / q;
      const double r[2][3] = {{x1 * x2, y1 * y2, -(z1 * z2)},
                              {x1 * x1 - x2 * x2, y1 * y1 - y2 * y2, -(z1 * z1 - z2 * z2)}};
      for (int k = 0; k < 2; k++) {
        n00 = n00 + r[k][0] * r[k][0];
        n01 = n01 + r[k][0] * r[k][1];
        n11 = n11 + r[k][1] * r[k][1];
        b0 = b0 + r[k][0] * r[k][2];
        b1 = b1 + r[k][1] * r[k][2];
      }
    }
  const double det = n00 * n11 - n01 * n01;
  const double a = (b0 * n11 - b1 * n01) / det, b = (n00 * b1 - n01 * b0) / det;
  if (!(a > 0.0) || !(b > 0.0) || !std::isfinite(a) || !std::isfinite(b)) return false;
  *fx = 1.0 / sqrt(a);
  *fy = 1.0 / sqrt(b);
  return std::isfinite(*fx) && std::isfinite(*fy);
}
}  // namespace

int cc_start_camera(const at_camcal& c, CcCam* out) {
  memcpy(out->v, &c.cfg.init, sizeof(out->v));
  if (!c.cfg.guess) return AT_OK;
  const double cx = (double)c.cfg.width / 2.0, cy = (double)c.cfg.height / 2.0;
  double fx, fy;
  if (!cc_focal_guess(c.obs, c.n, cx, cy, &fx, &fy)) return AT_E_INVALID;
  const CcCam g = {{fx, fy, cx, cy, 0.0, 0.0, 0.0, 0.0, 0.0}};
  *out = g;
  return AT_OK;
}

void cc_finish(at_camcal* c, const CalCtl& ctl, const CcCam& cam, const double* cov, const CalPose* pose,
               const double* viewcost, const int32_t* ntags, at_camcal_result* out) {
  at_camcal_result r;
  memset(&r, 0, sizeof(r));
  memcpy(&r.cam, cam.v, sizeof(r.cam));
  const double corners = (double)ctl.corners;
  r.rms_before = ctl.corners > 0 ? sqrt(ctl.cost0 / corners) : 0.0;
  r.rms_after = ctl.corners > 0 ? sqrt(ctl.cost / corners) : 0.0;
  r.views_used = ctl.used;
  r.views_skipped = c->n - ctl.used;
  r.corners = ctl.corners;
  r.accepted = ctl.accepted;
  r.rejected = ctl.rejected;
  r.cov_valid = ctl.cov_valid;
  for (int k = 0; k < 81; k++) r.cov[k] = ctl.cov_valid ? cov[k] : 0.0;
  c->views.assign((size_t)c->n, at_camcal_view());
  for (int i = 0; i < c->n; i++) {
    at_camcal_view& q = c->views[i];
    memset(&q, 0, sizeof(q));
    if (ntags[i] <= 0) continue;
    memcpy(q.R, pose[i].R, sizeof(q.R));
    memcpy(q.t, pose[i].t, sizeof(q.t));
    q.rms_px = sqrt(viewcost[i] / (double)(4 * ntags[i]));
    q.n_tags = ntags[i];
    q.used = 1;
  }
  c->result = r;
  if (out) *out = r;
}

}  // namespace at

using namespace at;

extern "C" int at_camcal_create(const at_camcal_config* cfg, const at_field_tag* board, int n_tags, int max_hamming,
                                double tag_size, at_camcal** out) {
  if (!out || !cfg || max_hamming < 0 || n_tags < 1) return AT_E_INVALID;
  if (cfg->free_mask < 0 || cfg->free_mask > 511 || cfg->width < 1 || cfg->height < 1) return AT_E_INVALID;
  if (!(tag_size > 0) || !std::isfinite(tag_size)) return AT_E_INVALID;
  if (!cfg->guess) {
    const double* v = &cfg->init.fx;
    for (int k = 0; k < kCcP; k++)
      if (!std::isfinite(v[k])) return AT_E_INVALID;
    if (!(cfg->init.fx > 0) || !(cfg->init.fy > 0)) return AT_E_INVALID;
  }
  std::unique_ptr<at_camcal> c(new (std::nothrow) at_camcal());
  if (!c) return AT_E_NOMEM;
  c->lut.resize(kFpMaxIds);
  const int rc = fp_build_layout(board, n_tags, c->lut.data(), &c->tags);
  if (rc != AT_OK) return rc;
  c->cfg = *cfg;
  c->cfg.guess = cfg->guess != 0;
  c->max_hamming = max_hamming;
  c->tag_size = tag_size;
  memset(&c->result, 0, sizeof(c->result));
  *out = c.release();
  return AT_OK;
}

extern "C" void at_camcal_destroy(at_camcal* c) {
  if (!c) return;
  if (c->gpu && c->gpu_free) c->gpu_free(c->gpu);
  delete c;
}

extern "C" int at_camcal_add(at_camcal* c, const at_detection* dets, int n) {
  if (!c || n < 0 || (n > 0 && !dets)) return AT_E_INVALID;
  if (c->n >= kCcMaxViews) return AT_E_CAPACITY;
  const FpLayout lay = {c->lut.data(), c->tags.data(), c->max_hamming};
  const HostDetSrc src = {dets, n};
  uint32_t cand[kFpSlots], id[kFpSlots];
  int m, dropped;
  fp_select(FpHostWave(), src, lay, cand, id, &m, &dropped);
  if (m < 1) return 0;
  CcObs o;
  memset(&o, 0, sizeof(o));
  o.m = m;
  for (int j = 0; j < m; j++) {
    const at_detection& d = dets[cand[4 * j]];
    o.ids[j] = (int32_t)id[4 * j];
    memcpy(o.p[j], &d.p[0][0], sizeof(o.p[j]));
    memcpy(o.H[j], d.H, sizeof(o.H[j]));
  }
  c->obs.push_back(o);
  c->n++;
  c->obs_dirty = true;
  return 1;
}

extern "C" int at_camcal_count(const at_camcal* c) { return c ? c->n : AT_E_INVALID; }

extern "C" int at_camcal_clear(at_camcal* c) {
  if (!c) return AT_E_INVALID;
  c->obs.clear();
  c->n = 0;
  c->obs_dirty = true;
  return AT_OK;
}

extern "C" int at_camcal_solve_host(at_camcal* c, at_camcal_result* out) {
  if (!c || !out || c->n < 1) return AT_E_INVALID;
  CcCam cam[2];
  const int rc = cc_start_camera(*c, &cam[0]);
  if (rc != AT_OK) return rc;
  cam[1] = cam[0];
  const int N = c->n;
  CcBufs b;
  memset(&b, 0, sizeof(b));
  b.N = N;
  b.tag_size = c->tag_size;
  b.free_mask = c->cfg.free_mask;
  const int nch = b.chunks();
  std::vector<int32_t> ntags((size_t)N);
  std::vector<CalPose> pose[2] = {std::vector<CalPose>((size_t)N), std::vector<CalPose>((size_t)N)};
  std::vector<double> view((size_t)N * kCcViewLen), part((size_t)N * kCcE), chunk((size_t)nch * kCcE), dc(kCcP);
  std::vector<double> viewcost((size_t)N), cov(81);
  CalCtl ctl;
  memset(&ctl, 0, sizeof(ctl));
  b.obs = c->obs.data();
  b.ntags = ntags.data();
  for (int q = 0; q < 2; q++) {
    b.pose[q] = pose[q].data();
    b.cam[q] = &cam[q];
  }
  b.view = view.data();
  b.part = part.data();
  b.chunk = chunk.data();
  b.dc = dc.data();
  b.viewcost = viewcost.data();
  b.cov = cov.data();
  b.ctl = &ctl;
  b.lay = {c->lut.data(), c->tags.data(), c->max_hamming};

  const CalHostTeam tm;
  std::unique_ptr<CcShared> sh(new CcShared());
  std::unique_ptr<CcSolveShared> ssh(new CcSolveShared());
  for (int i = 0; i < N; i++) cc_start(tm, *sh, b, i);
  for (int i = 0; i < N; i++) cc_back(tm, *sh, b, i, false);
  cc_decide(tm, *ssh, b, false);
  for (int it = 0; it <= kCcIters; it++) {
    const bool final = it == kCcIters;
    for (int i = 0; i < N; i++) cc_accum(tm, *sh, b, i, final);
    for (int ch = 0; ch < nch; ch++)
      for (int e = 0; e < kCcE; e++) cc_chunk_entry(b, ch, e);
    cc_reduced(tm, *ssh, b, final);
    if (final) break;
    for (int i = 0; i < N; i++) cc_back(tm, *sh, b, i, true);
    cc_decide(tm, *ssh, b, true);
  }
  for (int i = 0; i < N; i++) cc_back(tm, *sh, b, i, false);
  c->ns = 0;
  cc_finish(c, ctl, cam[ctl.which], cov.data(), pose[ctl.which].data(), viewcost.data(), ntags.data(), out);
  return AT_OK;
}

extern "C" int at_camcal_views(const at_camcal* c, at_camcal_view* out, int cap) {
  if (!c || cap < 0 || (cap > 0 && !out)) return AT_E_INVALID;
  const int n = (int)c->views.size();
  for (int i = 0; i < n && i < cap; i++) out[i] = c->views[i];
  return n;
}

extern "C" int at_camcal_set_profiling(at_camcal* c, int on) {
  if (!c) return AT_E_INVALID;
  c->profiling = on != 0;
  return AT_OK;
}

extern "C" int at_camcal_stats(const at_camcal* c, uint64_t* out, int cap) {
  if (!c || !out || cap < 1) return AT_E_INVALID;
  const uint64_t v[5] = {(uint64_t)c->result.views_used, (uint64_t)c->result.views_skipped,
                         (uint64_t)c->result.accepted, (uint64_t)c->result.rejected, c->ns};
  const int n = cap < 5 ? cap : 5;
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}
