// at_rigtrack.cpp -- the rig tracker's host side: creation and its refusals, the ring of stored
// instants (fp_select per camera when one is pushed), at_rigtrack_solve_host -- the CPU twin of
// the k_trk_* kernels over the arithmetic of at_rigtrack.h -- and the records of a finished solve.
// Host only (no HIP): at_rigtrack_solve and the device buffers are at_api.cpp's.
#include "at_rigtrack.h"

#include <string.h>

#include <cmath>
#include <memory>
#include <new>

namespace at {

static_assert(kTrkMaxWindow == AT_RIGTRACK_MAX_WINDOW, "at_rigtrack.h carries the ABI's window cap");
static_assert(sizeof(TrkOdom) == sizeof(at_rigtrack_odom), "TrkOdom is at_rigtrack_odom");

// (at_fieldpose.cpp, at_rigpose.cpp)
int fp_build_layout(const at_field_tag* tags, int n, int16_t* lut, std::vector<FpTag>* out);
bool rig_extrinsics_ok(const at_rig_extrinsics& e);

namespace {
struct HostCamSrc {
  const at_detection* dets;
  const at_pose* poses;
  int count;
  int n() const { return count; }
  int32_t id(int c) const { return dets[c].id; }
  int32_t hamming(int c) const { return dets[c].hamming; }
  float margin(int c) const { return dets[c].decision_margin; }
  const double* p(int c) const { return &dets[c].p[0][0]; }
  const double* pose_R(int c) const { return poses[c].R; }
  const double* pose_t(int c) const { return poses[c].t; }
};
bool positive(double v) { return v > 0 && std::isfinite(v); }
}  // namespace

void trk_fill_bufs(const at_rigtrack& t, TrkBufs* b) {
  b->tag_size = t.tag_size;
  b->wpx = 1.0 / (t.sigma_px * t.sigma_px);
  b->N = t.n;
  b->W = t.window;
  b->head = t.head;
  b->n_cams = t.n_cams;
  for (int i = 0; i < kRigMaxCams; i++) {
    const bool in = i < t.n_cams;
    b->fx[i] = in ? t.cams[i].cam.fx : 0.0;
    b->fy[i] = in ? t.cams[i].cam.fy : 0.0;
    b->cx[i] = in ? t.cams[i].cam.cx : 0.0;
    b->cy[i] = in ? t.cams[i].cam.cy : 0.0;
    memset(&b->ext[i], 0, sizeof(b->ext[i]));
    if (!in) continue;
    memcpy(b->ext[i].R, t.cams[i].extr.R, sizeof(b->ext[i].R));
    memcpy(b->ext[i].t, t.cams[i].extr.t, sizeof(b->ext[i].t));
  }
}

void trk_finish(at_rigtrack* t, const TrkCtl& ctl, const CalPose* pose, const double* cov, const double* instpx,
                const int32_t* own_nt, at_rigtrack_result* out) {
  at_rigtrack_result r;
  memset(&r, 0, sizeof(r));
  const double corners = (double)ctl.corners;
  r.n = t->n;
  r.with_tags = ctl.used;
  r.accepted = ctl.accepted;
  r.rejected = ctl.rejected;
  r.cost_before = ctl.cost0;
  r.cost_after = ctl.cost;
  r.rms_before = ctl.corners > 0 ? sqrt(ctl.px0 / corners) : 0.0;
  r.rms_after = ctl.corners > 0 ? sqrt(ctl.px / corners) : 0.0;
  const int last = t->n - 1;
  memcpy(r.R, pose[last].R, sizeof(r.R));
  memcpy(r.t, pose[last].t, sizeof(r.t));
  for (int k = 0; k < 36; k++) r.cov[k] = ctl.cov_valid ? cov[k] : 0.0;
  r.cov_valid = ctl.cov_valid;
  r.stamp = t->stamp[(size_t)((t->head + last) % t->window)];
  t->instants.assign((size_t)t->n, at_rigtrack_instant());
  for (int k = 0; k < t->n; k++) {
    at_rigtrack_instant& q = t->instants[k];
    memset(&q, 0, sizeof(q));
    const int s = (t->head + k) % t->window;
    memcpy(q.R, pose[k].R, sizeof(q.R));
    memcpy(q.t, pose[k].t, sizeof(q.t));
    q.stamp = t->stamp[(size_t)s];
    q.n_tags = own_nt[s] > 0 ? own_nt[s] : 0;
    q.rms_px = q.n_tags > 0 ? sqrt(instpx[k] / (double)(4 * q.n_tags)) : 0.0;
  }
  t->result = r;
  if (out) *out = r;
}

}  // namespace at

using namespace at;

extern "C" int at_rigtrack_create(const at_rigtrack_camera* cams, int n_cams, const at_field_tag* tags, int n_tags,
                                  int max_hamming, double tag_size, double sigma_px, int window, int iters,
                                  at_rigtrack** out) {
  if (!out || !cams || n_cams < 1 || n_cams > kRigMaxCams || max_hamming < 0 || n_tags < 1) return AT_E_INVALID;
  if (!positive(tag_size) || !positive(sigma_px)) return AT_E_INVALID;
  if (window < 2 || window > kTrkMaxWindow || iters < 1 || iters > kTrkMaxIters) return AT_E_INVALID;
  for (int i = 0; i < n_cams; i++)
    if (!rig_extrinsics_ok(cams[i].extr)) return AT_E_INVALID;
  std::unique_ptr<at_rigtrack> t(new (std::nothrow) at_rigtrack());
  if (!t) return AT_E_NOMEM;
  t->lut.resize(kFpMaxIds);
  const int rc = fp_build_layout(tags, n_tags, t->lut.data(), &t->tags);
  if (rc != AT_OK) return rc;
  t->n_cams = n_cams;
  t->max_hamming = max_hamming;
  t->tag_size = tag_size;
  t->sigma_px = sigma_px;
  t->window = window;
  t->iters = iters;
  for (int i = 0; i < n_cams; i++) t->cams[i] = cams[i];
  t->obs.resize((size_t)window * n_cams);
  t->odom.resize((size_t)window);
  t->stamp.resize((size_t)window);
  t->own.resize((size_t)window);
  t->own_nt.assign((size_t)window, -1);
  t->dev_stale.assign((size_t)window, 1);
  memset(&t->result, 0, sizeof(t->result));
  *out = t.release();
  return AT_OK;
}

extern "C" void at_rigtrack_destroy(at_rigtrack* t) {
  if (!t) return;
  if (t->gpu && t->gpu_free) t->gpu_free(t->gpu);
  delete t;
}

extern "C" int at_rigtrack_push(at_rigtrack* t, double stamp, const at_rigcal_frame* frames,
                                const at_rigtrack_odom* odom) {
  if (!t || !frames) return AT_E_INVALID;
  for (int i = 0; i < t->n_cams; i++)
    if (frames[i].n < 0 || (frames[i].n > 0 && (!frames[i].dets || !frames[i].poses))) return AT_E_INVALID;
  if (odom) {
    at_rig_extrinsics e;
    memcpy(e.R, odom->R, sizeof(e.R));
    memcpy(e.t, odom->t, sizeof(e.t));
    if (!rig_extrinsics_ok(e) || !positive(odom->sigma_rot) || !positive(odom->sigma_trans)) return AT_E_INVALID;
  }
  if (!odom) {  // a new chain
    t->n = 0;
    t->head = 0;
  }
  if (t->n == t->window) {  // the oldest leaves
    t->head = (t->head + 1) % t->window;
    t->n--;
  }
  const int s = (t->head + t->n) % t->window;
  const FpLayout lay = {t->lut.data(), t->tags.data(), t->max_hamming};
  for (int i = 0; i < t->n_cams; i++) {
    const HostCamSrc src = {frames[i].dets, frames[i].poses, frames[i].n};
    uint32_t cand[kFpSlots], id[kFpSlots];
    int m, dropped;
    fp_select(FpHostWave(), src, lay, cand, id, &m, &dropped);
    CalCamObs& o = t->obs[(size_t)s * t->n_cams + i];
    memset(&o, 0, sizeof(o));
    o.m = m;
    for (int j = 0; j < m; j++) {
      const int k = (int)cand[4 * j];
      o.ids[j] = (int32_t)id[4 * j];
      memcpy(o.p[j], src.p(k), sizeof(o.p[j]));
      memcpy(o.pose_R[j], src.pose_R(k), sizeof(o.pose_R[j]));
      memcpy(o.pose_t[j], src.pose_t(k), sizeof(o.pose_t[j]));
    }
  }
  TrkOdom& od = t->odom[(size_t)s];
  memset(&od, 0, sizeof(od));
  if (odom) memcpy(&od, odom, sizeof(od));
  else od.R[0] = od.R[4] = od.R[8] = od.sigma_rot = od.sigma_trans = 1.0;  // (never read: position 0)
  t->stamp[(size_t)s] = stamp;
  t->own_nt[(size_t)s] = -1;
  t->dev_stale[(size_t)s] = 1;
  t->n++;
  return t->n;
}

extern "C" int at_rigtrack_count(const at_rigtrack* t) { return t ? t->n : AT_E_INVALID; }

extern "C" int at_rigtrack_clear(at_rigtrack* t) {
  if (!t) return AT_E_INVALID;
  t->n = 0;
  t->head = 0;
  return AT_OK;
}

extern "C" int at_rigtrack_solve_host(at_rigtrack* t, at_rigtrack_result* out) {
  if (!t || !out || t->n < 1) return AT_E_INVALID;
  const size_t W = (size_t)t->window;
  TrkBufs b;
  memset(&b, 0, sizeof(b));
  trk_fill_bufs(*t, &b);
  std::vector<RigRecord> rec(W);
  std::vector<CalPose> pose[2] = {std::vector<CalPose>(W), std::vector<CalPose>(W)};
  std::vector<double> sums[2] = {std::vector<double>(W * kTrkSums), std::vector<double>(W * kTrkSums)};
  std::vector<double> instpx(W), cov(36);
  TrkCtl ctl;
  memset(&ctl, 0, sizeof(ctl));
  b.obs = t->obs.data();
  b.odom = t->odom.data();
  b.rec = rec.data();
  b.own = t->own.data();
  b.own_nt = t->own_nt.data();
  for (int q = 0; q < 2; q++) {
    b.pose[q] = pose[q].data();
    b.sums[q] = sums[q].data();
  }
  b.instpx = instpx.data();
  b.cov = cov.data();
  b.ctl = &ctl;
  b.lay = {t->lut.data(), t->tags.data(), t->max_hamming};

  const CalHostTeam tm;
  std::unique_ptr<RigShared> rsh(new RigShared());
  std::unique_ptr<TrkShared> sh(new TrkShared());
  std::unique_ptr<TrkSolveShared> ssh(new TrkSolveShared());
  for (int k = 0; k < t->n; k++)
    if (t->own_nt[(size_t)b.slot(k)] < 0) trk_start(tm, *rsh, b, b.slot(k));
  trk_fill(tm, b);
  if (!ctl.any) return AT_E_INVALID;
  for (int it = 0; it <= t->iters; it++) {
    for (int k = 0; k < t->n; k++) trk_accum(tm, *sh, b, k, it > 0);
    trk_solve(tm, *ssh, b, it == 0, it == t->iters);
  }
  for (int i = 0; i < 4; i++) t->ns[i] = 0;
  trk_finish(t, ctl, pose[ctl.which].data(), cov.data(), instpx.data(), t->own_nt.data(), out);
  return AT_OK;
}

extern "C" int at_rigtrack_instants(const at_rigtrack* t, at_rigtrack_instant* out, int cap) {
  if (!t || cap < 0 || (cap > 0 && !out)) return AT_E_INVALID;
  const int n = (int)t->instants.size();
  for (int i = 0; i < n && i < cap; i++) out[i] = t->instants[i];
  return n;
}

extern "C" int at_rigtrack_set_profiling(at_rigtrack* t, int on) {
  if (!t) return AT_E_INVALID;
  t->profiling = on != 0;
  return AT_OK;
}

extern "C" int at_rigtrack_stats(const at_rigtrack* t, uint64_t* out, int cap) {
  if (!t || !out || cap < 1) return AT_E_INVALID;
  uint64_t tags = 0;
  for (const at_rigtrack_instant& q : t->instants) tags += (uint64_t)q.n_tags;
  const uint64_t v[8] = {(uint64_t)t->result.n, tags, (uint64_t)t->result.accepted, (uint64_t)t->result.rejected,
                         t->ns[0], t->ns[1], t->ns[2], t->ns[3]};
  const int n = cap < 8 ? cap : 8;
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}
