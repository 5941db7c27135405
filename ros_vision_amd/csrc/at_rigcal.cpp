// at_rigcal.cpp -- the rig calibrator's host side: creation and its refusals, the stored
// instants (fp_select per camera when one is added), at_rigcal_solve_host -- the CPU twin of the
// k_cal_* kernels over the arithmetic of at_rigcal.h -- and the records of a finished solve.
// Host only (no HIP): at_rigcal_solve and the device buffers are at_api.cpp's.
#include "at_rigcal.h"

#include <string.h>

#include <cmath>
#include <memory>
#include <new>

namespace at {

static_assert(kCalMaxInstants == AT_RIGCAL_MAX_INSTANTS, "at_rigcal.h carries the ABI's instant cap");

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
}  // namespace

void cal_fill_bufs(const at_rigcal& c, CalBufs* b) {
  b->tag_size = c.tag_size;
  b->N = c.n;
  b->n_cams = c.n_cams;
  for (int i = 0; i < kRigMaxCams; i++) {
    const bool in = i < c.n_cams;
    b->fx[i] = in ? c.cams[i].cam.fx : 0.0;
    b->fy[i] = in ? c.cams[i].cam.fy : 0.0;
    b->cx[i] = in ? c.cams[i].cam.cx : 0.0;
    b->cy[i] = in ? c.cams[i].cam.cy : 0.0;
    b->free_rot[i] = in && c.cams[i].free_rot;
    b->free_trans[i] = in && c.cams[i].free_trans;
  }
}

void cal_finish(at_rigcal* c, const CalCtl& ctl, const CalPose* ext, const double* cov, const CalPose* pose,
                const double* instcost, const int32_t* ntags, at_rigcal_result* out) {
  at_rigcal_result r;
  memset(&r, 0, sizeof(r));
  const double corners = (double)ctl.corners;
  r.rms_before = ctl.corners > 0 ? sqrt(ctl.cost0 / corners) : 0.0;
  r.rms_after = ctl.corners > 0 ? sqrt(ctl.cost / corners) : 0.0;
  r.instants_used = ctl.used;
  r.instants_skipped = c->n - ctl.used;
  r.accepted = ctl.accepted;
  r.rejected = ctl.rejected;
  r.cov_valid = ctl.cov_valid;
  r.n_cams = c->n_cams;
  for (int i = 0; i < c->n_cams; i++) {
    memcpy(r.cams[i].R, ext[i].R, sizeof(r.cams[i].R));
    memcpy(r.cams[i].t, ext[i].t, sizeof(r.cams[i].t));
    for (int k = 0; k < 36; k++) r.cams[i].cov[k] = ctl.cov_valid ? cov[i * 36 + k] : 0.0;
  }
  c->instants.assign((size_t)c->n, at_rigcal_instant());
  for (int i = 0; i < c->n; i++) {
    at_rigcal_instant& q = c->instants[i];
    memset(&q, 0, sizeof(q));
    if (ntags[i] <= 0) continue;
    memcpy(q.R, pose[i].R, sizeof(q.R));
    memcpy(q.t, pose[i].t, sizeof(q.t));
    q.rms_px = sqrt(instcost[i] / (double)(4 * ntags[i]));
    q.n_tags = ntags[i];
    q.used = 1;
  }
  c->result = r;
  if (out) *out = r;
}

}  // namespace at

using namespace at;

extern "C" int at_rigcal_create(const at_rigcal_camera* cams, int n_cams, const at_field_tag* tags, int n_tags,
                                int max_hamming, double tag_size, at_rigcal** out) {
  if (!out || !cams || n_cams < 2 || n_cams > kRigMaxCams || max_hamming < 0 || n_tags < 1) return AT_E_INVALID;
  if (!(tag_size > 0) || !std::isfinite(tag_size)) return AT_E_INVALID;
  bool fixed = false, any_free = false;
  for (int i = 0; i < n_cams; i++) {
    if (!rig_extrinsics_ok(cams[i].extr)) return AT_E_INVALID;
    fixed = fixed || (!cams[i].free_rot && !cams[i].free_trans);
    any_free = any_free || cams[i].free_rot || cams[i].free_trans;
  }
  if (!fixed || !any_free) return AT_E_INVALID;
  std::unique_ptr<at_rigcal> c(new (std::nothrow) at_rigcal());
  if (!c) return AT_E_NOMEM;
  c->lut.resize(kFpMaxIds);
  const int rc = fp_build_layout(tags, n_tags, c->lut.data(), &c->tags);
  if (rc != AT_OK) return rc;
  c->n_cams = n_cams;
  c->max_hamming = max_hamming;
  c->tag_size = tag_size;
  for (int i = 0; i < n_cams; i++) {
    c->cams[i] = cams[i];
    c->cams[i].free_rot = cams[i].free_rot != 0;
    c->cams[i].free_trans = cams[i].free_trans != 0;
  }
  memset(&c->result, 0, sizeof(c->result));
  *out = c.release();
  return AT_OK;
}

extern "C" void at_rigcal_destroy(at_rigcal* c) {
  if (!c) return;
  if (c->gpu && c->gpu_free) c->gpu_free(c->gpu);
  delete c;
}

extern "C" int at_rigcal_add(at_rigcal* c, const at_rigcal_frame* frames) {
  if (!c || !frames) return AT_E_INVALID;
  for (int i = 0; i < c->n_cams; i++)
    if (frames[i].n < 0 || (frames[i].n > 0 && (!frames[i].dets || !frames[i].poses))) return AT_E_INVALID;
  if (c->n >= kCalMaxInstants) return AT_E_CAPACITY;
  const FpLayout lay = {c->lut.data(), c->tags.data(), c->max_hamming};
  std::vector<CalCamObs> inst((size_t)c->n_cams);
  int seen = 0;
  for (int i = 0; i < c->n_cams; i++) {
    const HostCamSrc src = {frames[i].dets, frames[i].poses, frames[i].n};
    uint32_t cand[kFpSlots], id[kFpSlots];
    int m, dropped;
    fp_select(FpHostWave(), src, lay, cand, id, &m, &dropped);
    CalCamObs& o = inst[i];
    memset(&o, 0, sizeof(o));
    o.m = m;
    for (int j = 0; j < m; j++) {
      const int k = (int)cand[4 * j];
      o.ids[j] = (int32_t)id[4 * j];
      memcpy(o.p[j], src.p(k), sizeof(o.p[j]));
      memcpy(o.pose_R[j], src.pose_R(k), sizeof(o.pose_R[j]));
      memcpy(o.pose_t[j], src.pose_t(k), sizeof(o.pose_t[j]));
    }
    seen += m > 0;
  }
  if (seen < 2) return 0;
  c->obs.insert(c->obs.end(), inst.begin(), inst.end());
  c->n++;
  c->obs_dirty = true;
  return 1;
}

extern "C" int at_rigcal_count(const at_rigcal* c) { return c ? c->n : AT_E_INVALID; }

extern "C" int at_rigcal_clear(at_rigcal* c) {
  if (!c) return AT_E_INVALID;
  c->obs.clear();
  c->n = 0;
  c->obs_dirty = true;
  return AT_OK;
}

extern "C" int at_rigcal_solve_host(at_rigcal* c, at_rigcal_result* out) {
  if (!c || !out || c->n < 1) return AT_E_INVALID;
  const int N = c->n, nc = c->n_cams;
  CalBufs b;
  memset(&b, 0, sizeof(b));
  cal_fill_bufs(*c, &b);
  const int E = b.E(), nch = b.chunks();
  std::vector<RigRecord> rec((size_t)N);
  std::vector<int32_t> ntags((size_t)N);
  std::vector<CalPose> pose[2] = {std::vector<CalPose>((size_t)N), std::vector<CalPose>((size_t)N)};
  std::vector<CalPose> ext[2] = {std::vector<CalPose>((size_t)nc), std::vector<CalPose>((size_t)nc)};
  std::vector<double> inst((size_t)N * b.inst_len()), part((size_t)N * E), chunk((size_t)nch * E), dc((size_t)b.M());
  std::vector<double> instcost((size_t)N), cov((size_t)nc * 36);
  CalCtl ctl;
  memset(&ctl, 0, sizeof(ctl));
  for (int i = 0; i < nc; i++) {
    memcpy(ext[0][i].R, c->cams[i].extr.R, sizeof(ext[0][i].R));
    memcpy(ext[0][i].t, c->cams[i].extr.t, sizeof(ext[0][i].t));
    ext[1][i] = ext[0][i];
  }
  b.obs = c->obs.data();
  b.rec = rec.data();
  b.ntags = ntags.data();
  for (int q = 0; q < 2; q++) {
    b.pose[q] = pose[q].data();
    b.ext[q] = ext[q].data();
  }
  b.inst = inst.data();
  b.part = part.data();
  b.chunk = chunk.data();
  b.dc = dc.data();
  b.instcost = instcost.data();
  b.cov = cov.data();
  b.ctl = &ctl;
  b.lay = {c->lut.data(), c->tags.data(), c->max_hamming};

  const CalHostTeam tm;
  std::unique_ptr<RigShared> rsh(new RigShared());
  std::unique_ptr<CalShared> sh(new CalShared());
  std::unique_ptr<CalSolveShared> ssh(new CalSolveShared());
  for (int i = 0; i < N; i++) cal_start(tm, *rsh, b, i);
  for (int i = 0; i < N; i++) cal_back(tm, *sh, b, i, false);
  cal_decide(tm, *ssh, b, false);
  for (int it = 0; it <= kCalIters; it++) {
    const bool final = it == kCalIters;
    for (int i = 0; i < N; i++) cal_accum(tm, *sh, b, i, final);
    for (int ch = 0; ch < nch; ch++)
      for (int e = 0; e < E; e++) cal_chunk_entry(b, ch, e);
    cal_reduced(tm, *ssh, b, final);
    if (final) break;
    for (int i = 0; i < N; i++) cal_back(tm, *sh, b, i, true);
    cal_decide(tm, *ssh, b, true);
  }
  for (int i = 0; i < N; i++) cal_back(tm, *sh, b, i, false);
  c->ns = 0;
  cal_finish(c, ctl, ext[ctl.which].data(), cov.data(), pose[ctl.which].data(), instcost.data(), ntags.data(), out);
  return AT_OK;
}

extern "C" int at_rigcal_instants(const at_rigcal* c, at_rigcal_instant* out, int cap) {
  if (!c || cap < 0 || (cap > 0 && !out)) return AT_E_INVALID;
  const int n = (int)c->instants.size();
  for (int i = 0; i < n && i < cap; i++) out[i] = c->instants[i];
  return n;
}

extern "C" int at_rigcal_set_profiling(at_rigcal* c, int on) {
  if (!c) return AT_E_INVALID;
  c->profiling = on != 0;
  return AT_OK;
}

extern "C" int at_rigcal_stats(const at_rigcal* c, uint64_t* out, int cap) {
  if (!c || !out || cap < 1) return AT_E_INVALID;
  const uint64_t v[5] = {(uint64_t)c->result.instants_used, (uint64_t)c->result.instants_skipped,
                         (uint64_t)c->result.accepted, (uint64_t)c->result.rejected, c->ns};
  const int n = cap < 5 ? cap : 5;
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}
