// at_fieldmap.cpp -- the field mapper's host side: creation and its refusals, the stored views
// (fp_select when one is added), the placing of tags without a start (fm_place), and
// at_fieldmap_solve_host -- the CPU twin of the k_fm_* kernels over the arithmetic of
// at_fieldmap.h -- and the records of a finished solve.
// Host only (no HIP): at_fieldmap_solve and the device buffers are at_api.cpp's.
#include "at_fieldmap.h"

#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

namespace at {

static_assert(kFmMaxTags == AT_FIELDMAP_MAX_TAGS, "at_fieldmap.h carries the ABI's tag cap");
static_assert(kFmMaxViews == AT_FIELDMAP_MAX_VIEWS, "at_fieldmap.h carries the ABI's view cap");

// (at_fieldpose.cpp)
int fp_build_layout(const at_field_tag* tags, int n, int16_t* lut, std::vector<FpTag>* out);

namespace {
struct HostSrc {
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

// corner c of stored tag j of view o as a slot
FmSlot corner_slot(const FmObs& o, int j, int c, double hs) {
  FmSlot s;
  s.sx = (c == 0 || c == 3) ? -hs : hs;
  s.sy = c < 2 ? hs : -hs;
  s.u = o.p[j][c * 2];
  s.v = o.p[j][c * 2 + 1];
  s.tag = o.idx[j];
  s.valid = true;
  return s;
}

// the camera pose of view o by the field pose's start rule over its placed tags
bool view_cam_pose(const FmObs& o, const int8_t* placed, const CalPose* pose, double hs, CalPose* out) {
  double cost = HUGE_VAL;
  bool found = false;
  for (int j = 0; j < o.m; j++) {
    const int J = o.idx[j];
    if (!placed[J]) continue;
    CalPose c;
    double rt[3];
    fp_mul_abt(o.pose_R[j], pose[J].R, c.R);
    fp_rot(c.R, pose[J].t, rt);
    for (int k = 0; k < 3; k++) c.t[k] = o.pose_t[j][k] - rt[k];
    double cj = 0.0;
    for (int q = 0; q < o.m; q++) {
      if (!placed[o.idx[q]]) continue;
      for (int k = 0; k < 4; k++) cj = cj + fm_slot_cost(corner_slot(o, q, k, hs), o, pose[o.idx[q]], c.R, c.t);
    }
    if (cj < cost) {  // (a NaN or an infinite cost never wins; ties stay with the lower id)
      cost = cj;
      found = true;
      *out = c;
    }
  }
  if (found) fp_project_rotation(out->R);
  return found;
}

// at_fieldmap.h: "Placing"
void fm_place(const at_fieldmap& m, int8_t* placed, CalPose* pose) {
  const int T = m.n_tags;
  const double hs = m.tag_size / 2.0;
  std::vector<int> order((size_t)T);
  for (int J = 0; J < T; J++) order[J] = J;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return m.tags[a].tag.id < m.tags[b].tag.id; });
  struct Seen {
    int view, slot;
    CalPose cam;
  };
  std::vector<Seen> seen;
  for (bool changed = true; changed;) {
    changed = false;
    for (int J : order) {
      if (placed[J]) continue;
      seen.clear();
      for (int i = 0; i < m.n; i++) {
        const FmObs& o = m.obs[i];
        int jt = -1;
        for (int j = 0; j < o.m; j++)
          if (o.idx[j] == J) jt = j;
        Seen s = {i, jt, {}};
        if (jt >= 0 && view_cam_pose(o, placed, pose, hs, &s.cam)) seen.push_back(s);
      }
      double best = HUGE_VAL;
      bool found = false;
      CalPose pick = {};
      for (const Seen& s : seen) {
        const FmObs& o = m.obs[s.view];
        // (cam_T_field)^-1 cam_T_tag: R^T pose_R, R^T (pose_t - t)
        CalPose c;
        double Rt[9], d[3];
        for (int r = 0; r < 3; r++)
          for (int k = 0; k < 3; k++) Rt[r * 3 + k] = s.cam.R[k * 3 + r];
        fp_mul_ab(Rt, o.pose_R[s.slot], c.R);
        for (int k = 0; k < 3; k++) d[k] = o.pose_t[s.slot][k] - s.cam.t[k];
        fp_rot(Rt, d, c.t);
        fp_project_rotation(c.R);
        double cj = 0.0;
        for (const Seen& v : seen) {
          const FmObs& ov = m.obs[v.view];
          for (int k = 0; k < 4; k++) cj = cj + fm_slot_cost(corner_slot(ov, v.slot, k, hs), ov, c, v.cam.R, v.cam.t);
        }
        if (cj < best) {  // (ties stay with the lower view)
          best = cj;
          found = true;
          pick = c;
        }
      }
      if (!found) continue;
      pose[J] = pick;
      placed[J] = 1;
      changed = true;
    }
  }
}
}  // namespace

void fm_prepare(const at_fieldmap& m, FmBufs* b, CalPose* start, int16_t* lut, FpTag* lay_tags, int32_t* seen) {
  const int T = m.n_tags;
  b->tag_size = m.tag_size;
  b->N = m.n;
  b->T = T;
  memset(b->placed, 0, sizeof(b->placed));
  memset(b->free_rot, 0, sizeof(b->free_rot));
  memset(b->free_trans, 0, sizeof(b->free_trans));
  for (int J = 0; J < T; J++) {
    memset(&start[J], 0, sizeof(start[J]));
    if (!m.tags[J].known) continue;
    memcpy(start[J].R, m.tags[J].tag.R, sizeof(start[J].R));
    memcpy(start[J].t, m.tags[J].tag.t, sizeof(start[J].t));
    b->placed[J] = 1;
  }
  fm_place(m, b->placed, start);
  for (int J = 0; J < T; J++) seen[J] = 0;
  for (int i = 0; i < m.n; i++)
    for (int j = 0; j < m.obs[i].m; j++) seen[m.obs[i].idx[j]]++;
  for (int i = 0; i < kFpMaxIds; i++) lut[i] = -1;
  for (int J = 0; J < T; J++) {
    memset(&lay_tags[J], 0, sizeof(lay_tags[J]));
    if (!b->placed[J]) continue;
    memcpy(lay_tags[J].R, start[J].R, sizeof(lay_tags[J].R));
    memcpy(lay_tags[J].t, start[J].t, sizeof(lay_tags[J].t));
    lut[m.tags[J].tag.id] = (int16_t)J;
    b->free_rot[J] = m.tags[J].free_rot && seen[J] > 0;
    b->free_trans[J] = m.tags[J].free_trans && seen[J] > 0;
  }
}

void fm_finish(at_fieldmap* m, const FmBufs& b, const CalCtl& ctl, const CalPose* start, const int32_t* seen,
               const CalPose* tag, const double* cov, const CalPose* pose, const double* viewcost,
               const int32_t* ntags, at_fieldmap_result* out) {
  at_fieldmap_result r;
  memset(&r, 0, sizeof(r));
  const double corners = (double)ctl.corners;
  r.rms_before = ctl.corners > 0 ? sqrt(ctl.cost0 / corners) : 0.0;
  r.rms_after = ctl.corners > 0 ? sqrt(ctl.cost / corners) : 0.0;
  r.views_used = ctl.used;
  r.views_skipped = m->n - ctl.used;
  r.corners = ctl.corners;
  r.accepted = ctl.accepted;
  r.rejected = ctl.rejected;
  r.cov_valid = ctl.cov_valid;
  r.n_tags = m->n_tags;
  m->tag_results.assign((size_t)m->n_tags, at_fieldmap_tag_result());
  for (int J = 0; J < m->n_tags; J++) {
    at_fieldmap_tag_result& q = m->tag_results[J];
    memset(&q, 0, sizeof(q));
    q.id = m->tags[J].tag.id;
    q.views = seen[J];
    if (!b.placed[J]) continue;
    q.placed = 1;
    r.n_placed++;
    memcpy(q.R, tag[J].R, sizeof(q.R));
    memcpy(q.t, tag[J].t, sizeof(q.t));
    memcpy(q.R0, start[J].R, sizeof(q.R0));
    memcpy(q.t0, start[J].t, sizeof(q.t0));
    for (int k = 0; k < 36; k++) q.cov[k] = ctl.cov_valid ? cov[J * 36 + k] : 0.0;
  }
  m->views.assign((size_t)m->n, at_fieldmap_view());
  for (int i = 0; i < m->n; i++) {
    at_fieldmap_view& q = m->views[i];
    memset(&q, 0, sizeof(q));
    if (ntags[i] <= 0) continue;
    memcpy(q.R, pose[i].R, sizeof(q.R));
    memcpy(q.t, pose[i].t, sizeof(q.t));
    q.rms_px = sqrt(viewcost[i] / (double)(4 * ntags[i]));
    q.n_tags = ntags[i];
    q.used = 1;
  }
  m->result = r;
  if (out) *out = r;
}

}  // namespace at

using namespace at;

extern "C" int at_fieldmap_create(const at_fieldmap_tag* tags, int n, int max_hamming, double tag_size,
                                  at_fieldmap** out) {
  if (!out || !tags || n < 1 || n > kFmMaxTags || max_hamming < 0) return AT_E_INVALID;
  if (!(tag_size > 0) || !std::isfinite(tag_size)) return AT_E_INVALID;
  // the layout's checks: ids for every tag, the pose for the known ones (identity stands in for the rest)
  std::vector<at_field_tag> chk((size_t)n);
  bool anchor = false;
  for (int i = 0; i < n; i++) {
    chk[i] = tags[i].tag;
    if (!tags[i].known) {
      const at_field_tag eye = {tags[i].tag.id, {1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
      chk[i] = eye;
    }
    anchor = anchor || (tags[i].known && !tags[i].free_rot && !tags[i].free_trans);
  }
  if (!anchor) return AT_E_INVALID;
  std::unique_ptr<at_fieldmap> m(new (std::nothrow) at_fieldmap());
  if (!m) return AT_E_NOMEM;
  m->lut.resize(kFpMaxIds);
  std::vector<FpTag> unused;
  const int rc = fp_build_layout(chk.data(), n, m->lut.data(), &unused);
  if (rc != AT_OK) return rc;
  m->n_tags = n;
  m->max_hamming = max_hamming;
  m->tag_size = tag_size;
  for (int i = 0; i < n; i++) {
    m->tags[i] = tags[i];
    m->tags[i].tag = chk[i];
    m->tags[i].known = tags[i].known != 0;
    m->tags[i].free_rot = tags[i].free_rot != 0;
    m->tags[i].free_trans = tags[i].free_trans != 0;
    m->tags[i].pad = 0;
  }
  memset(&m->result, 0, sizeof(m->result));
  *out = m.release();
  return AT_OK;
}

extern "C" void at_fieldmap_destroy(at_fieldmap* m) {
  if (!m) return;
  if (m->gpu && m->gpu_free) m->gpu_free(m->gpu);
  delete m;
}

extern "C" int at_fieldmap_add(at_fieldmap* m, const at_detection* dets, const at_pose* poses, int n,
                               const at_camera* cam) {
  if (!m || !cam || n < 0 || (n > 0 && (!dets || !poses))) return AT_E_INVALID;
  if (m->n >= kFmMaxViews) return AT_E_CAPACITY;
  const FpLayout lay = {m->lut.data(), nullptr, m->max_hamming};
  const HostSrc src = {dets, poses, n};
  uint32_t cand[kFpSlots], id[kFpSlots];
  int sel, dropped;
  fp_select(FpHostWave(), src, lay, cand, id, &sel, &dropped);
  if (sel < 2) return 0;
  FmObs o;
  memset(&o, 0, sizeof(o));
  o.m = sel;
  o.dropped = dropped;
  for (int j = 0; j < sel; j++) {
    const int k = (int)cand[4 * j];
    o.ids[j] = (int32_t)id[4 * j];
    o.idx[j] = m->lut[id[4 * j]];
    memcpy(o.p[j], src.p(k), sizeof(o.p[j]));
    memcpy(o.pose_R[j], src.pose_R(k), sizeof(o.pose_R[j]));
    memcpy(o.pose_t[j], src.pose_t(k), sizeof(o.pose_t[j]));
  }
  o.fx = cam->fx;
  o.fy = cam->fy;
  o.cx = cam->cx;
  o.cy = cam->cy;
  m->obs.push_back(o);
  m->n++;
  m->obs_dirty = true;
  return 1;
}

extern "C" int at_fieldmap_count(const at_fieldmap* m) { return m ? m->n : AT_E_INVALID; }

extern "C" int at_fieldmap_clear(at_fieldmap* m) {
  if (!m) return AT_E_INVALID;
  m->obs.clear();
  m->n = 0;
  m->obs_dirty = true;
  return AT_OK;
}

extern "C" int at_fieldmap_solve_host(at_fieldmap* m, at_fieldmap_result* out) {
  if (!m || !out || m->n < 1) return AT_E_INVALID;
  const int N = m->n, T = m->n_tags;
  FmBufs b;
  memset(&b, 0, sizeof(b));
  std::vector<CalPose> start((size_t)T);
  std::vector<int16_t> lut(kFpMaxIds);
  std::vector<FpTag> lay_tags((size_t)T);
  std::vector<int32_t> seen((size_t)T);
  fm_prepare(*m, &b, start.data(), lut.data(), lay_tags.data(), seen.data());
  const int E = b.E(), nch = b.chunks(), M = b.M();
  std::vector<FpRecord> rec((size_t)N);
  std::vector<int32_t> ntags((size_t)N), tab((size_t)N * kFpMaxTags), inv((size_t)N * kFmMaxTags);
  std::vector<CalPose> pose[2] = {std::vector<CalPose>((size_t)N), std::vector<CalPose>((size_t)N)};
  std::vector<CalPose> tag[2] = {start, start};
  std::vector<double> view((size_t)N * kFmViewLen), chunk((size_t)nch * E), S((size_t)E), A((size_t)M * M),
      Lm((size_t)M * (M + 1) / 2), dc((size_t)M), viewcost((size_t)N), cov((size_t)T * 36);
  CalCtl ctl;
  memset(&ctl, 0, sizeof(ctl));
  b.obs = m->obs.data();
  b.rec = rec.data();
  b.ntags = ntags.data();
  for (int q = 0; q < 2; q++) {
    b.pose[q] = pose[q].data();
    b.tag[q] = tag[q].data();
  }
  b.view = view.data();
  b.tab = tab.data();
  b.inv = inv.data();
  b.chunk = chunk.data();
  b.S = S.data();
  b.A = A.data();
  b.dc = dc.data();
  b.viewcost = viewcost.data();
  b.cov = cov.data();
  b.ctl = &ctl;
  b.lay = {lut.data(), lay_tags.data(), m->max_hamming};

  const FmHostTeam tm;
  std::unique_ptr<FmShared> sh(new FmShared());
  std::unique_ptr<FmSolveShared> ssh(new FmSolveShared());
  const int items = b.pairs() + T;
  for (int i = 0; i < N; i++) fm_start(tm, b, i);
  for (int i = 0; i < N; i++) fm_back(tm, *sh, b, i, false);
  fm_decide(tm, *ssh, b, false);
  for (int it = 0; it <= kFmIters; it++) {
    const bool final = it == kFmIters;
    for (int i = 0; i < N; i++) fm_accum(tm, *sh, b, i, final);
    for (int ch = 0; ch < nch; ch++)
      for (int item = 0; item < items; item++)
        for (int e = 0; e < (item < b.pairs() ? 36 : 12); e++) fm_chunk_entry(b, ch, item, e);
    for (int e = 0; e < E; e++) fm_total(b, e);
    fm_solve(tm, *ssh, b, Lm.data(), final);
    if (final) break;
    for (int i = 0; i < N; i++) fm_back(tm, *sh, b, i, true);
    fm_decide(tm, *ssh, b, true);
  }
  for (int i = 0; i < N; i++) fm_back(tm, *sh, b, i, false);
  m->ns = 0;
  fm_finish(m, b, ctl, start.data(), seen.data(), tag[ctl.which].data(), cov.data(), pose[ctl.which].data(),
            viewcost.data(), ntags.data(), out);
  return AT_OK;
}

extern "C" int at_fieldmap_tags(const at_fieldmap* m, at_fieldmap_tag_result* out, int cap) {
  if (!m || cap < 0 || (cap > 0 && !out)) return AT_E_INVALID;
  const int n = (int)m->tag_results.size();
  for (int i = 0; i < n && i < cap; i++) out[i] = m->tag_results[i];
  return n;
}

extern "C" int at_fieldmap_views(const at_fieldmap* m, at_fieldmap_view* out, int cap) {
  if (!m || cap < 0 || (cap > 0 && !out)) return AT_E_INVALID;
  const int n = (int)m->views.size();
  for (int i = 0; i < n && i < cap; i++) out[i] = m->views[i];
  return n;
}

extern "C" int at_fieldmap_set_profiling(at_fieldmap* m, int on) {
  if (!m) return AT_E_INVALID;
  m->profiling = on != 0;
  return AT_OK;
}

extern "C" int at_fieldmap_stats(const at_fieldmap* m, uint64_t* out, int cap) {
  if (!m || !out || cap < 1) return AT_E_INVALID;
  uint64_t dropped = 0;
  for (const FmObs& o : m->obs) dropped += (uint64_t)o.dropped;
  const uint64_t v[6] = {(uint64_t)m->result.views_used, (uint64_t)m->result.views_skipped,
                         (uint64_t)m->result.accepted, (uint64_t)m->result.rejected, m->ns, dropped};
  const int n = cap < 6 ? cap : 6;
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}
