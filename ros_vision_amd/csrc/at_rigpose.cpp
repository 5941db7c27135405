// at_rigpose.cpp -- at_rig_pose_host: the CPU twin of k_rig over the arithmetic of
// at_rigpose.h, and at_rig_pose_robust_host: the twin of k_rig_robust over at_rigrobust.h.
// Host only (no HIP): one thread holds every slot of every camera, and RigShared, the kernel's
// LDS block, is a local.
#include "at_rigpose.h"
#include "at_rigrobust.h"

#include <string.h>

#include <cmath>
#include <memory>
#include <vector>

#include "../../include/at_api.h"

namespace at {

static_assert(kRigMaxCams == AT_RIG_MAX_CAMS, "at_rigpose.h carries the ABI's camera cap");
static_assert(sizeof(RigRecord) == sizeof(at_rig_pose), "RigRecord is at_rig_pose");
static_assert(sizeof(RigRobustCfg) == sizeof(at_rig_robust_config), "RigRobustCfg is at_rig_robust_config");
static_assert(sizeof(RigRobustInfo) == sizeof(at_rig_robust_info), "RigRobustInfo is at_rig_robust_info");

// (at_fieldpose.cpp)
int fp_build_layout(const at_field_tag* tags, int n, int16_t* lut, std::vector<FpTag>* out);

// extrinsics as at_rig_create and at_rig_pose_host take them: R a rotation to 1e-6, t finite
bool rig_extrinsics_ok(const at_rig_extrinsics& e) {
  const at_field_tag g = {0, {e.R[0], e.R[1], e.R[2], e.R[3], e.R[4], e.R[5], e.R[6], e.R[7], e.R[8]},
                          {e.t[0], e.t[1], e.t[2]}};
  int16_t lut[kFpMaxIds];
  std::vector<FpTag> lt;
  return fp_build_layout(&g, 1, lut, &lt) == AT_OK;
}

void rig_write(const RigRecord& r, at_rig_pose* o) { memcpy(o, &r, sizeof(*o)); }

// a config as at_rig_solve_robust and at_rig_pose_robust_host take it (NaN thresholds fail `> 0`)
bool rig_robust_config(const at_rig_robust_config* c, RigRobustCfg* out) {
  if (!c) return false;
  const RigRobustCfg r = {c->huber_px, c->reject_px, c->max_rounds, c->min_keep};
  *out = r;
  return rig_robust_cfg_ok(r);
}

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
struct HostRigSrc {
  const at_rig_host_cam* cams;
  HostCamSrc cam(int i) const { return {cams[i].dets, cams[i].poses, cams[i].n}; }
  RigCam rigcam(int i) const {
    const at_rig_host_cam& c = cams[i];
    RigCam r = {c.cam->fx, c.cam->fy, c.cam->cx, c.cam->cy, {}, {}};
    memcpy(r.ER, c.extr.R, sizeof(r.ER));
    memcpy(r.Et, c.extr.t, sizeof(r.Et));
    return r;
  }
};
}  // namespace

}  // namespace at

using namespace at;

extern "C" int at_rig_pose_host(const at_rig_host_cam* cams, int n_cams, const at_field_tag* tags, int n_tags,
                                int max_hamming, double tag_size, at_rig_pose* out) {
  if (!out || !cams || n_cams < 1 || n_cams > kRigMaxCams || max_hamming < 0 || n_tags < 1) return AT_E_INVALID;
  if (!(tag_size > 0) || !std::isfinite(tag_size)) return AT_E_INVALID;
  for (int i = 0; i < n_cams; i++) {
    const at_rig_host_cam& c = cams[i];
    if (!c.cam || c.n < 0 || (c.n > 0 && (!c.dets || !c.poses)) || !rig_extrinsics_ok(c.extr)) return AT_E_INVALID;
  }
  int16_t lut[kFpMaxIds];
  std::vector<FpTag> lt;
  const int rc = fp_build_layout(tags, n_tags, lut, &lt);
  if (rc != AT_OK) return rc;
  const FpLayout lay = {lut, lt.data(), max_hamming};
  const HostRigSrc src = {cams};
  std::unique_ptr<RigShared> sh(new RigShared());
  RigRecord rec = {};
  rig_solve_instant(RigHostTeam(), src, *sh, lay, n_cams, tag_size, &rec, (RigRecord*)nullptr);
  rig_write(rec, out);
  return AT_OK;
}

extern "C" int at_rig_pose_robust_host(const at_rig_host_cam* cams, int n_cams, const at_field_tag* tags, int n_tags,
                                       int max_hamming, double tag_size, const at_rig_robust_config* cfg,
                                       at_rig_pose* out, at_rig_robust_info* info) {
  if (!out || !info || !cams || n_cams < 1 || n_cams > kRigMaxCams || max_hamming < 0 || n_tags < 1)
    return AT_E_INVALID;
  if (!(tag_size > 0) || !std::isfinite(tag_size)) return AT_E_INVALID;
  RigRobustCfg rc_cfg;
  if (!rig_robust_config(cfg, &rc_cfg)) return AT_E_INVALID;
  for (int i = 0; i < n_cams; i++) {
    const at_rig_host_cam& c = cams[i];
    if (!c.cam || c.n < 0 || (c.n > 0 && (!c.dets || !c.poses)) || !rig_extrinsics_ok(c.extr)) return AT_E_INVALID;
  }
  int16_t lut[kFpMaxIds];
  std::vector<FpTag> lt;
  const int rc = fp_build_layout(tags, n_tags, lut, &lt);
  if (rc != AT_OK) return rc;
  const FpLayout lay = {lut, lt.data(), max_hamming};
  const HostRigSrc src = {cams};
  std::unique_ptr<RigRobustShared> sh(new RigRobustShared());
  RigRecord rec = {};
  RigRobustInfo inf = {};
  rig_solve_instant_robust(RigRobustHostTeam(), src, *sh, lay, n_cams, tag_size, rc_cfg, &rec, (RigRecord*)nullptr,
                           &inf, (RigRobustInfo*)nullptr);
  rig_write(rec, out);
  memcpy(info, &inf, sizeof(*info));
  return AT_OK;
}
