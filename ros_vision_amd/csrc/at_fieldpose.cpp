// at_fieldpose.cpp -- at_field_pose_host, at_robot_in_field and the layout check: the CPU
// twin of k_field over the arithmetic of at_fieldpose.h.  Host only (no HIP): one thread
// holds the 64 corner slots a wave spreads over its lanes.
#include "at_fieldpose.h"

#include <string.h>

#include <cmath>

#include <vector>

#include "../../include/at_api.h"

namespace at {

static_assert(kFpMaxTags == AT_FIELD_MAX_TAGS, "at_fieldpose.h carries the ABI's tag cap");

// at_set_field_layout's argument check (ids in [0, kFpMaxIds), none twice, every R a
// rotation to 1e-6); on success the id table and the tags as the solver reads them.
int fp_build_layout(const at_field_tag* tags, int n, int16_t* lut, std::vector<FpTag>* out) {
  if (n < 0 || n > kFpMaxIds || (n > 0 && !tags)) return AT_E_INVALID;
  for (int i = 0; i < kFpMaxIds; i++) lut[i] = -1;
  out->clear();
  for (int i = 0; i < n; i++) {
    const at_field_tag& g = tags[i];
    if (g.id < 0 || g.id >= kFpMaxIds || lut[g.id] >= 0) return AT_E_INVALID;
    const double* R = g.R;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        const double v = R[r * 3] * R[c * 3] + R[r * 3 + 1] * R[c * 3 + 1] + R[r * 3 + 2] * R[c * 3 + 2];
        if (!(fabs(v - (r == c ? 1.0 : 0.0)) <= 1e-6)) return AT_E_INVALID;
      }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                       R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!(det > 0)) return AT_E_INVALID;
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(g.t[k])) return AT_E_INVALID;
    FpTag t;
    memcpy(t.R, g.R, sizeof(t.R));
    memcpy(t.t, g.t, sizeof(t.t));
    lut[g.id] = (int16_t)out->size();
    out->push_back(t);
  }
  return AT_OK;
}

void fp_write(const FpRecord& r, at_field_pose* o) {
  memset(o, 0, sizeof(*o));
  o->n_tags = r.n_tags;
  memcpy(o->ids, r.ids, sizeof(o->ids));
  memcpy(o->R, r.R, sizeof(o->R));
  memcpy(o->t, r.t, sizeof(o->t));
  o->rms_px = r.rms_px;
  o->steps_taken = r.steps_taken;
}

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
}  // namespace

}  // namespace at

using namespace at;

extern "C" {

int at_field_pose_host(const at_detection* dets, const at_pose* poses, int n, const at_field_tag* tags, int ntags,
                       int max_hamming, const at_camera* cam, double tag_size, at_field_pose* out) {
  if (!out || !cam || n < 0 || (n > 0 && (!dets || !poses)) || max_hamming < 0) return AT_E_INVALID;
  if (!(tag_size > 0) || !std::isfinite(tag_size)) return AT_E_INVALID;
  int16_t lut[kFpMaxIds];
  std::vector<FpTag> lt;
  const int rc = fp_build_layout(tags, ntags, lut, &lt);
  if (rc != AT_OK) return rc;
  const FpLayout lay = {lut, lt.data(), max_hamming};
  const FpCam fc = {cam->fx, cam->fy, cam->cx, cam->cy};
  const HostSrc src = {dets, poses, n};
  FpRecord rec = {};
  fp_solve_frame(FpHostWave(), src, lay, fc, tag_size, &rec, (FpRecord*)nullptr);
  fp_write(rec, out);
  return AT_OK;
}

// field_T_cam (robot_T_cam)^-1: the field pose holds cam_T_field = (R, t), the extrinsics
// robot_T_cam = (Re, te) (at_tag_detections' convention: robot = Re cam + te), so
// R_out = R^T Re^T and t_out = -R^T t - R_out te.
int at_robot_in_field(const at_field_pose* fp, const double* extr_R, const double* extr_t, double* R_out,
                      double* t_out) {
  if (!fp || !R_out || !t_out || fp->n_tags < 1) return AT_E_INVALID;
  static const double kEye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kZero[3] = {0, 0, 0};
  const double* Re = extr_R ? extr_R : kEye;
  const double* te = extr_t ? extr_t : kZero;
  const double* R = fp->R;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++)
      R_out[r * 3 + c] = R[0 * 3 + r] * Re[c * 3 + 0] + R[1 * 3 + r] * Re[c * 3 + 1] + R[2 * 3 + r] * Re[c * 3 + 2];
  for (int r = 0; r < 3; r++) {
    const double cam_in_field = -(R[0 * 3 + r] * fp->t[0] + R[1 * 3 + r] * fp->t[1] + R[2 * 3 + r] * fp->t[2]);
    t_out[r] = cam_in_field - (R_out[r * 3] * te[0] + R_out[r * 3 + 1] * te[1] + R_out[r * 3 + 2] * te[2]);
  }
  return AT_OK;
}

}  // extern "C"
