// at_undist.cpp -- at_ideal_detections_host and at_undistort_points_host: the CPU twins of the
// head of the pose stage and of k_und_points over the arithmetic of at_undist.h.  Host only
// (no HIP): one thread does what a wave or a quad of lanes spreads out.
#include "at_undist.h"

#include <string.h>

#include "../../include/at_api.h"

namespace at {

static_assert(sizeof(at_camera) == sizeof(UndCam), "UndCam is at_camera");

static bool und_cam_ok(const at_camera* c) { return c && c->fx != 0.0 && c->fy != 0.0; }
static UndCam und_cam_of(const at_camera* c) {
  return UndCam{c->fx, c->fy, c->cx, c->cy, c->k1, c->k2, c->p1, c->p2, c->k3};
}

}  // namespace at

using namespace at;

extern "C" {

int at_ideal_detections_host(const at_camera* cam, const at_detection* dets, int n, at_detection* out) {
  if (!und_cam_ok(cam) || n < 0 || (n > 0 && (!dets || !out))) return AT_E_INVALID;
  const UndCam c = und_cam_of(cam);
  for (int i = 0; i < n; i++) {
    double A[72];
    UndRecord u;
    und_detection(c, dets[i].H, dets[i].c, dets[i].p, dets[i].id, A, &u);
    at_detection o = dets[i];
    o.id = u.id;
    memcpy(o.H, u.H, sizeof(u.H));
    memcpy(o.c, u.c, sizeof(u.c));
    memcpy(o.p, u.p, sizeof(u.p));
    out[i] = o;
  }
  return n;
}

int at_undistort_points_host(const at_camera* cam, const double* xy, int n, double* out_xy, uint8_t* ok) {
  if (!und_cam_ok(cam) || n < 0 || (n > 0 && (!xy || !out_xy || !ok))) return AT_E_INVALID;
  const UndCam c = und_cam_of(cam);
  for (int i = 0; i < n; i++) {
    double ou, ov;
    ok[i] = und_point(c, xy[2 * i], xy[2 * i + 1], &ou, &ov) ? 1 : 0;
    out_xy[2 * i] = ou;
    out_xy[2 * i + 1] = ov;
  }
  return n;
}

}  // extern "C"
