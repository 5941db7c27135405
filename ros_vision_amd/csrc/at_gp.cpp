// at_gp.cpp -- host side of the game-piece output parse: at_gp_parse_host, the CPU
// reference of k_gp_cand / k_gp_nms over the arithmetic of at_gp.h.  Host only (no HIP):
// a plain C++ compiler builds it.
#include <math.h>

#include <algorithm>
#include <vector>

#include "../../include/at_api.h"
#include "at_gp.h"

using namespace at;

static_assert(sizeof(at_gp_box) == sizeof(GpBox) && AT_GP_MAX_CANDIDATES == kGpMaxCand, "at_gp.h carries the ABI's box");

extern "C" int at_gp_parse_host(const float* raw, int num_predictions, int num_classes, float conf_thr, float iou_thr,
                                int model_w, int model_h, int orig_w, int orig_h, at_gp_box* out, int cap, int* n) {
  if (n) *n = 0;
  if (!raw || !n || cap < 0 || (cap > 0 && !out) || num_predictions < 1 || num_classes < 1 || !isfinite(conf_thr) ||
      !isfinite(iou_thr) || model_w < 1 || model_h < 1 || orig_w < 1 || orig_h < 1)
    return AT_E_INVALID;
  const size_t P = (size_t)num_predictions;
  struct Cand {
    uint64_t key;
    float best;
    int32_t cls;
  };
  std::vector<Cand> cand;
  for (size_t i = 0; i < P; i++) {
    float best;
    int32_t cls;
    gp_candidate(raw, P, num_classes, i, &best, &cls);
    if (gp_dropped(best, conf_thr)) continue;
    cand.push_back({gp_key(best, (uint32_t)i), best, cls});
  }
  std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.key < b.key; });
  const size_t nc = cand.size();
  std::vector<GpCorners> box(nc);
  for (size_t k = 0; k < nc; k++) {
    const size_t i = gp_key_index(cand[k].key);
    box[k] = gp_corners(raw[i], raw[P + i], raw[2 * P + i], raw[3 * P + i], cand[k].cls);
  }
  const float sx = gp_scale(orig_w, model_w), sy = gp_scale(orig_h, model_h);
  std::vector<uint8_t> suppressed(nc, 0);
  int kept = 0;
  for (size_t a = 0; a < nc; a++) {
    if (suppressed[a]) continue;
    if (kept < cap) {
      const size_t i = gp_key_index(cand[a].key);
      const GpBox o = gp_scaled(raw[i], raw[P + i], raw[2 * P + i], raw[3 * P + i], cand[a].best, cand[a].cls, sx, sy);
      out[kept].x = o.x;
      out[kept].y = o.y;
      out[kept].w = o.w;
      out[kept].h = o.h;
      out[kept].conf = o.conf;
      out[kept].cls = o.cls;
    }
    kept++;
    for (size_t b = a + 1; b < nc; b++)
      if (!suppressed[b] && gp_suppresses(box[a], box[b], iou_thr)) suppressed[b] = 1;
  }
  *n = kept;
  return AT_OK;
}
