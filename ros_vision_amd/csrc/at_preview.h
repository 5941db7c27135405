// at_preview.h -- the preview stream, shared by host and device.
//
// A staged frame of any input format (BGR8, YUYV, GRAY8) becomes a small BGR8 image: a
// centred crop of pw * s x ph * s source pixels, every pixel converted to BGR8, then
// averaged per channel over its s x s box.  The existing draw and JPEG kernels then run
// at pw x ph.  Every integer operation of that definition lives here once, so the kernel
// (at_kernels.hip: k_preview) and the CPU reference (at_preview.cpp: at_preview_host)
// cannot drift apart.  Integers only; nothing here rounds in floating point.
//
// The YUYV conversion is written as OpenCV's fixed-point BT.601 limited-range
// COLOR_YUV2BGR_YUY2 from memory: no OpenCV was at hand to compare against, so parity
// with cv::cvtColor is NOT pinned by any test.  pv_yuyv_bgr below is the definition.
//
// Also here, because the preview's CPU reference draws on the host: the segment record
// of the annotated image and the two coverage tests k_draw runs per pixel (moved from
// at_kernels.hip unchanged, now __host__ __device__).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

// host and device (a plain C++ compiler builds at_preview.cpp too)
#if defined(__HIPCC__)
#define AT_PV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define AT_PV_HD static inline
#endif

namespace at {

// One 2-px-thick segment of the annotated image (at_draw_outlines_device).
struct DrawPrim {
  double x0, y0, x1, y1;
  uint8_t bgr[3];
};

// the pixels a segment can touch, clipped to the image; false: none
AT_PV_HD bool seg_box(const DrawPrim& q, int W, int H, int* x0, int* y0, int* bw, int* bh) {
  const double r = 1.0;  // thickness 2 / 2
  const int xa = (int)floor(fmin(q.x0, q.x1) - r), xb = (int)ceil(fmax(q.x0, q.x1) + r);
  const int ya = (int)floor(fmin(q.y0, q.y1) - r), yb = (int)ceil(fmax(q.y0, q.y1) + r);
  *x0 = xa > 0 ? xa : 0;
  *y0 = ya > 0 ? ya : 0;
  *bw = (xb < W - 1 ? xb : W - 1) - *x0 + 1;
  *bh = (yb < H - 1 ? yb : H - 1) - *y0 + 1;
  return *bw > 0 && *bh > 0;
}
AT_PV_HD bool seg_covers(const DrawPrim& q, int x, int y) {
  const double r = 1.0;
  const double dx = q.x1 - q.x0, dy = q.y1 - q.y0, l2 = dx * dx + dy * dy;
  double u = l2 > 0 ? ((x - q.x0) * dx + (y - q.y0) * dy) / l2 : 0.0;
  u = fmin(1.0, fmax(0.0, u));
  const double ex = q.x0 + u * dx - x, ey = q.y0 + u * dy - y;
  return ex * ex + ey * ey <= r * r;
}

// at_pixfmt
enum { kPvYuyv = 0, kPvBgr8 = 1, kPvGray8 = 2 };
constexpr int kPvMaxScale = 8;

// at_preview_size: pw = (W / s) & ~7, ph likewise (the encoder's multiples of 8), the
// crop of pw * s x ph * s source pixels centred
struct PvGeom {
  int W, H, s, pw, ph, ox, oy;
};
AT_PV_HD bool pv_geom(int W, int H, int s, PvGeom* g) {
  if (W < 1 || H < 1 || s < 1 || s > kPvMaxScale) return false;
  g->W = W;
  g->H = H;
  g->s = s;
  g->pw = (W / s) & ~7;
  g->ph = (H / s) & ~7;
  g->ox = (W - g->pw * s) / 2;
  g->oy = (H - g->ph * s) / 2;
  return g->pw >= 8 && g->ph >= 8;
}

AT_PV_HD int pv_bytes_per_pixel(int fmt) { return fmt == kPvBgr8 ? 3 : (fmt == kPvYuyv ? 2 : 1); }

AT_PV_HD int pv_sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One YUYV pixel (its Y, the U and V of its pair) to BGR8.  20-bit fixed point, BT.601
// limited range; >> of a negative sum is the arithmetic shift (floor).
AT_PV_HD void pv_yuyv_bgr(int Y, int U, int V, int* b, int* g, int* r) {
  const int y = (Y > 16 ? Y - 16 : 0) * 1220542 + (1 << 19);
  const int u = U - 128, v = V - 128;
  *r = pv_sat8((y + 1673527 * v) >> 20);
  *g = pv_sat8((y - 852492 * v - 409993 * u) >> 20);
  *b = pv_sat8((y + 2116026 * u) >> 20);
}

// the box average of one channel: sum of s * s values, rounded half up
AT_PV_HD int pv_avg(int sum, int s) { return (sum + (s * s) / 2) / (s * s); }

// source pixel (x, y) of a W-wide frame as BGR
AT_PV_HD void pv_src_bgr(const uint8_t* frame, int fmt, int W, int x, int y, int* b, int* g, int* r) {
  if (fmt == kPvBgr8) {
    const uint8_t* p = frame + ((size_t)y * W + x) * 3;
    *b = p[0];
    *g = p[1];
    *r = p[2];
  } else if (fmt == kPvYuyv) {
    const uint8_t* p = frame + ((size_t)y * W + (x & ~1)) * 2;  // Y0 U Y1 V
    pv_yuyv_bgr(p[(x & 1) * 2], p[1], p[3], b, g, r);
  } else {
    *b = *g = *r = frame[(size_t)y * W + x];
  }
}

// preview pixel (px, py): the definition, one source byte at a time (the CPU reference;
// k_preview reads the same rows with 8-byte loads and runs the same conversions)
AT_PV_HD void pv_pixel(const uint8_t* frame, int fmt, const PvGeom& g, int px, int py, uint8_t* out) {
  int sb = 0, sg = 0, sr = 0;
  for (int j = 0; j < g.s; j++)
    for (int i = 0; i < g.s; i++) {
      int b, gg, r;
      pv_src_bgr(frame, fmt, g.W, g.ox + px * g.s + i, g.oy + py * g.s + j, &b, &gg, &r);
      sb += b;
      sg += gg;
      sr += r;
    }
  out[0] = (uint8_t)pv_avg(sb, g.s);
  out[1] = (uint8_t)pv_avg(sg, g.s);
  out[2] = (uint8_t)pv_avg(sr, g.s);
}

}  // namespace at

// ---- host side (at_preview.cpp), used by the device path (at_api.cpp) and the CPU reference ----
#include <functional>
#include <vector>

#include "../../include/at_api.h"

namespace at {

// The segments of the annotated image in drawing order: tag outlines and id digits
// (node/at_node.cpp's draw_detection_outlines), box outlines (its draw_boxes) on a W x H image.
void outline_prims(const at_detection* dets, int n, std::vector<DrawPrim>* out);
void box_prims(int W, int H, const at_gp_box* boxes, int n, std::vector<DrawPrim>* out);

// Records mapped into the preview, before any segment is built: corners and centre
// (p - o) / s in double; boxes x' = (x - ox) / s, w' = w / s in float, likewise y and h.
// Then the preview's segments: boxes first, tag outlines on top, lines 2 px, glyphs at
// their fixed size.
void preview_prims(const PvGeom& g, const at_detection* dets, int n, const at_gp_box* boxes, int nb,
                   std::vector<DrawPrim>* out);

// The byte-budget search, one routine for both paths.  enc(q, limit, &len) encodes at quality
// q: AT_OK with the stream written and *len its size when that is <= limit, AT_E_CAPACITY
// with *len the size and nothing written otherwise, any other code on failure.
//   max_bytes == 0: one encode at `quality`.
//   max_bytes  > 0: encode at `quality`; if it does not fit, bisect on [1, quality - 1]
//   (mid = (lo + hi + 1) / 2; lo = mid if it fits, else hi = mid - 1; stop at lo == hi); the
//   result is the encode at lo (JPEG size is not strictly monotonic in quality: this rule,
//   not "the best q", is the contract).  Quality 1 not fitting: AT_E_CAPACITY, *len its
//   size, *quality_used = 1.  A stream that fits the budget but not `cap`: AT_E_CAPACITY at once.
// The last stream written is the result's: an encode that fits overwrites the one before, one
// that does not writes nothing, so no quality is encoded twice.  *encodes counts the calls:
// at most 2 + ceil(log2(quality - 1)).
typedef std::function<int(int q, size_t limit, size_t* len)> PvEncoder;
int preview_budget_search(int quality, size_t max_bytes, size_t cap, const PvEncoder& enc, size_t* len,
                          int* quality_used, int* encodes);

}  // namespace at
