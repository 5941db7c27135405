// at_preview.cpp -- host side of the preview stream: the geometry, the mapping of the
// records into the preview, the segments of the annotated image, the byte-budget search and
// the CPU reference (at_preview_host, at_preview_jpeg_host) over the arithmetic of
// at_preview.h.  Host only (no HIP): a plain C++ compiler builds it.
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>

#include "at_gp.h"
#include "at_preview.h"

namespace at {

static_assert(kPvYuyv == AT_FMT_YUYV && kPvBgr8 == AT_FMT_BGR8 && kPvGray8 == AT_FMT_GRAY8,
              "at_preview.h carries the ABI's pixel formats");

// The segments of node/at_node.cpp's draw_detection_outlines, in its drawing order:
// per detection the four sides (apriltag_utils.cu:58-65: corners truncated to int
// as cv::Point does; 0-1 green, 0-3 red, 1-2 and 2-3 blue), then the id's digit
// strokes centred on c (:67-77).  The digit strokes are the node's.
void outline_prims(const at_detection* dets, int n, std::vector<DrawPrim>* out) {
  static const uint8_t kGreen[3] = {0, 0xff, 0}, kRed[3] = {0, 0, 0xff}, kBlue[3] = {0xff, 0, 0},
                       kText[3] = {0xff, 0x99, 0};
  static const std::vector<std::vector<std::pair<int, int>>> kDigits[10] = {
      {{{0, 1}, {1, 0}, {3, 0}, {4, 1}, {4, 7}, {3, 8}, {1, 8}, {0, 7}, {0, 1}}},
      {{{1, 2}, {2, 0}, {2, 8}}, {{1, 8}, {3, 8}}},
      {{{0, 1}, {1, 0}, {3, 0}, {4, 1}, {4, 3}, {0, 8}, {4, 8}}},
      {{{0, 0}, {4, 0}, {2, 3}, {3, 3}, {4, 4}, {4, 7}, {3, 8}, {1, 8}, {0, 7}}},
      {{{3, 8}, {3, 0}, {0, 5}, {4, 5}}},
      {{{4, 0}, {0, 0}, {0, 3}, {3, 3}, {4, 4}, {4, 7}, {3, 8}, {0, 8}}},
      {{{4, 0}, {2, 0}, {0, 3}, {0, 7}, {1, 8}, {3, 8}, {4, 7}, {4, 5}, {3, 4}, {0, 4}}},
      {{{0, 0}, {4, 0}, {1, 8}}},
      {{{1, 4}, {0, 3}, {0, 1}, {1, 0}, {3, 0}, {4, 1}, {4, 3}, {3, 4}, {1, 4}, {0, 5}, {0, 7}, {1, 8},
        {3, 8}, {4, 7}, {4, 5}, {3, 4}}},
      {{{4, 4}, {1, 4}, {0, 3}, {0, 1}, {1, 0}, {3, 0}, {4, 1}, {4, 5}, {2, 8}, {0, 8}}},
  };
  auto seg = [&](double x0, double y0, double x1, double y1, const uint8_t c[3]) {
    DrawPrim q;
    q.x0 = x0; q.y0 = y0; q.x1 = x1; q.y1 = y1;
    q.bgr[0] = c[0]; q.bgr[1] = c[1]; q.bgr[2] = c[2];
    out->push_back(q);
  };
  for (int i = 0; i < n; i++) {
    const at_detection& d = dets[i];
    auto P = [&](int k, int c) { return (double)(int)d.p[k][c]; };
    seg(P(0, 0), P(0, 1), P(1, 0), P(1, 1), kGreen);
    seg(P(0, 0), P(0, 1), P(3, 0), P(3, 1), kRed);
    seg(P(1, 0), P(1, 1), P(2, 0), P(2, 1), kBlue);
    seg(P(2, 0), P(2, 1), P(3, 0), P(3, 1), kBlue);
    const std::string text = std::to_string(d.id);
    const double sc = 2.5, adv = 7 * sc;
    const double tw = adv * text.size() - 2 * sc, th = 8 * sc;
    const double ox = (int)(d.c[0] - tw / 2), oy = (int)(d.c[1] - th / 2);
    for (size_t k = 0; k < text.size(); ++k) {
      if (text[k] < '0' || text[k] > '9') continue;
      for (const auto& stroke : kDigits[text[k] - '0'])
        for (size_t t = 1; t < stroke.size(); ++t)
          seg(ox + k * adv + stroke[t - 1].first * sc, oy + stroke[t - 1].second * sc, ox + k * adv + stroke[t].first * sc,
              oy + stroke[t].second * sc, kText);
    }
  }
}

// The rectangle of detection_test.cpp:84-100 as four 2-px segments in the class colour
// (top, right, bottom, left), as node/at_node.cpp's draw_boxes draws them.
// (node/at_node.cpp's draw_boxes restates gp_trunc, the clamp and the palette of at_gp.h on its
// own: change one, change the other -- tests/test_gp_parse_gpu.py compares the pixels.)
void box_prims(int W, int H, const at_gp_box* boxes, int n, std::vector<DrawPrim>* out) {
  std::vector<DrawPrim>& prims = *out;
  prims.reserve(prims.size() + (size_t)n * 4);
  for (int i = 0; i < n; i++) {
    GpBox b;
    memcpy(&b, boxes + i, sizeof(b));
    int x1, y1, x2, y2;
    gp_box_corners(b, W, H, &x1, &y1, &x2, &y2);
    const uint8_t* c = kGpPalette[((b.cls % 6) + 6) % 6];
    const int seg[4][4] = {{x1, y1, x2, y1}, {x2, y1, x2, y2}, {x2, y2, x1, y2}, {x1, y2, x1, y1}};
    for (const auto& s : seg) {
      DrawPrim q;
      q.x0 = s[0]; q.y0 = s[1]; q.x1 = s[2]; q.y1 = s[3];
      q.bgr[0] = c[0]; q.bgr[1] = c[1]; q.bgr[2] = c[2];
      prims.push_back(q);
    }
  }
}

static void map_records(const PvGeom& g, const at_detection* dets, int n, const at_gp_box* boxes, int nb,
                        std::vector<at_detection>* md, std::vector<at_gp_box>* mb) {
  md->assign(dets, dets + n);
  for (at_detection& d : *md) {
    for (auto& p : d.p) {
      p[0] = (p[0] - g.ox) / g.s;
      p[1] = (p[1] - g.oy) / g.s;
    }
    d.c[0] = (d.c[0] - g.ox) / g.s;
    d.c[1] = (d.c[1] - g.oy) / g.s;
  }
  mb->assign(boxes, boxes + nb);
  for (at_gp_box& b : *mb) {
    b.x = (b.x - (float)g.ox) / (float)g.s;
    b.y = (b.y - (float)g.oy) / (float)g.s;
    b.w = b.w / (float)g.s;
    b.h = b.h / (float)g.s;
  }
}

void preview_prims(const PvGeom& g, const at_detection* dets, int n, const at_gp_box* boxes, int nb,
                   std::vector<DrawPrim>* out) {
  std::vector<at_detection> md;
  std::vector<at_gp_box> mb;
  map_records(g, dets, n, boxes, nb, &md, &mb);
  box_prims(g.pw, g.ph, mb.data(), nb, out);
  outline_prims(md.data(), n, out);
}

int preview_budget_search(int quality, size_t max_bytes, size_t cap, const PvEncoder& enc, size_t* len,
                          int* quality_used, int* encodes) {
  *len = 0;
  *quality_used = quality;
  *encodes = 0;
  const size_t limit = max_bytes ? std::min(cap, max_bytes) : cap;
  // 1 fits (written), 0 over the budget (nothing written), < 0 the code to return
  auto run = [&](int q) -> int {
    size_t l = 0;
    const int rc = enc(q, limit, &l);
    ++*encodes;
    *len = l;
    *quality_used = q;
    if (rc == AT_OK) return 1;
    if (rc != AT_E_CAPACITY) return rc < 0 ? rc : AT_E_INVALID;
    return (!max_bytes || l <= max_bytes) ? AT_E_CAPACITY : 0;  // within the budget: `cap` is what is too small
  };
  int r = run(quality);
  if (r != 0) return r < 0 ? r : AT_OK;
  if (quality == 1) return AT_E_CAPACITY;
  int lo = 1, hi = quality - 1;
  size_t lo_len = 0;
  bool have = false;  // the stream at lo is the one written
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    r = run(mid);
    if (r < 0) return r;
    if (r) {
      lo = mid;
      lo_len = *len;
      have = true;
    } else {
      hi = mid - 1;
    }
  }
  if (!have) {  // lo == 1, not encoded yet
    r = run(1);
    if (r < 0) return r;
    if (!r) return AT_E_CAPACITY;  // *len its size, *quality_used 1, nothing written
    lo_len = *len;
  }
  *len = lo_len;
  *quality_used = lo;
  return AT_OK;
}

// the segments drawn in order, a later one over an earlier one (what k_draw's two passes give)
static void draw_prims_host(const std::vector<DrawPrim>& prims, uint8_t* bgr, int W, int H) {
  for (const DrawPrim& q : prims) {
    int x0, y0, bw, bh;
    if (!seg_box(q, W, H, &x0, &y0, &bw, &bh)) continue;
    for (int y = y0; y < y0 + bh; y++)
      for (int x = x0; x < x0 + bw; x++)
        if (seg_covers(q, x, y)) memcpy(bgr + ((size_t)y * W + x) * 3, q.bgr, 3);
  }
}

}  // namespace at

using namespace at;

extern "C" int at_preview_size(int width, int height, int scale, int* pw, int* ph, int* ox, int* oy) {
  PvGeom g;
  if (!pv_geom(width, height, scale, &g)) return AT_E_INVALID;
  if (pw) *pw = g.pw;
  if (ph) *ph = g.ph;
  if (ox) *ox = g.ox;
  if (oy) *oy = g.oy;
  return AT_OK;
}

extern "C" int at_preview_host(const uint8_t* frame, at_pixfmt fmt, int w, int h, int scale, const at_detection* dets,
                               int n, const at_gp_box* boxes, int nb, uint8_t* bgr_out, size_t cap) {
  PvGeom g;
  if (!frame || !bgr_out || n < 0 || (n > 0 && !dets) || nb < 0 || (nb > 0 && !boxes)) return AT_E_INVALID;
  if (fmt != AT_FMT_YUYV && fmt != AT_FMT_BGR8 && fmt != AT_FMT_GRAY8) return AT_E_INVALID;
  if (!pv_geom(w, h, scale, &g) || (fmt == AT_FMT_YUYV && (w & 1))) return AT_E_INVALID;
  if (cap < (size_t)g.pw * g.ph * 3) return AT_E_INVALID;
  for (int py = 0; py < g.ph; py++)
    for (int px = 0; px < g.pw; px++) pv_pixel(frame, fmt, g, px, py, bgr_out + ((size_t)py * g.pw + px) * 3);
  std::vector<DrawPrim> prims;
  preview_prims(g, dets, n, boxes, nb, &prims);
  draw_prims_host(prims, bgr_out, g.pw, g.ph);
  return AT_OK;
}

extern "C" int at_preview_jpeg_host(const uint8_t* frame, at_pixfmt fmt, int w, int h, int scale,
                                    const at_detection* dets, int n, const at_gp_box* boxes, int nb, int quality,
                                    int sampling, size_t max_bytes, uint8_t* out, size_t cap, size_t* len,
                                    int* quality_used) {
  if (len) *len = 0;
  if (quality_used) *quality_used = 0;
  PvGeom g;
  if (!out || !len || !pv_geom(w, h, scale, &g) || quality < 1 || quality > 100) return AT_E_INVALID;
  if (at_jpeg_max_bytes(g.pw, g.ph, sampling) == 0) return AT_E_INVALID;
  std::vector<uint8_t> img((size_t)g.pw * g.ph * 3);
  const int rc = at_preview_host(frame, fmt, w, h, scale, dets, n, boxes, nb, img.data(), img.size());
  if (rc != AT_OK) return rc;
  int qu = 0, encodes = 0;
  const int src = preview_budget_search(
      quality, max_bytes, cap,
      [&](int q, size_t limit, size_t* l) { return at_jpeg_encode_host(img.data(), g.pw, g.ph, q, sampling, out, limit, l); },
      len, &qu, &encodes);
  if (quality_used) *quality_used = qu;
  return src;
}
