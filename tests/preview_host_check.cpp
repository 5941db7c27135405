// preview_host_check.cpp -- at_preview_host and the byte-budget search driven stand-alone
// (built by tests/test_preview_host.py with -fsanitize=address,undefined together with
// csrc/at_preview.cpp and csrc/at_mjpg.cpp): frames of every format in exact-size heap
// buffers, the odd crops (328 x 248 and 72 x 56 at s = 1, 2, 3, 4, 8), records partly and
// wholly outside the crop, output buffers of exactly the size asked for, budgets that fit at
// the first quality, in the middle of the search and never, and a `cap` below the budget.
// Prints "ok <previews> <searches>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/at_api.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);              \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static at_detection det_at(int id, double cx, double cy, double half) {
  at_detection d;
  std::memset(&d, 0, sizeof(d));
  d.id = id;
  d.c[0] = cx;
  d.c[1] = cy;
  const double sx[4] = {-1, 1, 1, -1}, sy[4] = {1, 1, -1, -1};
  for (int k = 0; k < 4; k++) {
    d.p[k][0] = cx + sx[k] * half;
    d.p[k][1] = cy + sy[k] * half;
  }
  return d;
}

int main() {
  const int sizes[2][2] = {{328, 248}, {72, 56}};
  const int scales[5] = {1, 2, 3, 4, 8};
  const at_pixfmt fmts[3] = {AT_FMT_YUYV, AT_FMT_BGR8, AT_FMT_GRAY8};
  int previews = 0, searches = 0;
  for (const auto& sz : sizes) {
    const int w = sz[0], h = sz[1];
    // inside, across the left / top edge of every crop, beyond the right edge, far outside
    const at_detection dets[4] = {det_at(7, w / 2.0, h / 2.0, 20.5), det_at(123, 3.0, 5.0, 30.0),
                                  det_at(586, w - 2.0, h - 1.0, 25.0), det_at(1, -5000.0, 1e7, 40.0)};
    const at_gp_box boxes[3] = {{w / 2.0f, h / 2.0f, 50.f, 30.f, 0.9f, 0},
                                {-10.f, -10.f, 60.f, 60.f, 0.8f, 7},
                                {(float)w, (float)h, 1e9f, 40.f, 0.7f, -3}};
    for (at_pixfmt fmt : fmts) {
      const size_t fb = (size_t)w * h * (fmt == AT_FMT_BGR8 ? 3 : (fmt == AT_FMT_YUYV ? 2 : 1));
      uint8_t* frame = (uint8_t*)std::malloc(fb);  // exact size: a read past the frame is seen
      for (size_t i = 0; i < fb; i++) frame[i] = (uint8_t)rnd();
      for (int s : scales) {
        int pw = 0, ph = 0, ox = 0, oy = 0;
        if (at_preview_size(w, h, s, &pw, &ph, &ox, &oy) != AT_OK) {
          CHECK(w / s < 8 || h / s < 8);
          continue;
        }
        CHECK(pw % 8 == 0 && ph % 8 == 0 && ox >= 0 && oy >= 0 && ox + pw * s <= w && oy + ph * s <= h);
        const size_t ob = (size_t)pw * ph * 3;
        uint8_t* plain = (uint8_t*)std::malloc(ob);
        uint8_t* drawn = (uint8_t*)std::malloc(ob);
        CHECK(at_preview_host(frame, fmt, w, h, s, nullptr, 0, nullptr, 0, plain, ob) == AT_OK);
        CHECK(at_preview_host(frame, fmt, w, h, s, dets, 4, boxes, 3, drawn, ob) == AT_OK);
        CHECK(at_preview_host(frame, fmt, w, h, s, dets, 4, boxes, 3, drawn, ob - 1) == AT_E_INVALID);
        CHECK(std::memcmp(plain, drawn, ob) != 0);
        previews += 2;
        // the search: no budget; a budget the first quality meets; one in the middle; none
        const size_t most = at_jpeg_max_bytes(pw, ph, AT_JPEG_420);
        size_t len = 0, full = 0;
        int used = 0;
        uint8_t* big = (uint8_t*)std::malloc(most);
        CHECK(at_preview_jpeg_host(frame, fmt, w, h, s, dets, 4, boxes, 3, 90, AT_JPEG_420, 0, big, most, &full,
                                   &used) == AT_OK);
        CHECK(used == 90 && full > 100 && full <= most);
        const size_t budgets[4] = {full, full * 2 / 3, full / 3, 100};
        for (size_t budget : budgets) {
          uint8_t* out = (uint8_t*)std::malloc(budget);  // exactly the budget: cap == max_bytes
          const int rc = at_preview_jpeg_host(frame, fmt, w, h, s, dets, 4, boxes, 3, 90, AT_JPEG_420, budget, out,
                                              budget, &len, &used);
          if (rc == AT_OK) {
            CHECK(len <= budget && used >= 1 && used <= 90 && out[0] == 0xff && out[1] == 0xd8 &&
                  out[len - 2] == 0xff && out[len - 1] == 0xd9);
            CHECK(budget != full || used == 90);
          } else {
            CHECK(rc == AT_E_CAPACITY && used == 1 && len > budget);
          }
          CHECK(budget != 100 || rc == AT_E_CAPACITY);
          std::free(out);
          searches++;
        }
        // a cap below a budget the stream meets: the size needed, at once
        uint8_t* tiny = (uint8_t*)std::malloc(64);
        CHECK(at_preview_jpeg_host(frame, fmt, w, h, s, dets, 4, boxes, 3, 90, AT_JPEG_420, full, tiny, 64, &len,
                                   &used) == AT_E_CAPACITY);
        CHECK(len == full && used == 90);
        std::free(tiny);
        std::free(big);
        std::free(plain);
        std::free(drawn);
      }
      std::free(frame);
    }
  }
  std::printf("ok %d %d\n", previews, searches);
  return 0;
}
