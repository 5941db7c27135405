// at_gp.h -- the game-piece node's output parse, shared by host and device.
//
// What the reference node does with the network's output
// (game_piece_detection_node.cu:287-292 over yolo_detection.h:53-209):
// parse_yolov11_output (class maximum per prediction, confidence threshold), apply_nms
// (sort by confidence, greedy per-class suppression) and scale_detections.  The tensor
// is raw[(4 + C) * P]: rows of P floats, x, y, w, h, score_0 .. score_{C-1}.
//
// Every comparison and float operation of the contract lives here once, so the kernels
// (at_kernels.hip: k_gp_cand, k_gp_nms) and the CPU reference (at_gp.cpp:
// at_gp_parse_host) cannot drift apart.  float32 throughout; compile with
// -ffp-contract=off.  std::max / std::min are spelled out as the comparisons they are
// ((a < b) ? b : a and (b < a) ? b : a): fmaxf / fminf treat NaN differently.
//
// Where the reference leaves something open this pins it: candidates of equal
// confidence go in ascending prediction index (std::sort leaves ties unspecified; this
// is the result of a stable sort).
//
// Not drawn: the reference's label text and filled label background
// (detection_test.cpp:102-115) -- OpenCV's Hershey font is not carried here.  The box
// outline (gp_box_corners, colour kGpPalette[cls % 6]) is.
#pragma once

#include <stdint.h>
#include <string.h>


// host and device (hipcc builds at_gp.cpp too, without the HIP runtime header)
#if defined(__HIPCC__)
#define AT_GP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define AT_GP_HD static inline
#endif

namespace at {

constexpr int kGpMaxCand = 4096;  // AT_GP_MAX_CANDIDATES: candidates of one frame the device path sorts
constexpr int kGpCntStride = 32;  // words between two frames' candidate counters (GpParseBufs::cnt)

// at_gp_box
struct GpBox {
  float x, y, w, h, conf;
  int32_t cls;
};
static_assert(sizeof(GpBox) == 24, "GpBox: 24 B");

// Buffers of the device path (at_gp_parse_device), [max_batch] frames, allocated once.
struct GpParseBufs {
  uint32_t* cnt;   // [B][kGpCntStride] candidates of each frame (word 0 of a 128-B line of its own, so one
                   // frame's atomics never wait behind another's); counts on past kGpMaxCand; k_gp_nms leaves it 0
  uint64_t* key;   // [B][kGpMaxCand] gp_key of each candidate, in the order the atomics landed
  int32_t* cls;    // [B][kGpMaxCand] its class, same slot
  GpBox* out;      // [B][kGpMaxCand] kept boxes in NMS order (mapped host memory)
  uint32_t* info;  // [B][2] boxes kept, candidates (mapped host memory)
};

// a candidate as the sweep needs it: corners, area, class
struct GpCorners {
  float x1, y1, x2, y2, area;
  int32_t cls;
};

AT_GP_HD float gp_max(float a, float b) { return (a < b) ? b : a; }  // std::max(a, b)
AT_GP_HD float gp_min(float a, float b) { return (b < a) ? b : a; }  // std::min(a, b)

AT_GP_HD uint32_t gp_float_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
AT_GP_HD float gp_bits_float(uint32_t u) { return __builtin_bit_cast(float, u); }

// (a) parse_yolov11_output's inner loop (yolo_detection.h:148-164) for prediction i:
// the first class holding the maximum score above 0 (a NaN never wins; nothing above 0
// leaves class 0, confidence 0).  `stride` = P.  The prediction is a candidate unless
// gp_dropped(best, conf_thr).
AT_GP_HD void gp_candidate(const float* raw, size_t stride, int num_classes, size_t i, float* best, int32_t* cls) {
  float b = 0.0f;
  int32_t k = 0;
  const float* s = raw + 4 * stride + i;
  for (int c = 0; c < num_classes; c++) {
    const float v = s[(size_t)c * stride];
    if (v > b) {
      b = v;
      k = c;
    }
  }
  *best = b;
  *cls = k;
}
AT_GP_HD bool gp_dropped(float best, float conf_thr) { return best < conf_thr; }

// (b) the order as one integer: ascending key = descending confidence, ties by ascending
// prediction index.  best >= +0 always (it starts at 0.0f and only a greater score
// replaces it), so its bit pattern is monotonic.
AT_GP_HD uint64_t gp_key(float best, uint32_t i) { return ((uint64_t)(~gp_float_bits(best)) << 32) | i; }
AT_GP_HD uint32_t gp_key_index(uint64_t key) { return (uint32_t)key; }
AT_GP_HD float gp_key_conf(uint64_t key) { return gp_bits_float(~(uint32_t)(key >> 32)); }

// YoloDetection::x1() .. y2() (yolo_detection.h:27-30) and w * h
AT_GP_HD GpCorners gp_corners(float x, float y, float w, float h, int32_t cls) {
  GpCorners c;
  c.x1 = x - w / 2.0f;
  c.y1 = y - h / 2.0f;
  c.x2 = x + w / 2.0f;
  c.y2 = y + h / 2.0f;
  c.area = w * h;
  c.cls = cls;
  return c;
}

// (c) calculate_iou(a, b) (yolo_detection.h:53-65), a the kept box, b the later one
AT_GP_HD float gp_iou(const GpCorners& a, const GpCorners& b) {
  const float x1 = gp_max(a.x1, b.x1);
  const float y1 = gp_max(a.y1, b.y1);
  const float x2 = gp_min(a.x2, b.x2);
  const float y2 = gp_min(a.y2, b.y2);
  const float inter = gp_max(0.0f, x2 - x1) * gp_max(0.0f, y2 - y1);
  const float uni = (a.area + b.area) - inter;
  return uni > 0 ? inter / uni : 0.0f;
}
// apply_nms's test (yolo_detection.h:97-103): the kept box a suppresses the later b
AT_GP_HD bool gp_suppresses(const GpCorners& a, const GpCorners& b, float iou_thr) {
  return a.cls == b.cls && gp_iou(a, b) > iou_thr;
}

// (d) scale_detections (yolo_detection.h:194-209)
AT_GP_HD float gp_scale(int orig, int model) { return (float)orig / (float)model; }
AT_GP_HD GpBox gp_scaled(float x, float y, float w, float h, float conf, int32_t cls, float sx, float sy) {
  GpBox o;
  o.x = x * sx;
  o.y = y * sy;
  o.w = w * sx;
  o.h = h * sy;
  o.conf = conf;
  o.cls = cls;
  return o;
}

// ---- the drawn box (detection_test.cpp:73-100) --------------------------------------
// class colours, BGR: green, orange, blue, yellow, magenta, cyan
constexpr uint8_t kGpPalette[6][3] = {{0, 255, 0}, {0, 165, 255}, {255, 0, 0}, {0, 255, 255}, {255, 0, 255}, {255, 255, 0}};

// a float as cv::Point / static_cast<int> truncates it; NaN -> 0 and values beyond int
// saturate (the cast itself is undefined for them)
static inline int gp_trunc(float v) {
  if (!(v == v)) return 0;
  if (v >= 2147483520.0f) return 2147483520;
  if (v <= -2147483520.0f) return -2147483520;
  return (int)v;
}
// the rectangle's corners: truncated, then clamped to the image (:86-95)
static inline void gp_box_corners(const GpBox& b, int W, int H, int* x1, int* y1, int* x2, int* y2) {
  auto clampi = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
  *x1 = clampi(gp_trunc(b.x - b.w / 2.0f), W - 1);
  *y1 = clampi(gp_trunc(b.y - b.h / 2.0f), H - 1);
  *x2 = clampi(gp_trunc(b.x + b.w / 2.0f), W - 1);
  *y2 = clampi(gp_trunc(b.y + b.h / 2.0f), H - 1);
}

}  // namespace at
