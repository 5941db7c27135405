// Stand-alone check of at_gp_parse_host (csrc/at_gp.cpp), meant to be built with
// -fsanitize=address,undefined and run on its own: every `out` is a heap buffer of exactly
// the size the call may write, so one record too many is a report.  Prints "ok <cases>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/at_api.h"

static int cases = 0;

static void fail(const char* what, int line) {
  std::fprintf(stderr, "gp_parse_host_check: %s (line %d)\n", what, line);
  std::exit(1);
}
#define EXPECT(c) \
  do {            \
    if (!(c)) fail(#c, __LINE__); \
  } while (0)

// tensor of P predictions, C classes on the heap, exactly (4 + C) * P floats
struct Tensor {
  int P, C;
  float* v;
  Tensor(int p, int c) : P(p), C(c), v((float*)std::malloc(sizeof(float) * (size_t)(4 + c) * p)) {
    for (size_t i = 0; i < (size_t)(4 + c) * p; i++) v[i] = 0.0f;
  }
  ~Tensor() { std::free(v); }
  void box(int i, float x, float y, float w, float h, int cls, float s) {
    v[i] = x; v[P + i] = y; v[2 * P + i] = w; v[3 * P + i] = h;
    v[(size_t)(4 + cls) * P + i] = s;
  }
};

// runs with cap = 0 (out == NULL), then with an exact-size buffer, then with one of half the size
static int run(const Tensor& t, float conf, float iou, std::vector<at_gp_box>* boxes) {
  int n0 = -1;
  EXPECT(at_gp_parse_host(t.v, t.P, t.C, conf, iou, 640, 640, 1280, 720, nullptr, 0, &n0) == AT_OK);
  EXPECT(n0 >= 0);
  at_gp_box* out = (at_gp_box*)std::malloc(sizeof(at_gp_box) * (size_t)(n0 ? n0 : 1));
  int n1 = -1;
  EXPECT(at_gp_parse_host(t.v, t.P, t.C, conf, iou, 640, 640, 1280, 720, n0 ? out : nullptr, n0, &n1) == AT_OK);
  EXPECT(n1 == n0);
  boxes->assign(out, out + n0);
  std::free(out);
  const int half = n0 / 2;
  at_gp_box* small = (at_gp_box*)std::malloc(sizeof(at_gp_box) * (size_t)(half ? half : 1));
  int n2 = -1;
  EXPECT(at_gp_parse_host(t.v, t.P, t.C, conf, iou, 640, 640, 1280, 720, half ? small : nullptr, half, &n2) == AT_OK);
  EXPECT(n2 == n0);
  EXPECT(half == 0 || std::memcmp(small, boxes->data(), sizeof(at_gp_box) * (size_t)half) == 0);
  std::free(small);
  cases++;
  return n0;
}

int main() {
  std::vector<at_gp_box> b;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  {  // P = 1
    Tensor t(1, 1);
    t.box(0, 320, 320, 64, 32, 0, 0.9f);
    EXPECT(run(t, 0.25f, 0.45f, &b) == 1);
    EXPECT(b[0].x == 640.0f && b[0].y == 360.0f && b[0].w == 128.0f && b[0].h == 36.0f && b[0].cls == 0);
    t.v[4] = 0.1f;
    EXPECT(run(t, 0.25f, 0.45f, &b) == 0);
    t.v[4] = nan;
    EXPECT(run(t, 0.0f, 0.45f, &b) == 1 && b[0].conf == 0.0f && b[0].cls == 0);
  }
  {  // the chain: A suppresses B, B must not suppress C
    Tensor t(3, 2);
    t.box(0, 100, 100, 100, 100, 1, 0.9f);
    t.box(1, 130, 100, 100, 100, 1, 0.8f);
    t.box(2, 160, 100, 100, 100, 1, 0.7f);
    EXPECT(run(t, 0.25f, 0.45f, &b) == 2);
    EXPECT(b[0].conf == 0.9f && b[1].conf == 0.7f && b[1].cls == 1);
  }
  {  // every prediction a candidate, odd values everywhere, many classes
    const int P = 257, C = 5;
    Tensor t(P, C);
    unsigned s = 12345;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
    for (int i = 0; i < P; i++) {
      t.box(i, 640 * rnd(), 640 * rnd(), 200 * rnd(), 200 * rnd(), 0, 0.0f);
      for (int c = 0; c < C; c++) t.v[(size_t)(4 + c) * P + i] = rnd() - 0.3f;
    }
    const float odd[] = {nan, inf, -inf, -0.0f, 0.0f, -1.0f, 1e30f, 3e38f};
    for (int k = 0; k < 64; k++) t.v[(size_t)((k * 7) % (4 + C)) * P + (k * 37) % P] = odd[k % 8];
    EXPECT(run(t, 0.0f, 0.45f, &b) >= 1);
    EXPECT(run(t, -1.0f, 0.0f, &b) >= 1);
    EXPECT(run(t, 0.25f, -1.0f, &b) >= 1);
    int n = 0;
    EXPECT(at_gp_parse_host(t.v, P, C, 0.0f, 2.0f, 640, 640, 640, 640, nullptr, 0, &n) == AT_OK && n == P);
  }
  {  // rejected arguments write nothing
    Tensor t(2, 1);
    int n = 5;
    EXPECT(at_gp_parse_host(nullptr, 2, 1, 0.25f, 0.45f, 640, 640, 640, 640, nullptr, 0, &n) == AT_E_INVALID && n == 0);
    EXPECT(at_gp_parse_host(t.v, 2, 1, 0.25f, 0.45f, 640, 640, 640, 640, nullptr, 1, &n) == AT_E_INVALID);
    EXPECT(at_gp_parse_host(t.v, 0, 1, 0.25f, 0.45f, 640, 640, 640, 640, nullptr, 0, &n) == AT_E_INVALID);
    EXPECT(at_gp_parse_host(t.v, 2, 0, 0.25f, 0.45f, 640, 640, 640, 640, nullptr, 0, &n) == AT_E_INVALID);
    EXPECT(at_gp_parse_host(t.v, 2, 1, nan, 0.45f, 640, 640, 640, 640, nullptr, 0, &n) == AT_E_INVALID);
    EXPECT(at_gp_parse_host(t.v, 2, 1, 0.25f, inf, 640, 640, 640, 640, nullptr, 0, &n) == AT_E_INVALID);
    EXPECT(at_gp_parse_host(t.v, 2, 1, 0.25f, 0.45f, 0, 640, 640, 640, nullptr, 0, &n) == AT_E_INVALID);
    EXPECT(at_gp_parse_host(t.v, 2, 1, 0.25f, 0.45f, 640, 640, 640, 640, nullptr, 0, nullptr) == AT_E_INVALID);
    cases++;
  }
  std::printf("ok %d\n", cases);
  return 0;
}
