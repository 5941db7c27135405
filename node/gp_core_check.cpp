// gp_core_check -- drives at_node::GamePieceCore with a stand-in engine (tests/test_gp_node.py).
//
//   gp_core_check W H frame.bgr tensor.f32 P C quality outdir
//
// frame.bgr: one W x H bgr8 frame; tensor.f32: the "network output", (4 + C) * P floats.  The
// stand-in engine keeps that tensor in device memory, copies the input it is handed back to
// the host (outdir/input.f32) and returns the tensor on a stream of its own.  The core runs
// twice: raw image (outdir/boxes.bin, names.txt, image.bgr), then JPEG (outdir/image.jpg).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "at_node.h"

namespace {
struct Engine {
  float* d_out = nullptr;
  hipStream_t stream = nullptr;
  size_t input_floats = 0;
  std::vector<float> seen;
  int calls = 0;
};

int infer(void* ctx, const float* d_input, const float** d_output, void** stream) {
  Engine* e = static_cast<Engine*>(ctx);
  e->seen.resize(e->input_floats);
  if (hipMemcpy(e->seen.data(), d_input, e->input_floats * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  e->calls++;
  *d_output = e->d_out;
  *stream = e->stream;
  return 0;
}

std::vector<char> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
void spill(const std::string& path, const void* p, size_t n) {
  std::ofstream f(path, std::ios::binary);
  f.write(static_cast<const char*>(p), (std::streamsize)n);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr, "usage: gp_core_check W H frame.bgr tensor.f32 P C quality outdir\n");
    return 2;
  }
  const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), P = std::atoi(argv[5]), C = std::atoi(argv[6]);
  const int quality = std::atoi(argv[7]);
  const std::string out = argv[8];
  const std::vector<char> frame = slurp(argv[3]), tensor = slurp(argv[4]);
  if (frame.size() != (size_t)W * H * 3 || tensor.size() != (size_t)(4 + C) * P * sizeof(float)) {
    std::fprintf(stderr, "gp_core_check: input sizes\n");
    return 2;
  }
  at_node::GamePieceParams prm;
  prm.num_predictions = P;
  prm.num_classes = C;
  prm.class_names = {"coral", "algae"};  // fewer names than classes: "unknown" beyond
  Engine eng;
  eng.input_floats = (size_t)prm.input_channels * prm.input_height * prm.input_width;
  try {
    at_node::GamePieceCore core(W, H, prm, infer, &eng);  // (creates the HIP context)
    if (hipMalloc((void**)&eng.d_out, tensor.size()) != hipSuccess || hipStreamCreate(&eng.stream) != hipSuccess ||
        hipMemcpy(eng.d_out, tensor.data(), tensor.size(), hipMemcpyHostToDevice) != hipSuccess) {
      std::fprintf(stderr, "gp_core_check: HIP set-up failed\n");
      return 1;
    }
    at_node::GamePieceOutputs res;
    at_node::ImageBuffer img;
    int rc = core.process(reinterpret_cast<const uint8_t*>(frame.data()), 1.0, &res, &img);
    if (rc != AT_OK) {
      std::fprintf(stderr, "gp_core_check: process: %s\n", at_strerror(rc));
      return 1;
    }
    spill(out + "/boxes.bin", res.boxes.data(), res.boxes.size() * sizeof(at_gp_box));
    std::string names;
    for (const std::string& s : res.class_names) names += s + "\n";
    spill(out + "/names.txt", names.data(), names.size());
    spill(out + "/image.bgr", img.data(), img.size());
    spill(out + "/input.f32", eng.seen.data(), eng.seen.size() * sizeof(float));
    core.set_image_jpeg(quality);
    at_node::GamePieceOutputs res2;
    rc = core.process(reinterpret_cast<const uint8_t*>(frame.data()), 2.0, &res2, &img);
    if (rc != AT_OK || res2.boxes.size() != res.boxes.size()) {
      std::fprintf(stderr, "gp_core_check: second process: %d\n", rc);
      return 1;
    }
    spill(out + "/image.jpg", img.data(), img.size());
    std::printf("{\"boxes\": %zu, \"status\": %d, \"infer_calls\": %d, \"jpeg_bytes\": %zu}\n", res.boxes.size(),
                res.status, eng.calls, img.size());
    (void)hipStreamDestroy(eng.stream);
    (void)hipFree(eng.d_out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "gp_core_check: %s\n", e.what());
    return 1;
  }
  return 0;
}
