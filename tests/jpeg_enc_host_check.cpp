// jpeg_enc_host_check.cpp -- stand-alone driver of the host JPEG encoder
// (ros_vision_amd/csrc/at_mjpg.cpp) for a sanitized build: tests/test_jpeg_enc_host.py
// compiles the two files with the host compiler and -fsanitize=address,undefined and runs
// this program.
//
// usage: jpeg_enc_host_check
//   Images of the edge sizes (partial MCUs at the right, at the bottom, at both) are encoded
//   at every sampling and at the ends of the quality range, first into a buffer of the
//   worst-case size, then into heap buffers of exactly the stream's size and of one byte
//   less (AT_E_CAPACITY, the needed size reported): a write past either is a heap overflow
//   the sanitizer sees.  Every stream then goes through MjpgDecoder to a BGR8 image, which
//   must stay near the input where the quantisation is fine (quality 100), so the round
//   trip stays inside the library.  Prints one line; exit status 0 unless a call misbehaves.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ros_vision_amd/csrc/at_mjpg.h"

static uint32_t rng_state = 12345u;
static uint32_t rng() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int main() {
  const int sizes[][2] = {{24, 40}, {40, 24}, {8, 8}, {16, 16}, {64, 48}, {328, 248}};
  const int qualities[] = {1, 50, 100};
  int encoded = 0;
  for (const auto& wh : sizes)
    for (int sampling = 0; sampling < 3; sampling++)
      for (int kind = 0; kind < 2; kind++)
        for (int quality : qualities) {
          const int W = wh[0], H = wh[1];
          // exact-size input: a read past the end is a heap overflow
          std::vector<uint8_t> img((size_t)W * H * 3);
          for (size_t i = 0; i < img.size(); i++)
            img[i] = kind ? (uint8_t)rng() : (uint8_t)(((i / 3) % W) * 255 / W);  // noise / a smooth ramp
          const size_t most = at_jpeg_max_bytes(W, H, sampling);
          std::vector<uint8_t> big(most);
          size_t len = 0;
          if (!most || at_jpeg_encode_host(img.data(), W, H, quality, sampling, big.data(), big.size(), &len) !=
                           at::kMjpgOk || len == 0 || len > most) {
            std::fprintf(stderr, "%dx%d s%d q%d: encode failed or exceeded at_jpeg_max_bytes\n", W, H, sampling, quality);
            return 1;
          }
          std::vector<uint8_t> exact(len);
          size_t len2 = 0;
          if (at_jpeg_encode_host(img.data(), W, H, quality, sampling, exact.data(), exact.size(), &len2) !=
                  at::kMjpgOk || len2 != len) {
            std::fprintf(stderr, "%dx%d s%d q%d: exact-size buffer refused\n", W, H, sampling, quality);
            return 1;
          }
          std::vector<uint8_t> small(len - 1, 0xa5);
          size_t need = 0;
          if (at_jpeg_encode_host(img.data(), W, H, quality, sampling, small.data(), small.size(), &need) != -3 ||
              need != len) {
            std::fprintf(stderr, "%dx%d s%d q%d: short buffer not reported\n", W, H, sampling, quality);
            return 1;
          }
          for (uint8_t b : small)
            if (b != 0xa5) {
              std::fprintf(stderr, "%dx%d s%d q%d: short buffer written to\n", W, H, sampling, quality);
              return 1;
            }
          at::MjpgDecoder dec;
          if (dec.decode(exact.data(), exact.size(), W, H, true) != at::kMjpgOk || dec.info().restart == 0) {
            std::fprintf(stderr, "%dx%d s%d q%d: the library's decoder refuses the stream\n", W, H, sampling, quality);
            return 1;
          }
          std::vector<uint8_t> back((size_t)W * H * 3);
          if (dec.to_bgr(back.data(), back.size()) != at::kMjpgOk) {
            std::fprintf(stderr, "%dx%d s%d q%d: to_bgr failed\n", W, H, sampling, quality);
            return 1;
          }
          if (quality == 100 && kind == 0) {
            // a smooth image at unit quantisation: rounding only (colour conversion both ways,
            // DCT both ways, chroma filters on a ramp)
            for (size_t i = 0; i < img.size(); i++)
              if (std::abs((int)img[i] - (int)back[i]) > 6) {
                std::fprintf(stderr, "%dx%d s%d: round trip off by %d at %zu\n", W, H, sampling,
                             (int)img[i] - (int)back[i], i);
                return 1;
              }
          }
          encoded++;
        }
  // rejected arguments write nothing and report no length
  uint8_t px[8 * 8 * 3] = {0}, out[16];
  size_t len = 99;
  if (at_jpeg_encode_host(px, 8, 8, 0, 0, out, sizeof(out), &len) != at::kMjpgInvalid || len != 0 ||
      at_jpeg_encode_host(px, 8, 8, 101, 0, out, sizeof(out), &len) != at::kMjpgInvalid ||
      at_jpeg_encode_host(px, 8, 8, 50, 3, out, sizeof(out), &len) != at::kMjpgInvalid ||
      at_jpeg_encode_host(px, 12, 8, 50, 0, out, sizeof(out), &len) != at::kMjpgInvalid ||
      at_jpeg_max_bytes(12, 8, 0) != 0) {
    std::fprintf(stderr, "bad arguments accepted\n");
    return 1;
  }
  std::printf("encoded %d\n", encoded);
  return 0;
}
