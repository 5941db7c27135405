// mjpg_host_check.cpp -- stand-alone driver of the host JPEG front end
// (ros_vision_amd/csrc/at_mjpg.cpp) for a sanitized build: tests/test_mjpg_host.py
// compiles the two files with the host compiler and -fsanitize=address,undefined
// and runs this program over truncated and corrupted streams read from files.
//
// usage: mjpg_host_check W H FILE...
//   Every file goes through the whole host path as the detector drives it for a
//   W x H camera: decode (parse + entropy decode), pack into a buffer of exactly the
//   size the detector reserves per frame, and the host IDCT to a W x H plane.  A
//   refused stream is fine; reading or writing out of bounds is what the sanitizers
//   catch.  Prints one line per file; exit status 0 unless a call misbehaves.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ros_vision_amd/csrc/at_mjpg.h"

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s W H FILE...\n", argv[0]);
    return 2;
  }
  const int W = std::atoi(argv[1]), H = std::atoi(argv[2]);
  const size_t nb = (size_t)(W / 8) * (H / 8);
  at::MjpgDecoder dec;  // reused, as a decode thread reuses its own
  int ok = 0, refused = 0;
  for (int i = 3; i < argc; i++) {
    std::FILE* f = std::fopen(argv[i], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot open %s\n", argv[i]);
      return 2;
    }
    std::vector<uint8_t> in;
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) in.insert(in.end(), buf, buf + n);
    std::fclose(f);
    // exact-size copy: a read past the end is a heap overflow the sanitizer sees
    std::vector<uint8_t> jpg(in.begin(), in.end());
    const int rc = dec.decode(jpg.data(), jpg.size(), W, H);
    if (rc != at::kMjpgOk) {
      if (rc != at::kMjpgInvalid && rc != at::kMjpgUnsupported) {
        std::fprintf(stderr, "%s: unexpected code %d\n", argv[i], rc);
        return 1;
      }
      refused++;
      continue;
    }
    std::vector<uint8_t> slot((size_t)at::kMjpgHdrBytes + 128 * nb);
    if (dec.packed_bytes() > slot.size() || dec.pack(slot.data(), slot.size()) != at::kMjpgOk) {
      std::fprintf(stderr, "%s: stream does not fit the frame slot\n", argv[i]);
      return 1;
    }
    std::vector<uint8_t> gray((size_t)W * H);
    if (dec.to_gray(gray.data(), gray.size()) != at::kMjpgOk) {
      std::fprintf(stderr, "%s: to_gray failed after a good decode\n", argv[i]);
      return 1;
    }
    // and the free-size entry point the bindings use
    int w = 0, h = 0;
    if (at_mjpg_decode_gray_host(jpg.data(), jpg.size(), gray.data(), gray.size(), &w, &h) != at::kMjpgOk || w != W ||
        h != H) {
      std::fprintf(stderr, "%s: at_mjpg_decode_gray_host disagrees\n", argv[i]);
      return 1;
    }
    ok++;
  }
  std::printf("decoded %d refused %d\n", ok, refused);
  return 0;
}
