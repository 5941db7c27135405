// mjpg_entropy_host_check.cpp -- stand-alone driver of the parallel entropy decode's host
// form (ros_vision_amd/csrc/at_mjpg_entropy.h, at_mjpg_entropy_host in at_mjpg.cpp) for a
// sanitized build: tests/test_mjpg_entropy_host.py compiles the two files with the host
// compiler and -fsanitize=address,undefined and runs this program over good, truncated and
// corrupted streams read from files.
//
// usage: mjpg_entropy_host_check W H S[,S...] FILE...
//   Every file goes through at_mjpg_entropy_host at every piece size S, with chroma kept
//   and without, into a buffer of exactly the size the streams take, and through the
//   serial decoder (at_mjpg_dense_host).  Both must give the same code, and on success the
//   same bytes.  A refused stream is fine; reading or writing out of bounds is what the
//   sanitizers catch.  Prints one line; exit status 0 unless a call misbehaves.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ros_vision_amd/csrc/at_mjpg_entropy.h"

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s W H S[,S...] FILE...\n", argv[0]);
    return 2;
  }
  const int W = std::atoi(argv[1]), H = std::atoi(argv[2]);
  std::vector<int> sizes;
  for (const char* p = argv[3]; *p;) {
    sizes.push_back(std::atoi(p));
    while (*p && *p != ',') p++;
    if (*p) p++;
  }
  int ok = 0, refused = 0, most_rounds = 0;
  for (int i = 4; i < argc; i++) {
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
    for (int chroma = 0; chroma < 2; chroma++) {
      size_t need = 0;
      const int want = at_mjpg_dense_host(jpg.data(), jpg.size(), W, H, chroma, nullptr, 0, &need);
      std::vector<uint8_t> ref(need ? need : 1);
      if (want == at::kMjpgOk &&
          at_mjpg_dense_host(jpg.data(), jpg.size(), W, H, chroma, ref.data(), need, &need) != at::kMjpgOk) {
        std::fprintf(stderr, "%s: at_mjpg_dense_host failed after a good decode\n", argv[i]);
        return 1;
      }
      // a refused stream has no size of its own: give it what a good frame of this geometry takes
      const size_t cap = want == at::kMjpgOk ? need : at::MjpgDecoder::slot_bytes(W, H, true);
      for (int S : sizes) {
        std::vector<uint8_t> out(cap);
        int rounds = 0;
        const int rc = at_mjpg_entropy_host(jpg.data(), jpg.size(), W, H, S, chroma, out.data(), out.size(), &rounds);
        if (rc != want) {
          std::fprintf(stderr, "%s (chroma %d, S %d): code %d, the serial decoder gives %d\n", argv[i], chroma, S, rc,
                       want);
          return 1;
        }
        if (rc == at::kMjpgOk && std::memcmp(out.data(), ref.data(), need) != 0) {
          std::fprintf(stderr, "%s (chroma %d, S %d): coefficients differ\n", argv[i], chroma, S);
          return 1;
        }
        if (rounds > most_rounds) most_rounds = rounds;
      }
      if (want == at::kMjpgOk) ok++; else refused++;
    }
  }
  std::printf("decoded %d refused %d rounds %d\n", ok, refused, most_rounds);
  return 0;
}
