// mjpg_color_host_check.cpp -- stand-alone driver of the colour half of the host JPEG
// front end (ros_vision_amd/csrc/at_mjpg.cpp) for a sanitized build:
// tests/test_mjpg_color_host.py compiles the two files with the host compiler and
// -fsanitize=address,undefined and runs this program over good, truncated and
// corrupted streams read from files.
//
// usage: mjpg_color_host_check W H FILE...
//   Every file goes through the host path as the detector drives it for a W x H camera
//   with colour on: decode with keep_chroma, pack (luma stream + the two chroma
//   sub-streams) into a buffer of exactly the size the detector reserves per frame,
//   and the host decode to a W x H BGR8 image.  The packed stream's own header is then
//   checked the way the kernels read it: the sub-stream offsets, their block counts and
//   payloads lie inside the bytes pack() reported.  A refused stream is fine (and must
//   carry one of the two refusal codes); reading or writing out of bounds is what the
//   sanitizers catch.  Prints one summary line; exit status 0 unless a call misbehaves.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ros_vision_amd/csrc/at_mjpg.h"

static uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  std::memcpy(&v, p, 4);
  return v;
}

// one plane's stream at s (bytes available: avail): header and payload inside
static bool stream_inside(const uint8_t* s, size_t avail, uint32_t want_nb) {
  if (avail < (size_t)at::kMjpgHdrBytes) return false;
  const uint32_t mode = rd32(s + at::kMjpgModeOff), ntok = rd32(s + at::kMjpgNtokOff), nb = rd32(s + at::kMjpgNblkOff);
  if (nb != want_nb) return false;
  const size_t pay = mode == at::kMjpgDense ? (size_t)128 * nb : (size_t)4 * (nb + 1) + (size_t)4 * ntok;
  if ((size_t)at::kMjpgHdrBytes + pay > avail) return false;
  if (mode == at::kMjpgSparse) {
    const uint8_t* off = s + at::kMjpgHdrBytes;
    for (uint32_t b = 0; b < nb; b++)
      if (rd32(off + 4 * b) > rd32(off + 4 * (b + 1))) return false;
    if (rd32(off + 4 * nb) != ntok) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s W H FILE...\n", argv[0]);
    return 2;
  }
  const int W = std::atoi(argv[1]), H = std::atoi(argv[2]);
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
    const int rc = dec.decode(jpg.data(), jpg.size(), W, H, true);
    if (rc != at::kMjpgOk) {
      if (rc != at::kMjpgInvalid && rc != at::kMjpgUnsupported) {
        std::fprintf(stderr, "%s: unexpected code %d\n", argv[i], rc);
        return 1;
      }
      refused++;
      continue;
    }
    std::vector<uint8_t> slot(at::MjpgDecoder::slot_bytes(W, H, true));
    const size_t bytes = dec.packed_bytes();
    if (bytes > slot.size() || dec.pack(slot.data(), slot.size()) != at::kMjpgOk) {
      std::fprintf(stderr, "%s: stream does not fit the frame slot\n", argv[i]);
      return 1;
    }
    // exactly packed_bytes() must do as well
    std::vector<uint8_t> tight(bytes);
    if (dec.pack(tight.data(), tight.size()) != at::kMjpgOk || std::memcmp(tight.data(), slot.data(), bytes) != 0) {
      std::fprintf(stderr, "%s: pack into packed_bytes() differs\n", argv[i]);
      return 1;
    }
    const uint32_t samp = rd32(tight.data() + at::kMjpgSampOff);
    const int ncomp = (int)(samp >> 16), hs = (int)(samp & 0xff), vs = (int)((samp >> 8) & 0xff);
    if (ncomp != dec.info().ncomp || hs != dec.info().hs || vs != dec.info().vs ||
        !stream_inside(tight.data(), bytes, dec.nblocks())) {
      std::fprintf(stderr, "%s: luma stream or sampling word wrong\n", argv[i]);
      return 1;
    }
    const uint32_t off[2] = {rd32(tight.data() + at::kMjpgCbOff), rd32(tight.data() + at::kMjpgCrOff)};
    if (ncomp == 1) {
      if (off[0] || off[1] || dec.chroma_nblocks()) {
        std::fprintf(stderr, "%s: a single-component frame with chroma sub-streams\n", argv[i]);
        return 1;
      }
    } else {
      for (int c = 0; c < 2; c++) {
        const bool in_range = off[c] >= (uint32_t)at::kMjpgHdrBytes && off[c] % at::kMjpgSubAlign == 0 && off[c] < bytes;
        if (!in_range || !stream_inside(tight.data() + off[c], bytes - off[c], dec.chroma_nblocks()) ||
            (int)rd32(tight.data() + off[c] + at::kMjpgHsOff) != hs ||
            (int)rd32(tight.data() + off[c] + at::kMjpgVsOff) != vs ||
            rd32(tight.data() + off[c] + at::kMjpgBwOff) != (uint32_t)((W + 8 * hs - 1) / (8 * hs))) {
          std::fprintf(stderr, "%s: chroma sub-stream %d outside the stream or mislabelled\n", argv[i], c);
          return 1;
        }
      }
      if (off[1] <= off[0]) {
        std::fprintf(stderr, "%s: sub-streams out of order\n", argv[i]);
        return 1;
      }
    }
    std::vector<uint8_t> bgr((size_t)W * H * 3);
    if (dec.to_bgr(bgr.data(), bgr.size()) != at::kMjpgOk) {
      std::fprintf(stderr, "%s: to_bgr failed after a good decode\n", argv[i]);
      return 1;
    }
    // and the free-size entry point the bindings use: the same image
    std::vector<uint8_t> again(bgr.size());
    int w = 0, h = 0;
    if (at_mjpg_decode_bgr_host(jpg.data(), jpg.size(), again.data(), again.size(), &w, &h) != at::kMjpgOk || w != W ||
        h != H || again != bgr) {
      std::fprintf(stderr, "%s: at_mjpg_decode_bgr_host disagrees\n", argv[i]);
      return 1;
    }
    // colour off again through the same decoder: no chroma left over
    if (dec.decode(jpg.data(), jpg.size(), W, H) != at::kMjpgOk || dec.chroma_nblocks() != 0 ||
        dec.packed_bytes() > (size_t)at::kMjpgHdrBytes + 128 * (size_t)dec.nblocks() ||
        dec.to_bgr(bgr.data(), bgr.size()) != at::kMjpgInvalid) {
      std::fprintf(stderr, "%s: colour-off decode after a colour-on one\n", argv[i]);
      return 1;
    }
    ok++;
  }
  std::printf("decoded %d refused %d\n", ok, refused);
  return 0;
}
