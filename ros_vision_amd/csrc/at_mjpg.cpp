// at_mjpg.cpp -- marker parser and Huffman decoder of the MJPG input path
// (at_mjpg.h).  Every read of the input is checked against its length; the decode
// loops are bounded by the picture's block count, so no input can make them spin.
#include "at_mjpg.h"
#include "at_mjpg_entropy.h"

#include <string.h>

namespace at {
namespace {

constexpr uint8_t kZigzag[64] = AT_MJPG_ZIGZAG;

// ITU-T T.81 Annex K.3 typical Huffman tables: what a stream without DHT segments
// (many UVC cameras) is coded with.  Slot 0: luminance, slot 1: chrominance.
constexpr uint8_t kStdDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kStdDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kStdDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kStdAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr uint8_t kStdAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kStdAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr uint8_t kStdAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

constexpr int kLookBits = 9;
constexpr size_t kMjpgMaxPixels = (size_t)1 << 26;  // larger pictures are refused, not attempted

struct Huff {
  bool defined = false;
  uint8_t vals[256] = {0};
  int32_t maxcode[18];   // largest code of each length, -1 if none; [17] stops the search
  int32_t valoff[17];    // vals index of the first code of each length, minus that code
  uint16_t look[1 << kLookBits];  // (length << 8) | symbol for codes of <= kLookBits bits, 0 otherwise
};

// JPEG's canonical code assignment (T.81 Annex C); false if the counts are no prefix code
bool huff_build(Huff* h, const uint8_t bits[16], const uint8_t* vals, int nvals) {
  int total = 0;
  for (int l = 0; l < 16; l++) total += bits[l];
  if (total > 256 || total != nvals) return false;
  memcpy(h->vals, vals, (size_t)nvals);
  memset(h->look, 0, sizeof(h->look));
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; l++) {
    const int n = bits[l - 1];
    if (code + n > (1 << l)) return false;
    h->valoff[l] = k - code;
    if (l <= kLookBits)
      for (int i = 0; i < n; i++) {
        const int first = (code + i) << (kLookBits - l);
        for (int j = 0; j < (1 << (kLookBits - l)); j++) h->look[first + j] = (uint16_t)((l << 8) | vals[k + i]);
      }
    k += n;
    code += n;
    h->maxcode[l] = n ? code - 1 : -1;
    code <<= 1;
  }
  h->maxcode[17] = 0x7fffffff;
  h->defined = true;
  return true;
}

// Entropy-coded segment reader: removes the 0x00 stuffed after 0xFF, stops at a
// marker (or the end of the input) and feeds zero bits from there on, counting them:
// a decode that consumed any of those ran past the data.
struct BitReader {
  const uint8_t* p;
  size_t len, pos;
  uint64_t acc = 0;
  int cnt = 0;       // valid bits in acc (low cnt bits)
  int fake = 0;      // of which zero bits supplied after the data ended
  BitReader(const uint8_t* d, size_t n, size_t at) : p(d), len(n), pos(at) {}
  void fill() {
    while (cnt <= 48) {
      uint32_t byte = 0;
      bool real = false;
      if (pos < len) {
        const uint8_t b = p[pos];
        if (b != 0xff) {
          byte = b;
          pos++;
          real = true;
        } else if (pos + 1 < len && p[pos + 1] == 0) {
          byte = 0xff;
          pos += 2;
          real = true;
        }  // else: a marker (or a lone 0xFF at the end): stay in front of it
      }
      if (!real) fake += 8;
      acc = (acc << 8) | byte;
      cnt += 8;
    }
  }
  // n <= 16
  uint32_t peek(int n) {
    if (cnt < n) fill();
    return (uint32_t)(acc >> (cnt - n)) & ((1u << n) - 1u);
  }
  void skip(int n) { cnt -= n; }
  bool overran() const { return fake > cnt; }
  void reset(size_t at) {
    pos = at;
    acc = 0;
    cnt = 0;
    fake = 0;
  }
};

// one Huffman symbol, or -1 (no code of up to 16 bits matches)
inline int huff_decode(BitReader& br, const Huff& h) {
  if (br.cnt < 16) br.fill();
  const uint32_t top = (uint32_t)(br.acc >> (br.cnt - 16)) & 0xffffu;
  const uint16_t e = h.look[top >> (16 - kLookBits)];
  if (e) {
    br.skip(e >> 8);
    return e & 0xff;
  }
  for (int l = kLookBits + 1; l <= 16; l++) {
    const int32_t code = (int32_t)(top >> (16 - l));
    if (code <= h.maxcode[l]) {
      br.skip(l);
      return h.vals[(code + h.valoff[l]) & 0xff];
    }
  }
  return -1;
}

// T.81 F.2.2.1 RECEIVE + EXTEND, 1 <= s <= 15
inline int receive_extend(BitReader& br, int s) {
  const int v = (int)br.peek(s);
  br.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

inline uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }

struct Comp {
  int id, h, v, tq, td, ta;
};

// What the marker parser leaves for the entropy decode (host or device).
struct Parsed {
  uint8_t qt[4][64];
  bool qt_def[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  Comp comp[3] = {};
  size_t scan_pos = 0;   // first byte of the scan data
  bool header_only = false;
};

// SOI .. SOS: sizes, sampling, tables (a slot no DHT filled takes the Annex K table of its
// kind).  want_w < 0: stops after the frame header (header_only).
int mjpg_parse(const uint8_t* jpg, size_t len, int want_w, int want_h, MjpgInfo* info, Parsed* P) {
  if (!jpg || len < 4 || jpg[0] != 0xff || jpg[1] != 0xd8) return kMjpgInvalid;
  uint8_t (&qt)[4][64] = P->qt;
  bool (&qt_def)[4] = P->qt_def;
  Huff (&dc)[4] = P->dc;
  Huff (&ac)[4] = P->ac;
  Comp (&comp)[3] = P->comp;
  P->header_only = false;
  bool have_sof = false;
  size_t pos = 2;
  for (;;) {
    // next marker: 0xFF fill bytes may precede it
    if (pos + 2 > len || jpg[pos] != 0xff) return kMjpgInvalid;
    while (pos < len && jpg[pos] == 0xff) pos++;
    if (pos >= len) return kMjpgInvalid;
    const uint8_t m = jpg[pos++];
    if (m == 0x00) return kMjpgInvalid;
    if (m == 0xd8 || m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;  // no segment
    if (m == 0xd9) return kMjpgInvalid;                                 // EOI before any scan
    if (pos + 2 > len) return kMjpgInvalid;
    const size_t L = be16(jpg + pos);
    if (L < 2 || pos + L > len) return kMjpgInvalid;
    const uint8_t* s = jpg + pos + 2;
    const size_t n = L - 2;
    pos += L;
    if (m == 0xc0) {  // SOF0
      if (have_sof || n < 6) return kMjpgInvalid;
      const int prec = s[0], h = (int)be16(s + 1), w = (int)be16(s + 3), nf = s[5];
      if (prec != 8) return kMjpgUnsupported;
      if (nf != 1 && nf != 3) return kMjpgUnsupported;
      if (n != (size_t)(6 + 3 * nf) || w <= 0 || h <= 0) return kMjpgInvalid;
      for (int i = 0; i < nf; i++) {
        comp[i].id = s[6 + 3 * i];
        comp[i].h = s[7 + 3 * i] >> 4;
        comp[i].v = s[7 + 3 * i] & 15;
        comp[i].tq = s[8 + 3 * i];
        if (comp[i].h < 1 || comp[i].h > 4 || comp[i].v < 1 || comp[i].v > 4 || comp[i].tq > 3) return kMjpgInvalid;
      }
      if (nf == 1) {
        comp[0].h = comp[0].v = 1;  // a single-component scan is not interleaved: blocks in raster order
      } else {
        const int lh = comp[0].h, lv = comp[0].v;
        if (!((lh == 1 && lv == 1) || (lh == 2 && lv == 1) || (lh == 2 && lv == 2))) return kMjpgUnsupported;
        for (int i = 1; i < 3; i++)
          if (comp[i].h != 1 || comp[i].v != 1) return kMjpgUnsupported;
      }
      info->width = w;
      info->height = h;
      info->ncomp = nf;
      info->hs = comp[0].h;
      info->vs = comp[0].v;
      have_sof = true;
      if ((want_w > 0 && w != want_w) || (want_h > 0 && h != want_h)) return kMjpgInvalid;
      if ((size_t)w * (size_t)h > kMjpgMaxPixels) return kMjpgInvalid;
      if (want_w < 0) {  // header only
        P->header_only = true;
        return kMjpgOk;
      }
    } else if ((m >= 0xc1 && m <= 0xcf) && m != 0xc4 && m != 0xc8) {
      return kMjpgUnsupported;  // extended, progressive, lossless, arithmetic (SOFn, DAC)
    } else if (m == 0xdb) {  // DQT
      size_t o = 0;
      while (o < n) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (pq != 0) return pq == 1 ? kMjpgUnsupported : kMjpgInvalid;
        if (tq > 3 || o + 65 > n) return kMjpgInvalid;
        memcpy(qt[tq], s + o + 1, 64);
        qt_def[tq] = true;
        o += 65;
      }
    } else if (m == 0xc4) {  // DHT
      size_t o = 0;
      while (o < n) {
        if (o + 17 > n) return kMjpgInvalid;
        const int tc = s[o] >> 4, th = s[o] & 15;
        if (tc > 1 || th > 3) return kMjpgInvalid;
        int cntv = 0;
        for (int l = 0; l < 16; l++) cntv += s[o + 1 + l];
        if (cntv > 256 || o + 17 + (size_t)cntv > n) return kMjpgInvalid;
        if (!huff_build(tc ? &ac[th] : &dc[th], s + o + 1, s + o + 17, cntv)) return kMjpgInvalid;
        o += 17 + (size_t)cntv;
      }
    } else if (m == 0xdd) {  // DRI
      if (n != 2) return kMjpgInvalid;
      info->restart = (int)be16(s);
    } else if (m == 0xda) {  // SOS
      if (!have_sof || n < 1) return kMjpgInvalid;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != (size_t)(4 + 2 * ns)) return kMjpgInvalid;
      if (ns != info->ncomp) return kMjpgUnsupported;  // one scan holds every component
      for (int i = 0; i < ns; i++) {
        if (s[1 + 2 * i] != comp[i].id) return kMjpgUnsupported;
        comp[i].td = s[2 + 2 * i] >> 4;
        comp[i].ta = s[2 + 2 * i] & 15;
        if (comp[i].td > 3 || comp[i].ta > 3) return kMjpgInvalid;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return kMjpgInvalid;
      break;
    }
    // APPn (the AVI1 APP0 of UVC cameras too), COM and every other segment: skipped
  }

  // tables the scan names; a slot no DHT filled takes the Annex K table of its kind
  if (!qt_def[comp[0].tq]) return kMjpgInvalid;
  for (int i = 0; i < info->ncomp; i++) {
    Huff& hd = dc[comp[i].td];
    Huff& ha = ac[comp[i].ta];
    if (!hd.defined) {
      if (comp[i].td > 1) return kMjpgInvalid;
      huff_build(&hd, comp[i].td ? kStdDcChrBits : kStdDcLumBits, kStdDcVals, 12);
      info->default_dht = 1;
    }
    if (!ha.defined) {
      if (comp[i].ta > 1) return kMjpgInvalid;
      huff_build(&ha, comp[i].ta ? kStdAcChrBits : kStdAcLumBits, comp[i].ta ? kStdAcChrVals : kStdAcLumVals, 162);
      info->default_dht = 1;
    }
  }
  P->scan_pos = pos;
  return kMjpgOk;
}

}  // namespace

uint32_t MjpgDecoder::decode_index(int bx, int by) const {
  // decode order of luma block (bx, by): MCU by MCU, hs x vs blocks in each
  const int hs = info_.hs, vs = info_.vs;
  const int mcux = gw_ / hs;
  const int mx = bx / hs, my = by / vs;
  return (uint32_t)(((my * mcux + mx) * vs + by % vs) * hs + bx % hs);
}

int MjpgDecoder::decode(const uint8_t* jpg, size_t len, int want_w, int want_h, bool keep_chroma) {
  info_ = MjpgInfo{};
  bw_ = bh_ = gw_ = gh_ = 0;
  kept_tokens_ = 0;
  chroma_ = false;
  cbw_ = cbh_ = 0;
  Parsed P;
  const int prc = mjpg_parse(jpg, len, want_w, want_h, &info_, &P);
  if (prc != kMjpgOk || P.header_only) return prc;
  const uint8_t (&qt)[4][64] = P.qt;
  const bool (&qt_def)[4] = P.qt_def;
  const Huff (&dc)[4] = P.dc;
  const Huff (&ac)[4] = P.ac;
  const Comp (&comp)[3] = P.comp;
  const size_t pos = P.scan_pos;
  for (int k = 0; k < 64; k++) q_[kZigzag[k]] = qt[comp[0].tq][k];
  const bool chroma = keep_chroma && info_.ncomp == 3;
  if (chroma)
    for (int c = 0; c < 2; c++) {
      // each component its own table: Cb and Cr may name different ones
      if (!qt_def[comp[c + 1].tq]) return kMjpgInvalid;
      for (int k = 0; k < 64; k++) cq_[c][kZigzag[k]] = qt[comp[c + 1].tq][k];
    }

  const int hs = info_.hs, vs = info_.vs;
  bw_ = (info_.width + 7) / 8;
  bh_ = (info_.height + 7) / 8;
  const int mcux = (bw_ + hs - 1) / hs, mcuy = (bh_ + vs - 1) / vs;
  gw_ = mcux * hs;
  gh_ = mcuy * vs;
  const size_t nluma = (size_t)gw_ * gh_;
  // (the lists keep their capacity from frame to frame; they grow with the data
  // decoded, never with what a header merely claims)
  tok_.clear();
  start_.clear();
  for (int c = 0; c < 2; c++) {
    ctok_[c].clear();
    cstart_[c].clear();
  }
  // where each component's tokens go: luma always, chroma only with colour on
  std::vector<uint32_t>* const tokv[3] = {&tok_, chroma ? &ctok_[0] : nullptr, chroma ? &ctok_[1] : nullptr};
  std::vector<uint32_t>* const startv[3] = {&start_, chroma ? &cstart_[0] : nullptr,
                                            chroma ? &cstart_[1] : nullptr};

  BitReader br(jpg, len, pos);
  int pred[3] = {0, 0, 0};
  const int nmcu = mcux * mcuy;
  const int ri = info_.restart;
  int rst = 0;
  const int nchroma = info_.ncomp == 3 ? 2 : 0;
  for (int mcu = 0; mcu < nmcu; mcu++) {
    if (ri && mcu && mcu % ri == 0) {
      // restart: the interval's data must have sufficed; drop the padding bits, find RSTn
      if (br.overran()) return kMjpgInvalid;
      size_t p = br.pos;
      while (p + 1 < len && !(jpg[p] == 0xff && jpg[p + 1] != 0 && jpg[p + 1] != 0xff)) p++;
      if (p + 1 >= len || jpg[p + 1] != 0xd0 + rst) return kMjpgInvalid;
      rst = (rst + 1) & 7;
      br.reset(p + 2);
      pred[0] = pred[1] = pred[2] = 0;
    }
    for (int b = 0; b < hs * vs + nchroma; b++) {
      const int ci = b < hs * vs ? 0 : b - hs * vs + 1;
      const Huff& hd = dc[comp[ci].td];
      const Huff& ha = ac[comp[ci].ta];
      std::vector<uint32_t>* const tk = tokv[ci];
      const bool keep = tk != nullptr;
      if (keep) startv[ci]->push_back((uint32_t)tk->size());
      const int t = huff_decode(br, hd);
      if (t < 0 || t > 15) return kMjpgInvalid;
      if (t) pred[ci] += receive_extend(br, t);
      pred[ci] = (int16_t)pred[ci];  // a coefficient is 16 bits (corrupt streams only get here)
      if (keep && pred[ci]) tk->push_back((uint32_t)(uint16_t)pred[ci]);
      for (int k = 1; k < 64;) {
        const int rs = huff_decode(br, ha);
        if (rs < 0) return kMjpgInvalid;
        const int r = rs >> 4, sz = rs & 15;
        if (!sz) {
          if (r != 15) break;  // EOB
          k += 16;
          continue;
        }
        k += r;
        if (k > 63) return kMjpgInvalid;
        const int v = receive_extend(br, sz);
        if (keep) tk->push_back(((uint32_t)k << 16) | (uint32_t)(uint16_t)v);
        k++;
      }
    }
    if (br.overran()) return kMjpgInvalid;  // truncated: stop early
  }
  start_.push_back((uint32_t)tok_.size());
  if (start_.size() != nluma + 1) return kMjpgInvalid;
  if (chroma) {
    // one block of each chroma component per MCU: the chroma grid is the MCU grid
    for (int c = 0; c < 2; c++) {
      cstart_[c].push_back((uint32_t)ctok_[c].size());
      if (cstart_[c].size() != (size_t)nmcu + 1) return kMjpgInvalid;
    }
    cbw_ = mcux;
    cbh_ = mcuy;
  }
  chroma_ = keep_chroma;
  uint32_t kept = 0;
  if (gw_ == bw_ && gh_ == bh_) {
    kept = (uint32_t)tok_.size();
  } else {
    for (int by = 0; by < bh_; by++)
      for (int bx = 0; bx < bw_; bx++) {
        const uint32_t i = decode_index(bx, by);
        kept += start_[i + 1] - start_[i];
      }
  }
  kept_tokens_ = kept;
  return kMjpgOk;
}

MjpgDecoder::Plane MjpgDecoder::plane(int c) const {
  if (c == 0) return Plane{q_, tok_.data(), start_.data(), bw_, bh_, kept_tokens_, true};
  const std::vector<uint32_t>& st = cstart_[c - 1];
  return Plane{cq_[c - 1], ctok_[c - 1].data(), st.data(), cbw_, cbh_, st.empty() ? 0u : st.back(), false};
}

bool MjpgDecoder::plane_dense(const Plane& p) {
  const size_t nb = (size_t)p.bw * p.bh;
  return 4 * (nb + 1) + 4 * (size_t)p.kept >= 128 * nb;
}

size_t MjpgDecoder::plane_bytes(const Plane& p, bool force_dense) {
  const size_t nb = (size_t)p.bw * p.bh;
  return (size_t)kMjpgHdrBytes + (force_dense || plane_dense(p) ? 128 * nb : 4 * (nb + 1) + 4 * (size_t)p.kept);
}

bool MjpgDecoder::dense() const { return plane_dense(plane(0)); }

static size_t sub_align(size_t n) { return (n + kMjpgSubAlign - 1) & ~(size_t)(kMjpgSubAlign - 1); }

size_t MjpgDecoder::packed_bytes() const {
  size_t n = plane_bytes(plane(0));
  if (chroma_ && cbw_)
    for (int c = 1; c < 3; c++) n = sub_align(n) + plane_bytes(plane(c));
  return n;
}

size_t MjpgDecoder::dense_bytes() const {
  size_t n = plane_bytes(plane(0), true);
  if (chroma_ && cbw_)
    for (int c = 1; c < 3; c++) n = sub_align(n) + plane_bytes(plane(c), true);
  return n;
}

size_t MjpgDecoder::slot_bytes(int w, int h, bool color) {
  const size_t one = (size_t)kMjpgHdrBytes + 128 * (size_t)((w + 7) / 8) * (size_t)((h + 7) / 8);
  return color ? 3 * sub_align(one) : one;
}

// header (q, mode, token count, block count) and payload of one plane
void MjpgDecoder::pack_plane(const Plane& p, uint8_t* dst, bool force_dense) const {
  const uint32_t nb = (uint32_t)(p.bw * p.bh);
  const bool dn = force_dense || plane_dense(p);
  memset(dst, 0, kMjpgHdrBytes);
  memcpy(dst, p.q, 64 * sizeof(uint16_t));
  const uint32_t mode = dn ? kMjpgDense : kMjpgSparse, ntok = dn ? 0 : p.kept;
  memcpy(dst + kMjpgModeOff, &mode, 4);
  memcpy(dst + kMjpgNtokOff, &ntok, 4);
  memcpy(dst + kMjpgNblkOff, &nb, 4);
  uint8_t* pay = dst + kMjpgHdrBytes;
  if (dn) {
    memset(pay, 0, (size_t)128 * nb);
    int16_t* out = reinterpret_cast<int16_t*>(pay);
    uint32_t b = 0;
    for (int by = 0; by < p.bh; by++)
      for (int bx = 0; bx < p.bw; bx++, b++) {
        const uint32_t i = block_index(p, bx, by);
        for (uint32_t t = p.start[i]; t < p.start[i + 1]; t++)
          out[(size_t)b * 64 + kZigzag[(p.tok[t] >> 16) & 63]] = (int16_t)(uint16_t)(p.tok[t] & 0xffffu);
      }
    return;
  }
  uint32_t* off = reinterpret_cast<uint32_t*>(pay);
  uint32_t* tk = off + nb + 1;
  uint32_t o = 0, b = 0;
  for (int by = 0; by < p.bh; by++)
    for (int bx = 0; bx < p.bw; bx++, b++) {
      const uint32_t i = block_index(p, bx, by);
      const uint32_t n = p.start[i + 1] - p.start[i];
      off[b] = o;
      if (n) memcpy(tk + o, p.tok + p.start[i], (size_t)n * 4);
      o += n;
    }
  off[nb] = o;
}

int MjpgDecoder::pack(uint8_t* dst, size_t cap) const { return pack_all(dst, cap, false); }
int MjpgDecoder::pack_dense(uint8_t* dst, size_t cap) const { return pack_all(dst, cap, true); }

int MjpgDecoder::pack_all(uint8_t* dst, size_t cap, bool fd) const {
  const uint32_t nb = nblocks();
  if (!dst || !nb || start_.size() != (size_t)gw_ * gh_ + 1 || cap < (fd ? dense_bytes() : packed_bytes()))
    return kMjpgInvalid;
  pack_plane(plane(0), dst, fd);
  if (!chroma_) return kMjpgOk;
  // colour on: the sampling word, then the chroma sub-streams behind the luma stream
  const uint32_t samp = (uint32_t)info_.hs | ((uint32_t)info_.vs << 8) | ((uint32_t)info_.ncomp << 16);
  memcpy(dst + kMjpgSampOff, &samp, 4);
  if (!cbw_) return kMjpgOk;  // a single-component frame: no sub-streams, offsets 0
  size_t at = plane_bytes(plane(0), fd);
  for (int c = 1; c < 3; c++) {
    const Plane p = plane(c);
    if (cstart_[c - 1].size() != (size_t)cbw_ * cbh_ + 1) return kMjpgInvalid;
    const size_t sub = sub_align(at);
    memset(dst + at, 0, sub - at);
    pack_plane(p, dst + sub, fd);
    const uint32_t off32 = (uint32_t)sub, bw = (uint32_t)cbw_, hs = (uint32_t)info_.hs, vs = (uint32_t)info_.vs;
    memcpy(dst + (c == 1 ? kMjpgCbOff : kMjpgCrOff), &off32, 4);
    memcpy(dst + sub + kMjpgBwOff, &bw, 4);
    memcpy(dst + sub + kMjpgHsOff, &hs, 4);
    memcpy(dst + sub + kMjpgVsOff, &vs, 4);
    at = sub + plane_bytes(p, fd);
  }
  return kMjpgOk;
}

void MjpgDecoder::idct_plane(const Plane& p, uint8_t* out, size_t stride, int w, int h) const {
  for (int by = 0; by < p.bh; by++)
    for (int bx = 0; bx < p.bw; bx++) {
      int32_t ws[64] = {0};
      const uint32_t i = block_index(p, bx, by);
      for (uint32_t t = p.start[i]; t < p.start[i + 1]; t++) {
        const int nat = kZigzag[(p.tok[t] >> 16) & 63];
        ws[nat] = (int32_t)(int16_t)(uint16_t)(p.tok[t] & 0xffffu) * (int32_t)p.q[nat];
      }
      for (int c = 0; c < 8; c++) {
        int32_t v[8];
        for (int r = 0; r < 8; r++) v[r] = ws[r * 8 + c];
        mjpg_idct_1d<11>(v);
        for (int r = 0; r < 8; r++) ws[r * 8 + c] = v[r];
      }
      for (int r = 0; r < 8; r++) {
        const int y = by * 8 + r;
        if (y >= h) break;
        int32_t v[8];
        for (int c = 0; c < 8; c++) v[c] = ws[r * 8 + c];
        mjpg_idct_1d<18>(v);
        for (int c = 0; c < 8 && bx * 8 + c < w; c++) out[(size_t)y * stride + bx * 8 + c] = (uint8_t)mjpg_pixel(v[c]);
      }
    }
}

int MjpgDecoder::to_gray(uint8_t* gray, size_t cap) const {
  const int W = info_.width, H = info_.height;
  if (!gray || !nblocks() || start_.size() != (size_t)gw_ * gh_ + 1 || cap < (size_t)W * H) return kMjpgInvalid;
  idct_plane(plane(0), gray, (size_t)W, W, H);
  return kMjpgOk;
}

int MjpgDecoder::to_bgr(uint8_t* bgr, size_t cap) const {
  const int W = info_.width, H = info_.height;
  if (!bgr || !nblocks() || !chroma_ || start_.size() != (size_t)gw_ * gh_ + 1 || cap < (size_t)W * H * 3)
    return kMjpgInvalid;
  std::vector<uint8_t> y((size_t)W * H);
  idct_plane(plane(0), y.data(), (size_t)W, W, H);
  if (!cbw_) {
    for (size_t i = 0; i < y.size(); i++) bgr[3 * i] = bgr[3 * i + 1] = bgr[3 * i + 2] = y[i];
    return kMjpgOk;
  }
  const int hs = info_.hs, vs = info_.vs;
  const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;  // the real chroma samples
  if (cw > cbw_ * 8 || ch > cbh_ * 8) return kMjpgInvalid;
  std::vector<uint8_t> cc[2];
  for (int c = 0; c < 2; c++) {
    if (cstart_[c].size() != (size_t)cbw_ * cbh_ + 1) return kMjpgInvalid;
    cc[c].resize((size_t)cw * ch);
    idct_plane(plane(c + 1), cc[c].data(), (size_t)cw, cw, ch);
  }
  for (int py = 0; py < H; py++) {
    // vertical neighbour of a 4:2:0 row: above for the even output row, below for the
    // odd one, the first / last real chroma row replicated
    const int j = py / vs, k = py & 1;
    const int n = k ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
    for (int px = 0; px < W; px++) {
      int32_t v[2];
      for (int c = 0; c < 2; c++) {
        const uint8_t* a = cc[c].data() + (size_t)j * cw;
        if (hs == 1) {
          v[c] = a[px];
          continue;
        }
        const int i = px >> 1, odd = px & 1;
        const int nb = odd ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
        if (vs == 1) {
          v[c] = mjpg_up_h2v1(a[i], a[nb], odd);
        } else {
          const uint8_t* an = cc[c].data() + (size_t)n * cw;
          v[c] = mjpg_up_h2v2(3 * a[i] + an[i], 3 * a[nb] + an[nb], odd);
        }
      }
      const uint32_t p = mjpg_bgr(y[(size_t)py * W + px], v[0], v[1]);
      uint8_t* o = bgr + ((size_t)py * W + px) * 3;
      o[0] = (uint8_t)p;
      o[1] = (uint8_t)(p >> 8);
      o[2] = (uint8_t)(p >> 16);
    }
  }
  return kMjpgOk;
}

}  // namespace at

extern "C" int at_mjpg_decode_gray_host(const uint8_t* jpg, size_t len, uint8_t* gray, size_t cap, int* w, int* h) {
  at::MjpgDecoder dec;
  if (w) *w = 0;
  if (h) *h = 0;
  // gray == NULL: the frame header only (the size a caller allocates for)
  const int rc = dec.decode(jpg, len, gray ? 0 : -1, 0);
  if (w) *w = dec.info().width;
  if (h) *h = dec.info().height;
  if (rc != at::kMjpgOk || !gray) return rc;
  return dec.to_gray(gray, cap);
}

extern "C" int at_mjpg_decode_bgr_host(const uint8_t* jpg, size_t len, uint8_t* bgr, size_t cap, int* w, int* h) {
  at::MjpgDecoder dec;
  if (w) *w = 0;
  if (h) *h = 0;
  const int rc = dec.decode(jpg, len, bgr ? 0 : -1, 0, true);
  if (w) *w = dec.info().width;
  if (h) *h = dec.info().height;
  if (rc != at::kMjpgOk || !bgr) return rc;
  return dec.to_bgr(bgr, cap);
}

extern "C" int at_mjpg_stream_mode_host(const uint8_t* jpg, size_t len, int want_w, int want_h,
                                        size_t* stream_bytes) {
  at::MjpgDecoder dec;
  const int rc = dec.decode(jpg, len, want_w > 0 ? want_w : 0, want_h > 0 ? want_h : 0);
  if (rc != at::kMjpgOk) return rc;
  if (stream_bytes) *stream_bytes = dec.packed_bytes();
  return dec.dense() ? 1 : 0;
}

// ---- device entropy decode: the marker parse, and the algorithm run on the host ----------
namespace at {

int mjpg_entropy_parse(const uint8_t* jpg, size_t len, int want_w, int want_h, bool keep_chroma, uint32_t subseq,
                       uint8_t* rec, size_t* scan_pos) {
  MjpgInfo info{};
  Parsed P;
  const int rc = mjpg_parse(jpg, len, want_w > 0 ? want_w : 0, want_h > 0 ? want_h : 0, &info, &P);
  if (rc != kMjpgOk) return rc;
  const bool chroma = keep_chroma && info.ncomp == 3;
  if (chroma)
    for (int c = 1; c < 3; c++)
      if (!P.qt_def[P.comp[c].tq]) return kMjpgInvalid;
  if (len - P.scan_pos > 0xfffffff0u) return kMjpgInvalid;
  EntGeom g{};
  g.scan_len = (uint32_t)(len - P.scan_pos);
  g.ncomp = (uint32_t)info.ncomp;
  g.hs = (uint32_t)info.hs;
  g.vs = (uint32_t)info.vs;
  g.bw = (uint32_t)((info.width + 7) / 8);
  g.bh = (uint32_t)((info.height + 7) / 8);
  g.mcux = (g.bw + g.hs - 1) / g.hs;
  g.mcuy = (g.bh + g.vs - 1) / g.vs;
  g.restart = (uint32_t)info.restart;
  g.keep_chroma = chroma ? 1 : 0;
  g.subseq = subseq;
  // the tables the scan names, each once
  EntTab* tabs = reinterpret_cast<EntTab*>(rec + kEntTabsOff);
  int slot_of[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};
  for (int i = 0; i < info.ncomp; i++)
    for (int cls = 0; cls < 2; cls++) {
      const int id = cls ? P.comp[i].ta : P.comp[i].td;
      if (slot_of[cls][id] < 0) {
        const Huff& h = cls ? P.ac[id] : P.dc[id];
        EntTab t;
        memset(&t, 0, sizeof(t));
        memcpy(t.look, h.look, sizeof(t.look));
        memcpy(t.maxcode + 1, h.maxcode + 1, 17 * sizeof(int32_t));
        memcpy(t.valoff + 1, h.valoff + 1, 16 * sizeof(int32_t));
        memcpy(t.vals, h.vals, sizeof(t.vals));
        memcpy(&tabs[g.ntab], &t, sizeof(t));
        slot_of[cls][id] = (int)g.ntab++;
      }
      g.tabsel |= (uint32_t)slot_of[cls][id] << (4 * (2 * i + cls));
    }
  const EntLayout L = ent_layout(g);
  g.cb_off = L.cb_off;
  g.cr_off = L.cr_off;
  memcpy(rec, &g, sizeof(g));
  // the stream headers, as pack() writes them for dense planes
  uint8_t* hdr = rec + kEntHdrsOff;
  memset(hdr, 0, 3 * (size_t)kMjpgHdrBytes);
  for (int c = 0; c < (L.cnb ? 3 : 1); c++) {
    uint8_t* h = hdr + (size_t)c * kMjpgHdrBytes;
    uint16_t q[64];
    for (int k = 0; k < 64; k++) q[kZigzag[k]] = P.qt[P.comp[c].tq][k];
    memcpy(h, q, sizeof(q));
    const uint32_t mode = kMjpgDense, nb = c ? L.cnb : L.nb;
    memcpy(h + kMjpgModeOff, &mode, 4);
    memcpy(h + kMjpgNblkOff, &nb, 4);
    if (c) {
      memcpy(h + kMjpgBwOff, &g.mcux, 4);
      memcpy(h + kMjpgHsOff, &g.hs, 4);
      memcpy(h + kMjpgVsOff, &g.vs, 4);
    }
  }
  if (keep_chroma) {
    const uint32_t samp = g.hs | (g.vs << 8) | (g.ncomp << 16);
    memcpy(hdr + kMjpgSampOff, &samp, 4);
    memcpy(hdr + kMjpgCbOff, &L.cb_off, 4);
    memcpy(hdr + kMjpgCrOff, &L.cr_off, 4);
  }
  *scan_pos = P.scan_pos;
  return kMjpgOk;
}

}  // namespace at

extern "C" int at_mjpg_entropy_host(const uint8_t* jpg, size_t len, int want_w, int want_h, int subseq_bytes,
                                    int keep_chroma, uint8_t* out, size_t cap, int* rounds) {
  using namespace at;
  if (rounds) *rounds = 0;
  if (subseq_bytes < 1) return kMjpgInvalid;  // (the kernel's pieces are 16 bytes or more; any size goes here)
  std::vector<uint8_t> rec(kEntRecordMax);
  size_t scan_pos = 0;
  // (any piece size goes here; one larger than the scan is one piece: the serial decode)
  const int rc = mjpg_entropy_parse(jpg, len, want_w, want_h, keep_chroma != 0, (uint32_t)subseq_bytes, rec.data(),
                                    &scan_pos);
  if (rc != kMjpgOk) return rc;
  EntGeom g;
  memcpy(&g, rec.data(), sizeof(g));
  const EntLayout L = ent_layout(g);
  if (!out || cap < L.total) return kMjpgInvalid;
  std::vector<EntTab> tabs(g.ntab);
  memcpy(tabs.data(), rec.data() + kEntTabsOff, g.ntab * sizeof(EntTab));
  const EntCtx c = ent_ctx(g, tabs.data(), jpg + scan_pos);
  const uint32_t np = ent_pieces(g), total = ent_total_blocks(g);

  // synchronise: round 0 from the guesses, then whoever's entry changed decodes again
  std::vector<uint64_t> entry(np), exitv(np);
  std::vector<uint32_t> nblk(np);
  std::vector<uint8_t> dirty(np, 0);
  auto run = [&](uint32_t i) {
    EntCount cnt;
    exitv[i] = ent_pack(ent_decode_piece(c, ent_unpack(entry[i]), ent_piece_end(c, i, np), cnt));
    nblk[i] = cnt.blocks;
  };
  for (uint32_t i = 0; i < np; i++) {
    EntState s0 = ent_guess(c, i);
    entry[i] = ent_pack(s0);
    run(i);
  }
  int nrounds = 1;
  for (uint32_t r = 1; r <= np; r++) {  // truth advances a piece a round: np rounds at the most
    bool changed = false;
    for (uint32_t i = 1; i < np; i++)
      if ((dirty[i] = exitv[i - 1] != entry[i])) {
        entry[i] = exitv[i - 1];
        changed = true;
      }
    if (!changed) break;
    for (uint32_t i = 1; i < np; i++)
      if (dirty[i]) run(i);
    nrounds++;
  }
  if (rounds) *rounds = nrounds;

  // place: each piece's first block; write: once more from the true states
  memset(out, 0, L.total);
  std::vector<int16_t> dcdiff(total ? total : 1, 0);
  EntOut o;
  o.luma = reinterpret_cast<int16_t*>(out + kMjpgHdrBytes);
  o.chroma[0] = L.cnb ? reinterpret_cast<int16_t*>(out + L.cb_off + kMjpgHdrBytes) : nullptr;
  o.chroma[1] = L.cnb ? reinterpret_cast<int16_t*>(out + L.cr_off + kMjpgHdrBytes) : nullptr;
  o.dcdiff = dcdiff.data();
  int err = 0;
  uint64_t first = 0;
  for (uint32_t i = 0; i < np; i++) {
    const EntState s = ent_unpack(entry[i]);
    // (pieces behind the picture's last block decode whatever follows it, into nothing)
    const uint32_t f32 = first > total ? total + 1 : (uint32_t)first;
    EntWrite w(&c, o, f32, s.zz != 0);
    ent_decode_piece(c, s, ent_piece_end(c, i, np), w);
    err |= w.err;
    first += nblk[i];
  }
  if (first < total) err |= kEntErrBlocks;
  if (err) {
    memset(out, 0, L.total);
    return kMjpgInvalid;
  }
  // DC: the segmented prefix sum, here as one range
  EntDcSum zero{};
  ent_dc_range(c, o, 0, g.mcux * g.mcuy, true, zero);
  memcpy(out, rec.data() + kEntHdrsOff, kMjpgHdrBytes);
  if (L.cnb) {
    memcpy(out + L.cb_off, rec.data() + kEntHdrsOff + kMjpgHdrBytes, kMjpgHdrBytes);
    memcpy(out + L.cr_off, rec.data() + kEntHdrsOff + 2 * (size_t)kMjpgHdrBytes, kMjpgHdrBytes);
  }
  return kMjpgOk;
}

extern "C" int at_mjpg_dense_host(const uint8_t* jpg, size_t len, int want_w, int want_h, int keep_chroma,
                                  uint8_t* out, size_t cap, size_t* out_bytes) {
  at::MjpgDecoder dec;
  if (out_bytes) *out_bytes = 0;
  const int rc = dec.decode(jpg, len, want_w > 0 ? want_w : 0, want_h > 0 ? want_h : 0, keep_chroma != 0);
  if (rc != at::kMjpgOk) return rc;
  if (out_bytes) *out_bytes = dec.dense_bytes();
  if (!out) return at::kMjpgOk;
  return dec.pack_dense(out, cap);
}

// ---- JPEG output: tables, header and the sequential host encoder ------------------------
namespace at {
namespace {

constexpr uint8_t kJpgQBase[2][64] = {AT_JPG_QBASE_LUMA, AT_JPG_QBASE_CHROMA};

// T.81 Annex C code assignment of one table into code | length << 16 per symbol
void jpg_huff_table(const uint8_t bits[16], const uint8_t* vals, uint32_t* tab, int nsym) {
  for (int i = 0; i < nsym; i++) tab[i] = 0;
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; l++) {
    for (int i = 0; i < bits[l - 1]; i++, k++, code++) tab[vals[k]] = code | ((uint32_t)l << 16);
    code <<= 1;
  }
}

size_t put_segment(uint8_t* p, uint8_t marker, const uint8_t* body, size_t n) {
  p[0] = 0xff;
  p[1] = marker;
  p[2] = (uint8_t)((n + 2) >> 8);
  p[3] = (uint8_t)(n + 2);
  memcpy(p + 4, body, n);
  return n + 4;
}

// one sample of component c (0 Y, 1 Cb, 2 Cr) of the picture as libjpeg sees it in front of
// the DCT: (x, y) in the component's own plane, which for chroma runs on past the real
// samples -- the last input column repeated before the downsampling, the last downsampled
// row after it
int32_t jpg_sample(const uint8_t* bgr, int w, const JpgGeom& g, int c, int x, int y) {
  auto px = [&](int xx, int yy) {
    const uint8_t* p = bgr + ((size_t)yy * w + (xx < w ? xx : w - 1)) * 3;
    return mjpg_ycc(c, p[2], p[1], p[0]);
  };
  if (c == 0 || g.hs == 1) return px(x, y);
  if (y > g.ch - 1) y = g.ch - 1;
  if (g.vs == 1) return mjpg_down_h2v1(px(2 * x, y), px(2 * x + 1, y), x);
  return mjpg_down_h2v2(px(2 * x, 2 * y), px(2 * x + 1, 2 * y), px(2 * x, 2 * y + 1), px(2 * x + 1, 2 * y + 1), x);
}

// forward DCT and quantisation of the block at (bx, by) of component c's plane: 64 values
// in zig-zag order
void jpg_block(const uint8_t* bgr, int w, const JpgGeom& g, int c, int bx, int by, const uint16_t* q, int16_t* zz) {
  int32_t ws[64];
  for (int r = 0; r < 8; r++) {
    int32_t v[8];
    for (int k = 0; k < 8; k++) v[k] = jpg_sample(bgr, w, g, c, bx * 8 + k, by * 8 + r) - 128;
    mjpg_fdct_1d<0>(v);
    for (int k = 0; k < 8; k++) ws[r * 8 + k] = v[k];
  }
  for (int k = 0; k < 8; k++) {
    int32_t v[8];
    for (int r = 0; r < 8; r++) v[r] = ws[r * 8 + k];
    mjpg_fdct_1d<1>(v);
    for (int r = 0; r < 8; r++) ws[r * 8 + k] = mjpg_quantise(v[r], q[r * 8 + k]);
  }
  for (int k = 0; k < 64; k++) zz[k] = (int16_t)ws[kZigzag[k]];
}

// entropy-coded segment writer: MSB first, FF -> FF 00
struct BitWriter {
  std::vector<uint8_t>* out;
  uint64_t acc = 0;
  int cnt = 0;
  void byte(uint8_t b) {
    out->push_back(b);
    if (b == 0xff) out->push_back(0);
  }
  void put(uint32_t code, int len) {  // len <= 32
    acc = (acc << len) | code;
    cnt += len;
    while (cnt >= 8) {
      byte((uint8_t)(acc >> (cnt - 8)));
      cnt -= 8;
    }
  }
  void flush() {  // pad with 1-bits to a byte
    if (cnt) put((1u << (8 - cnt)) - 1u, 8 - cnt);
    acc = 0;
  }
};

void jpg_code_block(BitWriter& bw, const int16_t* zz, int pred, const uint32_t* dc, const uint32_t* ac) {
  const int diff = zz[0] - pred;
  int n = mjpg_nbits(diff, 11);
  bw.put(dc[n] & 0xffffu, (int)(dc[n] >> 16));
  if (n) bw.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
  int run = 0;
  for (int k = 1; k < 64; k++) {
    const int v = zz[k];
    if (!v) {
      run++;
      continue;
    }
    for (; run > 15; run -= 16) bw.put(ac[0xf0] & 0xffffu, (int)(ac[0xf0] >> 16));
    n = mjpg_nbits(v, 10);
    const uint32_t e = ac[(run << 4) | n];
    bw.put(e & 0xffffu, (int)(e >> 16));
    bw.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
    run = 0;
  }
  if (run) bw.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));
}

}  // namespace

void jpg_huff_tables(uint32_t* tab) {
  jpg_huff_table(kStdDcLumBits, kStdDcVals, tab, kJpgDcTab);
  jpg_huff_table(kStdDcChrBits, kStdDcVals, tab + kJpgDcTab, kJpgDcTab);
  jpg_huff_table(kStdAcLumBits, kStdAcLumVals, tab + 2 * kJpgDcTab, kJpgAcTab);
  jpg_huff_table(kStdAcChrBits, kStdAcChrVals, tab + 2 * kJpgDcTab + kJpgAcTab, kJpgAcTab);
}

size_t jpg_write_header(uint8_t* dst, int w, int h, int quality, int sampling) {
  JpgGeom g;
  if (!jpg_geom(w, h, sampling, &g)) return 0;
  uint8_t* p = dst;
  *p++ = 0xff;
  *p++ = 0xd8;
  static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  p += put_segment(p, 0xe0, jfif, sizeof(jfif));
  for (int t = 0; t < 2; t++) {
    uint8_t body[65];
    body[0] = (uint8_t)t;
    for (int k = 0; k < 64; k++) body[1 + k] = (uint8_t)mjpg_quant_entry(kJpgQBase[t][kZigzag[k]], quality);
    p += put_segment(p, 0xdb, body, sizeof(body));
  }
  const uint8_t sof[15] = {8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, 3,
                           1, (uint8_t)((g.hs << 4) | g.vs), 0, 2, 0x11, 1, 3, 0x11, 1};
  p += put_segment(p, 0xc0, sof, sizeof(sof));
  const struct {
    uint8_t id;
    const uint8_t* bits;
    const uint8_t* vals;
    int n;
  } dht[4] = {{0x00, kStdDcLumBits, kStdDcVals, 12}, {0x10, kStdAcLumBits, kStdAcLumVals, 162},
              {0x01, kStdDcChrBits, kStdDcVals, 12}, {0x11, kStdAcChrBits, kStdAcChrVals, 162}};
  for (const auto& t : dht) {
    uint8_t body[17 + 162];
    body[0] = t.id;
    memcpy(body + 1, t.bits, 16);
    memcpy(body + 17, t.vals, (size_t)t.n);
    p += put_segment(p, 0xc4, body, 17 + (size_t)t.n);
  }
  const uint8_t dri[2] = {(uint8_t)(g.mcux >> 8), (uint8_t)g.mcux};
  p += put_segment(p, 0xdd, dri, sizeof(dri));
  static const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  p += put_segment(p, 0xda, sos, sizeof(sos));
  return (size_t)(p - dst);
}

size_t jpg_max_bytes(int w, int h, int sampling) {
  JpgGeom g;
  if (!jpg_geom(w, h, sampling, &g)) return 0;
  // per MCU row: its blocks at their worst, doubled by stuffing, and RSTm or EOI
  return kJpgHeaderMax + (size_t)g.mcuy * (2 * (size_t)g.mcux * g.bpm * kJpgBlockBytes + 2);
}

}  // namespace at

extern "C" size_t at_jpeg_max_bytes(int width, int height, int sampling) {
  return at::jpg_max_bytes(width, height, sampling);
}

extern "C" int at_jpeg_encode_host(const uint8_t* bgr, int w, int h, int quality, int sampling, uint8_t* out,
                                   size_t cap, size_t* len) {
  using namespace at;
  if (len) *len = 0;
  JpgGeom g;
  if (!bgr || !out || !len || quality < 1 || quality > 100 || !jpg_geom(w, h, sampling, &g)) return kMjpgInvalid;
  uint16_t q[2][64];
  for (int t = 0; t < 2; t++)
    for (int k = 0; k < 64; k++) q[t][k] = (uint16_t)mjpg_quant_entry(kJpgQBase[t][k], quality);
  uint32_t tab[kJpgTabWords];
  jpg_huff_tables(tab);
  const uint32_t* dc[2] = {tab, tab + kJpgDcTab};
  const uint32_t* ac[2] = {tab + 2 * kJpgDcTab, tab + 2 * kJpgDcTab + kJpgAcTab};
  std::vector<uint8_t> s(kJpgHeaderMax);
  s.resize(jpg_write_header(s.data(), w, h, quality, sampling));
  BitWriter bw{&s};
  int16_t zz[64];
  for (int my = 0; my < g.mcuy; my++) {
    int pred[3] = {0, 0, 0};
    for (int mx = 0; mx < g.mcux; mx++) {
      int last_dc = 0;  // quantised DC of the luma block before, inside this MCU
      for (int k = 0; k < g.hs * g.vs; k++) {
        const int bx = mx * g.hs + k % g.hs, by = my * g.vs + k / g.hs;
        if (bx < g.bw && by < g.bh) {
          jpg_block(bgr, w, g, 0, bx, by, q[0], zz);
        } else {  // a dummy block beyond the picture
          memset(zz, 0, sizeof(zz));
          zz[0] = (int16_t)last_dc;
        }
        jpg_code_block(bw, zz, pred[0], dc[0], ac[0]);
        pred[0] = last_dc = zz[0];
      }
      for (int c = 1; c < 3; c++) {
        jpg_block(bgr, w, g, c, mx, my, q[1], zz);
        jpg_code_block(bw, zz, pred[c], dc[1], ac[1]);
        pred[c] = zz[0];
      }
    }
    bw.flush();
    s.push_back(0xff);
    s.push_back(my + 1 < g.mcuy ? (uint8_t)(0xd0 + (my & 7)) : (uint8_t)0xd9);
  }
  *len = s.size();
  if (s.size() > cap) return -3;  // AT_E_CAPACITY: *len is what the stream needs
  memcpy(out, s.data(), s.size());
  return kMjpgOk;
}
