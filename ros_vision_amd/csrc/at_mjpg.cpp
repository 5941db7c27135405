// at_mjpg.cpp -- marker parser and Huffman decoder of the MJPG input path
// (at_mjpg.h).  Every read of the input is checked against its length; the decode
// loops are bounded by the picture's block count, so no input can make them spin.
#include "at_mjpg.h"

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

}  // namespace

uint32_t MjpgDecoder::decode_index(int bx, int by) const {
  // decode order of luma block (bx, by): MCU by MCU, hs x vs blocks in each
  const int hs = info_.hs, vs = info_.vs;
  const int mcux = gw_ / hs;
  const int mx = bx / hs, my = by / vs;
  return (uint32_t)(((my * mcux + mx) * vs + by % vs) * hs + bx % hs);
}

int MjpgDecoder::decode(const uint8_t* jpg, size_t len, int want_w, int want_h) {
  info_ = MjpgInfo{};
  bw_ = bh_ = gw_ = gh_ = 0;
  kept_tokens_ = 0;
  if (!jpg || len < 4 || jpg[0] != 0xff || jpg[1] != 0xd8) return kMjpgInvalid;
  uint8_t qt[4][64];
  bool qt_def[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  Comp comp[3] = {};
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
      info_.width = w;
      info_.height = h;
      info_.ncomp = nf;
      info_.hs = comp[0].h;
      info_.vs = comp[0].v;
      have_sof = true;
      if ((want_w > 0 && w != want_w) || (want_h > 0 && h != want_h)) return kMjpgInvalid;
      if ((size_t)w * (size_t)h > kMjpgMaxPixels) return kMjpgInvalid;
      if (want_w < 0) return kMjpgOk;  // header only
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
      info_.restart = (int)be16(s);
    } else if (m == 0xda) {  // SOS
      if (!have_sof || n < 1) return kMjpgInvalid;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != (size_t)(4 + 2 * ns)) return kMjpgInvalid;
      if (ns != info_.ncomp) return kMjpgUnsupported;  // one scan holds every component
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
  for (int i = 0; i < info_.ncomp; i++) {
    Huff& hd = dc[comp[i].td];
    Huff& ha = ac[comp[i].ta];
    if (!hd.defined) {
      if (comp[i].td > 1) return kMjpgInvalid;
      huff_build(&hd, comp[i].td ? kStdDcChrBits : kStdDcLumBits, kStdDcVals, 12);
      info_.default_dht = 1;
    }
    if (!ha.defined) {
      if (comp[i].ta > 1) return kMjpgInvalid;
      huff_build(&ha, comp[i].ta ? kStdAcChrBits : kStdAcLumBits, comp[i].ta ? kStdAcChrVals : kStdAcLumVals, 162);
      info_.default_dht = 1;
    }
  }
  for (int k = 0; k < 64; k++) q_[kZigzag[k]] = qt[comp[0].tq][k];

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
      const bool keep = ci == 0;
      if (keep) start_.push_back((uint32_t)tok_.size());
      const int t = huff_decode(br, hd);
      if (t < 0 || t > 15) return kMjpgInvalid;
      if (t) pred[ci] += receive_extend(br, t);
      pred[ci] = (int16_t)pred[ci];  // a coefficient is 16 bits (corrupt streams only get here)
      if (keep && pred[0]) tok_.push_back((uint32_t)(uint16_t)pred[0]);
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
        if (keep) tok_.push_back(((uint32_t)k << 16) | (uint32_t)(uint16_t)v);
        k++;
      }
    }
    if (br.overran()) return kMjpgInvalid;  // truncated: stop early
  }
  start_.push_back((uint32_t)tok_.size());
  if (start_.size() != nluma + 1) return kMjpgInvalid;
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

bool MjpgDecoder::dense() const {
  const size_t nb = nblocks();
  return 4 * (nb + 1) + 4 * (size_t)kept_tokens_ >= 128 * nb;
}

size_t MjpgDecoder::packed_bytes() const {
  const size_t nb = nblocks();
  return (size_t)kMjpgHdrBytes + (dense() ? 128 * nb : 4 * (nb + 1) + 4 * (size_t)kept_tokens_);
}

int MjpgDecoder::pack(uint8_t* dst, size_t cap) const {
  const uint32_t nb = nblocks();
  if (!dst || !nb || start_.size() != (size_t)gw_ * gh_ + 1 || cap < packed_bytes()) return kMjpgInvalid;
  const bool dn = dense();
  memset(dst, 0, kMjpgHdrBytes);
  memcpy(dst, q_, sizeof(q_));
  const uint32_t mode = dn ? kMjpgDense : kMjpgSparse, ntok = dn ? 0 : kept_tokens_;
  memcpy(dst + kMjpgModeOff, &mode, 4);
  memcpy(dst + kMjpgNtokOff, &ntok, 4);
  memcpy(dst + kMjpgNblkOff, &nb, 4);
  uint8_t* pay = dst + kMjpgHdrBytes;
  if (dn) {
    memset(pay, 0, (size_t)128 * nb);
    int16_t* out = reinterpret_cast<int16_t*>(pay);
    uint32_t b = 0;
    for (int by = 0; by < bh_; by++)
      for (int bx = 0; bx < bw_; bx++, b++) {
        const uint32_t i = decode_index(bx, by);
        for (uint32_t t = start_[i]; t < start_[i + 1]; t++)
          out[(size_t)b * 64 + kZigzag[(tok_[t] >> 16) & 63]] = (int16_t)(uint16_t)(tok_[t] & 0xffffu);
      }
    return kMjpgOk;
  }
  uint32_t* off = reinterpret_cast<uint32_t*>(pay);
  uint32_t* tk = off + nb + 1;
  uint32_t o = 0, b = 0;
  for (int by = 0; by < bh_; by++)
    for (int bx = 0; bx < bw_; bx++, b++) {
      const uint32_t i = decode_index(bx, by);
      const uint32_t n = start_[i + 1] - start_[i];
      off[b] = o;
      if (n) memcpy(tk + o, tok_.data() + start_[i], (size_t)n * 4);
      o += n;
    }
  off[nb] = o;
  return kMjpgOk;
}

int MjpgDecoder::to_gray(uint8_t* gray, size_t cap) const {
  const int W = info_.width, H = info_.height;
  if (!gray || !nblocks() || start_.size() != (size_t)gw_ * gh_ + 1 || cap < (size_t)W * H) return kMjpgInvalid;
  for (int by = 0; by < bh_; by++)
    for (int bx = 0; bx < bw_; bx++) {
      int32_t ws[64] = {0};
      const uint32_t i = decode_index(bx, by);
      for (uint32_t t = start_[i]; t < start_[i + 1]; t++) {
        const int nat = kZigzag[(tok_[t] >> 16) & 63];
        ws[nat] = (int32_t)(int16_t)(uint16_t)(tok_[t] & 0xffffu) * (int32_t)q_[nat];
      }
      for (int c = 0; c < 8; c++) {
        int32_t v[8];
        for (int r = 0; r < 8; r++) v[r] = ws[r * 8 + c];
        mjpg_idct_1d<11>(v);
        for (int r = 0; r < 8; r++) ws[r * 8 + c] = v[r];
      }
      for (int r = 0; r < 8; r++) {
        const int y = by * 8 + r;
        if (y >= H) break;
        int32_t v[8];
        for (int c = 0; c < 8; c++) v[c] = ws[r * 8 + c];
        mjpg_idct_1d<18>(v);
        for (int c = 0; c < 8 && bx * 8 + c < W; c++) gray[(size_t)y * W + bx * 8 + c] = (uint8_t)mjpg_pixel(v[c]);
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

extern "C" int at_mjpg_stream_mode_host(const uint8_t* jpg, size_t len, int want_w, int want_h,
                                        size_t* stream_bytes) {
  at::MjpgDecoder dec;
  const int rc = dec.decode(jpg, len, want_w > 0 ? want_w : 0, want_h > 0 ? want_h : 0);
  if (rc != at::kMjpgOk) return rc;
  if (stream_bytes) *stream_bytes = dec.packed_bytes();
  return dec.dense() ? 1 : 0;
}
