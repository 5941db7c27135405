// at_mjpg_entropy.h -- the entropy decode of the MJPG input path as a parallel
// algorithm: the arithmetic k_mjpg_entropy (at_kernels.hip) and its CPU reference
// at_mjpg_entropy_host (at_mjpg.cpp) both compile.  Plain C++17, no HIP include.
//
// A baseline scan is one Huffman bit stream.  It is cut into pieces of S bytes; each
// piece is decoded by its own thread from an entry state, and the threads exchange
// states until nothing changes (Weissenberger & Schmidt, ICPP 2018: a decoder started
// at a wrong bit falls into step with the true one after a few codewords).
//
// State of a decoder at a point of the scan:
//   pos, bit   the next unread bit: byte `pos` of the scan (never the 00 stuffed behind
//              an FF), `bit` bits of it already used
//   zz         0: a block's DC symbol comes next; 1..63: the AC symbol for zig-zag
//              index zz comes next
//   blk        block index within the MCU (selects the component and its tables)
//   n          MCUs finished since the last restart marker (0 without restarts)
//   end        the data is used up (pos == scan length)
// A step decodes one symbol with its magnitude bits, or moves over a marker.  A piece
// owns the steps that start inside it, so a symbol that straddles a boundary belongs to
// the piece it starts in, and a piece whose entry state lies beyond its end owns none.
//
// Markers, as MjpgDecoder treats them.  After `restart` MCUs the rest of the interval is
// dropped up to the next marker (FF fill bytes in front of it included) and the state
// becomes (byte after the marker, 0, 0, 0).  Bits needed from beyond a marker or the end
// of the data are an error for the true decoder; a speculative one takes the marker as a
// synchronisation point all the same.  So does it continue (bounded, by a fixed rule)
// after a code no table has or a run past coefficient 63: every step uses at least one
// bit or passes a marker, which bounds a piece's loop by 8 * length + 8 steps.
//
// The true entry states are a fixed point of "entry of piece i = exit of piece i - 1",
// and piece 0's entry is known, so after round r the first r + 1 pieces are final: the
// exchange ends within `pieces` rounds whatever the stream, and what it ends in is the
// serial decode.  Errors are only looked at in the last pass, which runs from the true
// states: a code no table has, a run past 63, bits from beyond the data, a wrong or
// missing RSTn, too few blocks.
#ifndef AT_MJPG_ENTROPY_H_
#define AT_MJPG_ENTROPY_H_

#include "at_mjpg.h"

namespace at {

constexpr int kEntLookBits = 9;
constexpr int kEntMaxTabs = 6;            // DC + AC of up to three components
constexpr uint32_t kEntNoLimit = 0xffffffffu;
constexpr int kEntSubseqMin = 4, kEntSubseqMax = 4096, kEntSubseqDefault = 128;

// One decode table (Huff of at_mjpg.cpp, laid out for the device): 1424 bytes.
struct EntTab {
  uint16_t look[1 << kEntLookBits];  // (length << 8) | symbol for codes of <= 9 bits, 0 otherwise
  int32_t maxcode[18];               // largest code of each length, -1 if none; [17] unused
  int32_t valoff[17];                // vals index of the first code of each length, minus that code
  uint8_t vals[256];
  uint8_t pad[4];
};
static_assert(sizeof(EntTab) == 1424, "EntTab is part of the table block");

// Geometry of one frame's scan: the head of its table block (64 bytes).
struct EntGeom {
  uint32_t scan_len;     // bytes of scan data (stuffing and markers in)
  uint32_t ncomp;        // 1 or 3
  uint32_t hs, vs;       // luma sampling factors
  uint32_t mcux, mcuy;   // MCU grid
  uint32_t restart;      // restart interval in MCUs (0: none)
  uint32_t bw, bh;       // visible luma block grid
  uint32_t keep_chroma;  // write the Cb / Cr coefficients too
  uint32_t ntab;         // tables that follow
  uint32_t tabsel;       // 4 bits each: table of (comp 0 DC, AC, comp 1 DC, AC, comp 2 DC, AC)
  uint32_t cb_off, cr_off;  // byte offsets of the chroma sub-streams in the coefficient slot (0: none)
  uint32_t subseq;       // piece size S in bytes
  uint32_t reserved;     // 0 (a frame the host decoded has no record: its directory entry is 0)
};
static_assert(sizeof(EntGeom) == 64, "EntGeom is part of the table block");

// One frame's record on the link: geometry, the 256-byte stream headers (luma, Cb, Cr;
// mode = dense), `ntab` tables, then the scan bytes.
constexpr size_t kEntHdrsOff = sizeof(EntGeom);
constexpr size_t kEntTabsOff = kEntHdrsOff + 3 * (size_t)kMjpgHdrBytes;
AT_MJPG_HD size_t ent_scan_off(uint32_t ntab) { return kEntTabsOff + (size_t)ntab * sizeof(EntTab); }
constexpr size_t kEntRecordMax = kEntTabsOff + kEntMaxTabs * sizeof(EntTab);  // without the scan bytes

AT_MJPG_HD uint32_t ent_bpm(const EntGeom& g) { return g.hs * g.vs + (g.ncomp == 3 ? 2u : 0u); }
AT_MJPG_HD uint32_t ent_total_blocks(const EntGeom& g) { return g.mcux * g.mcuy * ent_bpm(g); }
AT_MJPG_HD uint32_t ent_pieces(const EntGeom& g) {
  const uint32_t n = (g.scan_len + g.subseq - 1) / g.subseq;
  return n ? n : 1u;
}
// Blocks the most a w x h picture (multiples of 8) decodes, over every sampling: the size of
// the DC scratch.
AT_MJPG_HD size_t ent_max_blocks(int w, int h) { return 3 * (size_t)(w / 8 + 1) * (size_t)(h / 8 + 1); }

struct EntState {
  uint32_t pos;
  uint32_t n;
  uint8_t bit, zz, blk, end;
};
AT_MJPG_HD uint64_t ent_pack(const EntState& s) {
  return (uint64_t)s.pos | ((uint64_t)s.bit << 32) | ((uint64_t)s.zz << 35) | ((uint64_t)s.blk << 41) |
         ((uint64_t)(s.n & 0xffffu) << 44) | ((uint64_t)s.end << 60);
}
AT_MJPG_HD EntState ent_unpack(uint64_t v) {
  EntState s;
  s.pos = (uint32_t)v;
  s.bit = (uint8_t)((v >> 32) & 7);
  s.zz = (uint8_t)((v >> 35) & 63);
  s.blk = (uint8_t)((v >> 41) & 7);
  s.n = (uint32_t)((v >> 44) & 0xffffu);
  s.end = (uint8_t)((v >> 60) & 1);
  return s;
}
AT_MJPG_HD EntState ent_end_state(uint32_t len) {
  EntState s;
  s.pos = len;
  s.n = 0;
  s.bit = s.zz = s.blk = 0;
  s.end = 1;
  return s;
}

// What a decoder needs of one frame.
struct EntCtx {
  const uint8_t* scan;
  uint32_t len;
  const EntTab* tab;  // ntab tables
  EntGeom g;
  uint32_t bpm, nluma;  // blocks per MCU, luma blocks of it
};
AT_MJPG_HD EntCtx ent_ctx(const EntGeom& g, const EntTab* tab, const uint8_t* scan) {
  EntCtx c;
  c.scan = scan;
  c.len = g.scan_len;
  c.tab = tab;
  c.g = g;
  c.bpm = ent_bpm(g);
  c.nluma = g.hs * g.vs;
  return c;
}
// The geometry is the host's, but a kernel trusts nothing it indexes with.
AT_MJPG_HD bool ent_geom_ok(const EntGeom& g) {
  if (g.ncomp != 1 && g.ncomp != 3) return false;
  if (!((g.hs == 1 && g.vs == 1) || (g.hs == 2 && g.vs == 1) || (g.hs == 2 && g.vs == 2))) return false;
  if (g.ncomp == 1 && g.hs * g.vs != 1) return false;
  if (!g.mcux || !g.mcuy || g.mcux > 8192 || g.mcuy > 8192 || !g.bw || !g.bh) return false;
  if (g.bw > g.mcux * g.hs || g.bh > g.mcuy * g.vs) return false;
  if (g.ntab < 2 || g.ntab > (uint32_t)kEntMaxTabs || g.restart > 0xffffu) return false;
  if (g.subseq < (uint32_t)kEntSubseqMin || g.subseq > (uint32_t)kEntSubseqMax) return false;
  for (int i = 0; i < 6; i++)
    if (((g.tabsel >> (4 * i)) & 15u) >= g.ntab) return false;
  return true;
}

// ---- bit reader over stuffed bytes ---------------------------------------------------
// Up to four data bytes from byte `pos` on, first byte in the top bits: a byte other than
// FF, or FF 00 as FF.  Stops in front of anything else (a marker, a lone FF, the end of the
// scan) and gives zeros from there.  *nreal: the data bytes found; *wide: bit i set when
// byte i took two scan bytes.  Every read is inside [0, len).
AT_MJPG_HD uint32_t ent_peek(const uint8_t* sc, uint32_t len, uint32_t pos, int* nreal, uint32_t* wide) {
  uint32_t acc = 0, w = 0, p = pos;
  int n = 0;
  bool stop = false;
  for (int i = 0; i < 4; i++) {
    uint32_t b = 0;
    if (!stop) {
      if (p < len) {
        const uint32_t b0 = sc[p];
        if (b0 != 0xffu) {
          b = b0;
          p++;
          n++;
        } else if (p + 1 < len && sc[p + 1] == 0) {
          b = 0xffu;
          p += 2;
          w |= 1u << i;
          n++;
        } else {
          stop = true;
        }
      } else {
        stop = true;
      }
    }
    acc = (acc << 8) | b;
  }
  *nreal = n;
  *wide = w;
  return acc;
}
// (pos, bit) moved on by `bits` <= 32 - bit, all of them inside the data bytes ent_peek found
AT_MJPG_HD void ent_advance(uint32_t* pos, uint32_t* bit, uint32_t wide, int bits) {
  uint32_t t = *bit + (uint32_t)bits, p = *pos;
  for (int i = 0; i < 4 && t >= 8; i++, t -= 8) p += 1u + ((wide >> i) & 1u);
  *pos = p;
  *bit = t;
}
// The first marker at or after byte `from`: FF followed by neither 00 nor FF.  Returns the
// position of its FF, or len if there is none.
AT_MJPG_HD uint32_t ent_find_marker(const uint8_t* sc, uint32_t len, uint32_t from) {
  uint32_t p = from;
  while (p + 1 < len && !(sc[p] == 0xffu && sc[p + 1] != 0 && sc[p + 1] != 0xffu)) p++;
  return p + 1 < len ? p : len;
}

// ---- table lookup -----------------------------------------------------------------------
// The symbol coded by the top bits of `top16`; *l its length, 0 if no code of up to 16
// bits matches.
AT_MJPG_HD int ent_lookup(const EntTab& h, uint32_t top16, int* l) {
  const uint16_t e = h.look[top16 >> (16 - kEntLookBits)];
  if (e) {
    *l = e >> 8;
    return e & 0xff;
  }
  for (int k = kEntLookBits + 1; k <= 16; k++) {
    const int32_t code = (int32_t)(top16 >> (16 - k));
    if (code <= h.maxcode[k]) {
      *l = k;
      return h.vals[(code + h.valoff[k]) & 0xff];
    }
  }
  *l = 0;
  return 0;
}

// T.81 F.2.2.1 EXTEND of the s-bit value v, 1 <= s <= 15
AT_MJPG_HD int ent_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// ---- the per-piece step function -----------------------------------------------------
enum { kEntErrCode = 1, kEntErrRun = 2, kEntErrData = 4, kEntErrRestart = 8, kEntErrBlocks = 16 };

// Decodes from state s the steps that start in front of byte `end` (kEntNoLimit: all that are
// left) and returns the state it ends in.  The sink sees what is decoded:
//   bool full()            no further block may begin (the picture is complete)
//   void begin()           a block begins
//   void dc(int diff), void ac(int k, int v)
//   void restart(int m)    an interval ended at marker FF m (m < 0: no marker left)
//   void error(int what)   returns nothing; the decode goes on by its fixed rule
//   bool stop()            give up (asked after every step)
template <class Sink>
AT_MJPG_HD EntState ent_decode_piece(const EntCtx& c, EntState s, uint32_t end, Sink& sink) {
  const uint8_t* sc = c.scan;
  const uint32_t len = c.len;
  const uint32_t most = 8u * len + 8u;  // every step uses a bit or passes a marker
  for (uint32_t it = 0; it < most && !s.end && s.pos < end && !sink.stop(); it++) {
    if (s.zz == 0 && sink.full()) break;
    if (s.zz == 0 && s.blk == 0 && c.g.restart && s.n == c.g.restart) {
      // the interval is complete: drop its padding, find the marker
      uint32_t from = s.pos;
      if (s.bit) from += (sc[s.pos] == 0xffu) ? 2u : 1u;
      const uint32_t m = ent_find_marker(sc, len, from);
      if (m >= len) {
        sink.restart(-1);
        s = ent_end_state(len);
      } else {
        sink.restart((int)sc[m + 1]);
        s.pos = m + 2;
        s.bit = s.zz = s.blk = 0;
        s.n = 0;
      }
      continue;
    }
    const uint32_t comp = s.blk < c.nluma ? 0u : s.blk - c.nluma + 1u;
    const bool is_dc = s.zz == 0;
    if (is_dc) sink.begin();
    const EntTab& h = c.tab[(c.g.tabsel >> (4 * (2 * comp + (is_dc ? 0u : 1u)))) & 15u];
    int nreal;
    uint32_t wide;
    uint32_t pos = s.pos, bit = s.bit;
    uint32_t w = ent_peek(sc, len, pos, &nreal, &wide) << bit;
    int avail = 8 * nreal - (int)bit;  // data bits in w, at the top
    int l;
    int sym = ent_lookup(h, w >> 16, &l);
    bool ran_out = false;
    int sz = 0;
    if (l == 0) {
      if (avail >= 16) {
        sink.error(kEntErrCode);
        l = 1;  // the fixed rule: one bit on, same place in the block
        ent_advance(&pos, &bit, wide, l);
        s.pos = pos;
        s.bit = (uint8_t)bit;
        continue;
      }
      ran_out = true;
    } else if (l > avail) {
      ran_out = true;
    } else {
      if (is_dc && sym > 15) {
        sink.error(kEntErrCode);
        sym &= 15;
      }
      sz = sym & 15;
    }
    int v = 0;
    if (!ran_out && sz) {
      if (l + sz > avail) {
        // the magnitude bits may lie beyond the four bytes: look again from behind the code
        ent_advance(&pos, &bit, wide, l);
        w = ent_peek(sc, len, pos, &nreal, &wide) << bit;
        avail = 8 * nreal - (int)bit;
        l = 0;
        if (sz > avail) ran_out = true;
      }
      if (!ran_out) v = ent_extend((int)((w << l) >> (32 - sz)), sz);
    }
    if (ran_out) {
      // bits from beyond the data: the marker (if one is there) synchronises
      sink.error(kEntErrData);
      uint32_t stop_at = pos;
      for (int i = 0; i < nreal; i++) stop_at += 1u + ((wide >> i) & 1u);
      const uint32_t m = ent_find_marker(sc, len, stop_at);
      if (m >= len) {
        s = ent_end_state(len);
      } else {
        s.pos = m + 2;
        s.bit = s.zz = s.blk = 0;
        s.n = 0;
      }
      continue;
    }
    ent_advance(&pos, &bit, wide, l + sz);
    s.pos = pos;
    s.bit = (uint8_t)bit;
    bool block_done = false;
    if (is_dc) {
      sink.dc(v);
      s.zz = 1;
    } else {
      const int r = sym >> 4;
      if (!sz) {
        if (r != 15) {
          block_done = true;  // EOB
        } else {
          const int k = s.zz + 16;
          if (k >= 64) block_done = true; else s.zz = (uint8_t)k;
        }
      } else {
        const int k = s.zz + r;
        if (k > 63) {
          sink.error(kEntErrRun);
          block_done = true;
        } else {
          sink.ac(k, v);
          if (k == 63) block_done = true; else s.zz = (uint8_t)(k + 1);
        }
      }
    }
    if (block_done) {
      s.zz = 0;
      s.blk++;
      if (s.blk >= c.bpm) {
        s.blk = 0;
        s.n = c.g.restart ? s.n + 1 : 0;
      }
    }
  }
  return s;
}

// Entry state guessed for piece i > 0 in round 0: its first whole byte, the start of an MCU.
// (Not a stuffed 00 and not a marker's second byte, where that can be told.)
AT_MJPG_HD EntState ent_guess(const EntCtx& c, uint32_t i) {
  EntState s;
  s.pos = i * c.g.subseq;
  s.n = 0;
  s.bit = s.zz = s.blk = s.end = 0;
  if (i && s.pos < c.len && c.scan[s.pos - 1] == 0xffu && c.scan[s.pos] != 0xffu) s.pos++;
  if (s.pos >= c.len) s = ent_end_state(c.len);
  return s;
}
// where piece i ends (the last piece takes whatever is left)
AT_MJPG_HD uint32_t ent_piece_end(const EntCtx& c, uint32_t i, uint32_t npieces) {
  return i + 1 >= npieces ? kEntNoLimit : (i + 1) * c.g.subseq;
}

// The sink of the synchronisation rounds: counts the blocks begun.
struct EntCount {
  uint32_t blocks = 0;
  AT_MJPG_HD bool full() const { return false; }
  AT_MJPG_HD bool stop() const { return false; }
  AT_MJPG_HD void begin() { blocks++; }
  AT_MJPG_HD void dc(int) {}
  AT_MJPG_HD void ac(int, int) {}
  AT_MJPG_HD void restart(int) {}
  AT_MJPG_HD void error(int) {}
};

// Where the coefficients go: the dense payloads of at_mjpg.h and the DC differences of
// every decoded block in decode order (the padding blocks' too: the prediction runs
// through them).
struct EntOut {
  int16_t* luma;     // [bw * bh][64]
  int16_t* chroma[2];  // [mcux * mcuy][64] each, or null
  int16_t* dcdiff;   // [total blocks]
};
// payload of block `a` (decode order), or null if it is dropped
AT_MJPG_HD int16_t* ent_block_ptr(const EntCtx& c, const EntOut& o, uint32_t a) {
  const uint32_t m = a / c.bpm, b = a - m * c.bpm;
  if (b < c.nluma) {
    const uint32_t my = m / c.g.mcux, mx = m - my * c.g.mcux;
    const uint32_t bx = mx * c.g.hs + b % c.g.hs, by = my * c.g.vs + b / c.g.hs;
    if (bx >= c.g.bw || by >= c.g.bh) return nullptr;
    return o.luma + ((size_t)by * c.g.bw + bx) * 64;
  }
  int16_t* p = b == c.nluma ? o.chroma[0] : o.chroma[1];  // (selected, not indexed: the struct stays in registers)
  return p ? p + (size_t)m * 64 : nullptr;
}

// The sink of the last pass, which runs from the true entry states.
struct EntWrite {
  const EntCtx* c;
  EntOut o;
  int64_t cur;        // the block being decoded (decode order); first - 1 on entry
  uint32_t total;
  int16_t* dst;       // its payload, or null
  int err = 0;
  AT_MJPG_HD EntWrite(const EntCtx* ctx, const EntOut& out, uint32_t first, bool mid_block)
      : c(ctx), o(out), cur((int64_t)first - 1), total(ent_total_blocks(ctx->g)), dst(nullptr) {
    if (mid_block && cur >= 0 && cur < (int64_t)total) dst = ent_block_ptr(*c, o, (uint32_t)cur);
  }
  AT_MJPG_HD bool full() const { return cur + 1 >= (int64_t)total; }
  // (what follows the picture's last block is not the picture's: nothing of it is looked at)
  AT_MJPG_HD bool stop() const { return err != 0 || cur >= (int64_t)total; }
  AT_MJPG_HD void begin() {
    cur++;
    dst = ent_block_ptr(*c, o, (uint32_t)cur);
  }
  AT_MJPG_HD void dc(int diff) {
    if (cur >= 0 && cur < (int64_t)total) o.dcdiff[cur] = (int16_t)diff;
  }
  AT_MJPG_HD void ac(int k, int v) {
    static constexpr uint8_t zz[64] = AT_MJPG_ZIGZAG;
    if (dst) dst[zz[k & 63]] = (int16_t)v;
  }
  AT_MJPG_HD void restart(int m) {
    // an interval ends on a whole number of MCUs, and its marker counts modulo 8
    const uint32_t next = (uint32_t)(cur + 1);
    const uint32_t mcu = next / c->bpm;
    if (m < 0 || next % c->bpm || !mcu || mcu % c->g.restart ||
        m != (int)(0xd0u + ((mcu / c->g.restart - 1u) & 7u)))
      err |= kEntErrRestart;
  }
  AT_MJPG_HD void error(int what) { err |= what; }
};

// ---- DC prediction: a segmented prefix sum in 16-bit modular arithmetic -----------------
// MjpgDecoder keeps each component's predictor as int16 after every block, so the DC of a
// block is the sum modulo 2^16 of the differences since the last restart.  The segments are
// static: a new one starts at every MCU whose index is a multiple of `restart`.
struct EntDcSum {
  uint16_t s[3];
  uint16_t reset;  // a segment starts inside the range (the sums count from the last start)
};
AT_MJPG_HD EntDcSum ent_dc_join(const EntDcSum& a, const EntDcSum& b) {  // a in front of b
  EntDcSum r;
  for (int k = 0; k < 3; k++) r.s[k] = (uint16_t)(b.reset ? b.s[k] : a.s[k] + b.s[k]);
  r.reset = a.reset | b.reset;
  return r;
}
// MCUs [m0, m1): their sums; with `apply`, starting from `carry` (the join of everything in
// front), the DC values into coefficient 0 of every block kept.
AT_MJPG_HD EntDcSum ent_dc_range(const EntCtx& c, const EntOut& o, uint32_t m0, uint32_t m1, bool apply,
                                 const EntDcSum& carry) {
  EntDcSum r;
  r.reset = 0;
  for (int k = 0; k < 3; k++) r.s[k] = apply ? carry.s[k] : 0;
  for (uint32_t m = m0; m < m1; m++) {
    if (c.g.restart && m % c.g.restart == 0) {
      r.s[0] = r.s[1] = r.s[2] = 0;
      r.reset = 1;
    }
    for (uint32_t b = 0; b < c.bpm; b++) {
      const uint32_t comp = b < c.nluma ? 0u : b - c.nluma + 1u;
      const uint32_t a = m * c.bpm + b;
      const uint16_t v = (uint16_t)((comp == 0 ? r.s[0] : (comp == 1 ? r.s[1] : r.s[2])) + (uint16_t)o.dcdiff[a]);
      if (comp == 0) r.s[0] = v; else if (comp == 1) r.s[1] = v; else r.s[2] = v;
      if (apply) {
        int16_t* p = ent_block_ptr(c, o, a);
        if (p) p[0] = (int16_t)v;
      }
    }
  }
  return r;
}

// Where the dense streams of a frame lie in its coefficient slot: luma at 0, Cb and Cr at
// multiples of kMjpgSubAlign behind it (0: none), `total` bytes in all.
struct EntLayout {
  uint32_t nb, cnb;          // luma (visible) and chroma blocks
  uint32_t cb_off, cr_off;
  size_t total;
};
AT_MJPG_HD EntLayout ent_layout(const EntGeom& g) {
  const size_t al = (size_t)kMjpgSubAlign - 1;
  EntLayout L;
  L.nb = g.bw * g.bh;
  L.cnb = g.ncomp == 3 && g.keep_chroma ? g.mcux * g.mcuy : 0;
  const size_t luma = (size_t)kMjpgHdrBytes + 128 * (size_t)L.nb;
  L.cb_off = L.cr_off = 0;
  L.total = luma;
  if (L.cnb) {
    const size_t sub = (size_t)kMjpgHdrBytes + 128 * (size_t)L.cnb;
    L.cb_off = (uint32_t)((luma + al) & ~al);
    L.cr_off = (uint32_t)((L.cb_off + sub + al) & ~al);
    L.total = L.cr_off + sub;
  }
  return L;
}

// What k_mjpg_entropy works on (at_api.cpp allocates, at_kernels.hip launches).
struct EntBufs {
  const uint8_t* in;     // the batch as it crossed the link: u64 dir[frames] (byte offset of each
                         // frame's record, 0: the frame is not decoded here), then the records
  size_t in_bytes;       // bytes of `in` that are valid
  uint8_t* coef;         // coefficient slots, `slot` bytes apart
  size_t slot;
  uint32_t nb;           // luma blocks of the detector's geometry (what k_mjpg_idct reads)
  uint64_t* entry;       // per frame `pieces` words each: the state a piece was last decoded from,
  uint64_t* exit;        // ... the state it ended in,
  uint32_t* nblk;        // ... the blocks it began (then: its first block)
  uint32_t pieces;
  int16_t* dcdiff;       // per frame `dc_blocks` DC differences in decode order
  uint32_t dc_blocks;
  uint32_t* info;        // per frame kEntInfoWords: error bits, synchronisation rounds (zeroed per batch)
};
constexpr int kEntInfoWords = 4;
constexpr int kEntErrGeom = 32;  // a record the kernel does not trust (never from at_enqueue_mjpg)

// ---- host side (at_mjpg.cpp) ------------------------------------------------------------
// The marker parse of at_enqueue_mjpg with the device decode on: SOI .. SOS, the tables
// (Annex K defaults included), the size and sampling checks -- MjpgDecoder's, with its
// codes -- and nothing decoded.  Writes the frame's record (geometry, headers, tables) to
// `rec` (kEntRecordMax bytes); *scan_pos is where the scan bytes start in jpg.
int mjpg_entropy_parse(const uint8_t* jpg, size_t len, int want_w, int want_h, bool keep_chroma, uint32_t subseq,
                       uint8_t* rec, size_t* scan_pos);

}  // namespace at

// The same subsequence algorithm run sequentially over the threads' pieces: the CPU
// reference of k_mjpg_entropy.  Writes the frame's dense streams (headers and payloads, the
// layout of at_mjpg.h; with keep_chroma the sub-streams too) to out, as many bytes as
// at_mjpg_dense_host reports; *rounds (may be NULL) the synchronisation rounds it took, round
// 0 included.  Returns 0, or the code MjpgDecoder::decode gives for the stream.
extern "C" int at_mjpg_entropy_host(const uint8_t* jpg, size_t len, int want_w, int want_h, int subseq_bytes,
                                    int keep_chroma, uint8_t* out, size_t cap, int* rounds);
// What MjpgDecoder decodes, every plane in the dense encoding: the same layout, for comparison.
extern "C" int at_mjpg_dense_host(const uint8_t* jpg, size_t len, int want_w, int want_h, int keep_chroma,
                                  uint8_t* out, size_t cap, size_t* out_bytes);

#endif  // AT_MJPG_ENTROPY_H_
