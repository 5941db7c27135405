// at_mjpg.h -- host JPEG front end of the MJPG input path.
//
// Baseline sequential 8-bit Huffman JPEG (SOF0), the format UVC cameras emit as
// MJPG.  The serial part of the decode runs on the host: marker parsing, Huffman
// decode of every component (an interleaved scan cannot skip the chroma bits), DC
// prediction and restart handling.  Only the luma coefficients are kept (AprilTag
// detection reads luma); they go to the GPU still quantised, where k_mjpg_idct
// (at_kernels.hip) dequantises, runs the inverse DCT and writes the GRAY8 plane.
// With colour on (decode(..., keep_chroma), at_mjpg_set_color) the Cb and Cr
// coefficients are kept too and travel as two more sub-streams behind the luma
// one; k_mjpg_idct_chroma and k_mjpg_bgr then produce the BGR8 image.
//
// With at_mjpg_set_device_entropy the host stops after the marker parse and the Huffman
// decode runs on the GPU as well (at_mjpg_entropy.h, k_mjpg_entropy), which leaves the
// dense layout below in the frame's slot.
//
// Plain C++17, no HIP include: compiles alone with the host compiler (the
// sanitized stand-alone check tests/mjpg_host_check.cpp builds it that way).
//
// Coefficient stream of one frame (what the host writes and the kernel reads):
//   header, kMjpgHdrBytes:
//     u16 q[64]     luma quantisation table, natural (row-major) order
//     u32 mode      kMjpgSparse / kMjpgDense
//     u32 ntokens   sparse: number of tokens
//     u32 nblocks   (W/8) * (H/8)
//   payload, sparse:  u32 off[nblocks + 1], then u32 token[ntokens]; block b owns
//                     token[off[b] .. off[b+1]); a token is (zig-zag position << 16) |
//                     (u16)(i16 quantised value); only non-zero coefficients appear
//   payload, dense:   i16 coef[nblocks][64], natural order
// Blocks are in raster order of the W/8 x H/8 grid: the blocks an MCU grid pads
// beyond the picture (4:2:0 at 1080 rows: 1088) are decoded for their DC
// prediction and dropped here, so the stream holds exactly the visible blocks.
// Dense is chosen whenever sparse would not be smaller, so the payload never
// exceeds 128 B per block (2 B per pixel) and no frame can fail for size.
//
// Colour on: the luma header also carries
//     u32 cb_off, cr_off   byte offsets of the Cb / Cr sub-streams from the start of the
//                          frame's stream (multiples of 16; 0: a single-component frame)
//     u32 sampling         hs | vs << 8 | ncomp << 16
// and each chroma sub-stream is a header of the same kMjpgHdrBytes (the component's own
// q[64], mode, ntokens, nblocks, then u32 bw: the plane's width in blocks, u32 hs, u32 vs)
// followed by a sparse or dense payload chosen by the same rule.  A chroma plane is
// cw = ceil(W / hs) by ch = ceil(H / vs) samples on a grid of ceil(cw / 8) x ceil(ch / 8)
// blocks, which is the MCU grid: chroma has no padding blocks to drop.  With colour off
// those header bytes are zero and nothing follows the luma payload, as before.
#ifndef AT_MJPG_H_
#define AT_MJPG_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIP__)  // compiled as HIP: the kernel calls the IDCT pass too
#define AT_MJPG_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define AT_MJPG_HD inline
#endif

namespace at {

constexpr int kMjpgHdrBytes = 256;
constexpr uint32_t kMjpgSparse = 0, kMjpgDense = 1;
constexpr int kMjpgModeOff = 128, kMjpgNtokOff = 132, kMjpgNblkOff = 136;
// colour on, luma header: the sub-streams' offsets and the sampling word
constexpr int kMjpgCbOff = 140, kMjpgCrOff = 144, kMjpgSampOff = 148;
// chroma sub-stream header: plane width in blocks, the frame's sampling factors
constexpr int kMjpgBwOff = 140, kMjpgHsOff = 144, kMjpgVsOff = 148;
constexpr int kMjpgSubAlign = 16;  // a dense payload is read in 16-byte words

// error codes of include/at_api.h (this header stands alone)
constexpr int kMjpgOk = 0, kMjpgInvalid = -1, kMjpgUnsupported = -6;

// zig-zag position -> natural index (ITU-T T.81 figure 5)
#define AT_MJPG_ZIGZAG                                                                            \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,       \
   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,       \
   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// One 1-D pass of libjpeg's integer "slow" inverse DCT (jidctint: 13-bit constants,
// 2 pass bits), on 8 values in place.  SHIFT is the descale: 11 for the column
// pass (CONST_BITS - PASS1_BITS), 18 for the row pass (CONST_BITS + PASS1_BITS + 3).
// Integers only; the sums wrap in uint32_t, which is the same bit pattern as int32
// arithmetic on every valid stream and defined behaviour on a corrupt one.
template <int SHIFT>
AT_MJPG_HD void mjpg_idct_1d(int32_t (&v)[8]) {
  typedef uint32_t U;
  const U i0 = (U)v[0], i1 = (U)v[1], i2 = (U)v[2], i3 = (U)v[3], i4 = (U)v[4], i5 = (U)v[5], i6 = (U)v[6],
          i7 = (U)v[7];
  // even part
  U z1 = (i2 + i6) * 4433u;         // FIX(0.541196100)
  U tmp2 = z1 - i6 * 15137u;        // FIX(1.847759065)
  U tmp3 = z1 + i2 * 6270u;         // FIX(0.765366865)
  U tmp0 = (i0 + i4) << 13;
  U tmp1 = (i0 - i4) << 13;
  const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  // odd part
  tmp0 = i7; tmp1 = i5; tmp2 = i3; tmp3 = i1;
  z1 = tmp0 + tmp3;
  U z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
  const U z5 = (z3 + z4) * 9633u;   // FIX(1.175875602)
  tmp0 *= 2446u;                    // FIX(0.298631336)
  tmp1 *= 16819u;                   // FIX(2.053119869)
  tmp2 *= 25172u;                   // FIX(3.072711026)
  tmp3 *= 12299u;                   // FIX(1.501321110)
  z1 = 0u - z1 * 7373u;             // -FIX(0.899976223)
  z2 = 0u - z2 * 20995u;            // -FIX(2.562915447)
  z3 = 0u - z3 * 16069u;            // -FIX(1.961570560)
  z4 = 0u - z4 * 3196u;             // -FIX(0.390180644)
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  const U rnd = (U)1 << (SHIFT - 1);
  v[0] = (int32_t)(tmp10 + tmp3 + rnd) >> SHIFT;
  v[7] = (int32_t)(tmp10 - tmp3 + rnd) >> SHIFT;
  v[1] = (int32_t)(tmp11 + tmp2 + rnd) >> SHIFT;
  v[6] = (int32_t)(tmp11 - tmp2 + rnd) >> SHIFT;
  v[2] = (int32_t)(tmp12 + tmp1 + rnd) >> SHIFT;
  v[5] = (int32_t)(tmp12 - tmp1 + rnd) >> SHIFT;
  v[3] = (int32_t)(tmp13 + tmp0 + rnd) >> SHIFT;
  v[4] = (int32_t)(tmp13 - tmp0 + rnd) >> SHIFT;
}

// level shift and clamp of a row-pass result
AT_MJPG_HD uint32_t mjpg_pixel(int32_t v) {
  v += 128;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// libjpeg's "fancy" (triangle filter) chroma upsampling, one output sample.  `a` is
// the nearer chroma sample, `nb` its neighbour on the output sample's side (the sample
// itself at the picture's edge), `odd` the output column's parity.
// 4:2:2 (h2v1): a and nb are samples of one chroma row.
AT_MJPG_HD int32_t mjpg_up_h2v1(int32_t a, int32_t nb, int odd) { return (3 * a + nb + (odd ? 2 : 1)) >> 2; }
// 4:2:0 (h2v2): a and nb are column sums s = 3 * (nearer row) + (farther row).
AT_MJPG_HD int32_t mjpg_up_h2v2(int32_t a, int32_t nb, int odd) { return (3 * a + nb + (odd ? 7 : 8)) >> 4; }

// libjpeg's YCbCr -> RGB (jdcolor.c: 16-bit fixed point, arithmetic shifts), packed
// B | G << 8 | R << 16.  y, cb, cr in 0..255.
AT_MJPG_HD uint32_t mjpg_bgr(int32_t y, int32_t cb, int32_t cr) {
  cb -= 128;
  cr -= 128;
  int32_t r = y + ((91881 * cr + 32768) >> 16);                 // FIX(1.40200)
  int32_t b = y + ((116130 * cb + 32768) >> 16);                // FIX(1.77200)
  int32_t g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16);   // FIX(0.34414), FIX(0.71414)
  r = r < 0 ? 0 : (r > 255 ? 255 : r);
  g = g < 0 ? 0 : (g > 255 ? 255 : g);
  b = b < 0 ? 0 : (b > 255 ? 255 : b);
  return (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16);
}

// ---- JPEG output (at_jpeg_encode_host, k_jpg_fdct ... k_jpg_pack) -----------------------
// The forward half, libjpeg's integer "slow" path again, shared by the host encoder and the
// kernels so that both produce libjpeg's bytes.
//
// libjpeg's RGB -> YCbCr (jccolor.c: 16-bit fixed point), component c of one pixel, 0..255:
//   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//   Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
// (the constants selected, not three branches: lanes of one wave convert different components)
AT_MJPG_HD int32_t mjpg_ycc(int c, int32_t r, int32_t g, int32_t b) {
  const int32_t kr = c == 0 ? 19595 : (c == 1 ? -11059 : 32768);
  const int32_t kg = c == 0 ? 38470 : (c == 1 ? -21709 : -27439);
  const int32_t kb = c == 0 ? 7471 : (c == 1 ? 32768 : -5329);
  const int32_t off = c == 0 ? 32768 : (128 << 16) + 32767;
  return (kr * r + kg * g + kb * b + off) >> 16;
}
// libjpeg's chroma downsampling (jcsample.c), one output sample of output column `col`:
// 4:2:0 (h2v2) over a 2 x 2 square, the bias alternating 1, 2; 4:2:2 (h2v1) over a pair, 0, 1
AT_MJPG_HD int32_t mjpg_down_h2v2(int32_t a, int32_t b, int32_t c, int32_t d, int col) {
  return (a + b + c + d + 1 + (col & 1)) >> 2;
}
AT_MJPG_HD int32_t mjpg_down_h2v1(int32_t a, int32_t b, int col) { return (a + b + (col & 1)) >> 1; }

// One 1-D pass of libjpeg's integer "slow" forward DCT (jfdctint: the constants of
// mjpg_idct_1d, 2 pass bits) on 8 values in place.  PASS 0 is the row pass (results scaled
// up by 4), PASS 1 the column pass that follows it (the block ends scaled by 8).
template <int PASS>
AT_MJPG_HD void mjpg_fdct_1d(int32_t (&v)[8]) {
  constexpr int kShift = PASS == 0 ? 11 : 15;  // CONST_BITS -/+ PASS1_BITS
  constexpr int32_t kRnd = 1 << (kShift - 1);
  const int32_t t0 = v[0] + v[7], t7 = v[0] - v[7], t1 = v[1] + v[6], t6 = v[1] - v[6];
  const int32_t t2 = v[2] + v[5], t5 = v[2] - v[5], t3 = v[3] + v[4], t4 = v[3] - v[4];
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (PASS == 0) {
    v[0] = (t10 + t11) * 4;
    v[4] = (t10 - t11) * 4;
  } else {
    v[0] = (t10 + t11 + 2) >> 2;
    v[4] = (t10 - t11 + 2) >> 2;
  }
  int32_t z1 = (t12 + t13) * 4433;                    // FIX(0.541196100)
  v[2] = (z1 + t13 * 6270 + kRnd) >> kShift;          // FIX(0.765366865)
  v[6] = (z1 - t12 * 15137 + kRnd) >> kShift;         // FIX(1.847759065)
  z1 = t4 + t7;
  int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int32_t z5 = (z3 + z4) * 9633;                // FIX(1.175875602)
  const int32_t a4 = t4 * 2446, a5 = t5 * 16819;      // FIX(0.298631336), FIX(2.053119869)
  const int32_t a6 = t6 * 25172, a7 = t7 * 12299;     // FIX(3.072711026), FIX(1.501321110)
  z1 *= -7373;                                        // FIX(0.899976223)
  z2 *= -20995;                                       // FIX(2.562915447)
  z3 = z3 * -16069 + z5;                              // FIX(1.961570560)
  z4 = z4 * -3196 + z5;                               // FIX(0.390180644)
  v[7] = (a4 + z1 + z3 + kRnd) >> kShift;
  v[5] = (a5 + z2 + z4 + kRnd) >> kShift;
  v[3] = (a6 + z2 + z3 + kRnd) >> kShift;
  v[1] = (a7 + z1 + z4 + kRnd) >> kShift;
}

// libjpeg's quality rule (jpeg_quality_scaling + jpeg_add_quant_table, baseline): the entry
// of an Annex K base value at quality 1..100
AT_MJPG_HD int32_t mjpg_quant_entry(int32_t base, int quality) {
  const int32_t scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int32_t q = (base * scale + 50) / 100;
  return q < 1 ? 1 : (q > 255 ? 255 : q);
}
// the quantiser: a forward DCT result (scaled by 8) by the table entry q, rounded half away
AT_MJPG_HD int32_t mjpg_quantise(int32_t c, int32_t q) {
  const int32_t d = 8 * q, a = c < 0 ? -c : c;
  const int32_t m = (a + (d >> 1)) / d;
  return c < 0 ? -m : m;
}
// magnitude category of a coefficient or DC difference, at most `most` (10 for AC, 11 for DC:
// 8-bit samples give no more; the clamp makes the bound hold for the buffers' sake whatever
// the arithmetic gave)
AT_MJPG_HD int mjpg_nbits(int32_t v, int most) {
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  const int n = a ? 32 - __builtin_clz(a) : 0;
  return n > most ? most : n;
}

// Annex K.1 base quantisation tables, natural (row-major) order
#define AT_JPG_QBASE_LUMA                                                                         \
  {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  \
   69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,  \
   81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99}
#define AT_JPG_QBASE_CHROMA                                                                       \
  {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, \
   47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, \
   99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}

// sampling codes of the C ABI (AT_JPEG_420 ...)
constexpr int kJpg420 = 0, kJpg422 = 1, kJpg444 = 2;
// Most bits one block can take: a DC code of at most 11 bits with 11 magnitude bits, 63 AC
// codes of at most 16 bits with 10 magnitude bits each (1660); the buffers give every block
// 208 bytes.  Byte stuffing at most doubles a segment.
constexpr int kJpgBlockBytes = 208;
static_assert(22 + 63 * 26 <= 8 * kJpgBlockBytes, "a block's worst case fits its share");

// Geometry of the output stream for a w x h picture (multiples of 8) at a sampling.
struct JpgGeom {
  int hs, vs;        // luma sampling factors
  int bw, bh;        // luma block grid (w / 8, h / 8)
  int mcux, mcuy;    // MCU grid; one restart interval = one MCU row
  int bpm;           // blocks per MCU: hs * vs + 2
  int cw, ch;        // real chroma samples (w / hs, h / vs)
};
AT_MJPG_HD bool jpg_geom(int w, int h, int sampling, JpgGeom* g) {
  if (w < 8 || h < 8 || (w & 7) || (h & 7) || w > 65528 || h > 65528) return false;
  if (sampling != kJpg420 && sampling != kJpg422 && sampling != kJpg444) return false;
  g->hs = sampling == kJpg444 ? 1 : 2;
  g->vs = sampling == kJpg420 ? 2 : 1;
  g->bw = w / 8;
  g->bh = h / 8;
  g->mcux = (g->bw + g->hs - 1) / g->hs;
  g->mcuy = (g->bh + g->vs - 1) / g->vs;
  g->bpm = g->hs * g->vs + 2;
  g->cw = w / g->hs;
  g->ch = h / g->vs;
  return true;
}

// The four Annex K Huffman tables as encoder tables: entry = code | length << 16 for symbol s
// of table [0] DC luma, [1] DC chroma (16 entries each), [2] AC luma, [3] AC chroma (256 each).
constexpr int kJpgDcTab = 16, kJpgAcTab = 256, kJpgTabWords = 2 * kJpgDcTab + 2 * kJpgAcTab;
void jpg_huff_tables(uint32_t* tab /* kJpgTabWords */);
// The stream's header (SOI .. SOS) into dst (cap >= kJpgHeaderMax); returns its length.
constexpr size_t kJpgHeaderMax = 1024;
size_t jpg_write_header(uint8_t* dst, int w, int h, int quality, int sampling);
// A capacity no stream of this geometry exceeds (0: bad geometry).
size_t jpg_max_bytes(int w, int h, int sampling);

// What the marker parser found.
struct MjpgInfo {
  int width, height;
  int ncomp;          // 1 or 3
  int hs, vs;         // luma sampling factors (1x1, 2x1, 2x2)
  int restart;        // restart interval in MCUs (0: none)
  int default_dht;    // a Huffman table slot was filled from the built-in Annex K tables
};

// Entropy decoder with its scratch memory (token and offset lists of one frame):
// one per decoding thread, reused from frame to frame, so nothing is allocated per
// frame once it has seen the largest frame.
class MjpgDecoder {
 public:
  // Parses and entropy-decodes one JPEG.  want_w / want_h > 0: the picture must
  // have exactly that size (kMjpgInvalid otherwise).  On success the luma tokens
  // are held in this object until the next call; info() describes the stream.
  // keep_chroma: the Cb and Cr tokens of a three-component stream are held too, with
  // each component's quantisation table (colour on); pack() then appends them.
  int decode(const uint8_t* jpg, size_t len, int want_w, int want_h, bool keep_chroma = false);
  const MjpgInfo& info() const { return info_; }
  uint32_t nblocks() const { return (uint32_t)(bw_ * bh_); }
  // chroma plane: blocks (0 unless chroma was kept), width in blocks
  uint32_t chroma_nblocks() const { return (uint32_t)(cbw_ * cbh_); }
  // bytes pack() writes (header + payload in the smaller encoding; colour on: the
  // chroma sub-streams and the alignment in front of them too)
  size_t packed_bytes() const;
  bool dense() const;  // the luma stream's encoding
  // Writes the coefficient stream of the decoded frame to dst (cap bytes, at least
  // packed_bytes(); slot_bytes() of the picture's size always suffices).
  int pack(uint8_t* dst, size_t cap) const;
  // The same with every plane in the dense encoding whatever its size (what the device
  // entropy decode leaves in the slot, at_mjpg_entropy.h): dense_bytes() bytes.
  size_t dense_bytes() const;
  int pack_dense(uint8_t* dst, size_t cap) const;
  // The most a frame of w x h pixels can take (every plane dense; colour: 4:4:4).
  static size_t slot_bytes(int w, int h, bool color);
  // Full host decode: the luma plane (width x height) through the same integer IDCT.
  int to_gray(uint8_t* gray, size_t cap) const;
  // Full host decode to BGR8 [height][width][3] (after decode(..., keep_chroma = true)):
  // chroma IDCT, fancy upsampling and colour conversion as libjpeg does them; a
  // single-component stream gives B = G = R = Y.
  int to_bgr(uint8_t* bgr, size_t cap) const;

 private:
  MjpgInfo info_{};
  int bw_ = 0, bh_ = 0;              // visible block grid (ceil(width / 8), ceil(height / 8))
  int gw_ = 0, gh_ = 0;              // decoded (MCU padded) luma block grid
  uint16_t q_[64] = {0};             // luma quantisation table, natural order
  std::vector<uint32_t> tok_;        // tokens in decode order
  std::vector<uint32_t> start_;      // first token of each decoded block (decode order), + end
  uint32_t kept_tokens_ = 0;         // tokens of the visible blocks
  bool chroma_ = false;              // the last decode kept chroma (colour on)
  int cbw_ = 0, cbh_ = 0;            // chroma block grid (the MCU grid); 0 x 0 without chroma
  uint16_t cq_[2][64] = {{0}};       // Cb / Cr quantisation tables, natural order
  std::vector<uint32_t> ctok_[2];    // Cb / Cr tokens, blocks in raster (= decode) order
  std::vector<uint32_t> cstart_[2];  // first token of each chroma block, + end
  uint32_t decode_index(int bx, int by) const;
  // one plane's stream: the blocks of a bw x bh grid, block (bx, by) owning the tokens
  // start[i] .. start[i + 1] with i = decode_index (luma) or raster (chroma)
  struct Plane {
    const uint16_t* q;
    const uint32_t* tok;
    const uint32_t* start;
    int bw, bh;
    uint32_t kept;
    bool luma;
  };
  Plane plane(int c) const;  // 0 luma, 1 Cb, 2 Cr
  uint32_t block_index(const Plane& p, int bx, int by) const {
    return p.luma ? decode_index(bx, by) : (uint32_t)(by * p.bw + bx);
  }
  static bool plane_dense(const Plane& p);
  static size_t plane_bytes(const Plane& p, bool force_dense = false);
  void pack_plane(const Plane& p, uint8_t* dst, bool force_dense = false) const;
  int pack_all(uint8_t* dst, size_t cap, bool force_dense) const;
  // IDCT of the plane's blocks into out (row stride `stride`), cropped to w x h
  void idct_plane(const Plane& p, uint8_t* out, size_t stride, int w, int h) const;
};

}  // namespace at

// Host-only full decode to a luma plane (C ABI, exported from the library; the CPU
// reference of the tests).  Returns 0 or a negative AT_E* code; *w / *h receive the
// picture size as soon as the frame header has been parsed.
extern "C" int at_mjpg_decode_gray_host(const uint8_t* jpg, size_t len, uint8_t* gray, size_t cap, int* w, int* h);
// the same for the colour image: BGR8 [h][w][3], cap >= 3 * w * h (bgr == NULL: header only)
extern "C" int at_mjpg_decode_bgr_host(const uint8_t* jpg, size_t len, uint8_t* bgr, size_t cap, int* w, int* h);
// which encoding a frame of this stream takes on the link to a want_w x want_h detector
// (0 x 0: any size): 0 sparse, 1 dense, < 0 the error at_enqueue_mjpg would give
extern "C" int at_mjpg_stream_mode_host(const uint8_t* jpg, size_t len, int want_w, int want_h,
                                        size_t* stream_bytes);

// Host-only baseline JPEG encoder (the CPU reference of the GPU encoder): BGR8 [h][w][3],
// w and h multiples of 8, quality 1..100, sampling kJpg420 / kJpg422 / kJpg444; one restart
// interval per MCU row.  Writes the whole file; *len receives its size, also when it does
// not fit cap (then -3, AT_E_CAPACITY, and nothing is written).
extern "C" int at_jpeg_encode_host(const uint8_t* bgr, int w, int h, int quality, int sampling, uint8_t* out,
                                   size_t cap, size_t* len);
extern "C" size_t at_jpeg_max_bytes(int width, int height, int sampling);

#endif  // AT_MJPG_H_
