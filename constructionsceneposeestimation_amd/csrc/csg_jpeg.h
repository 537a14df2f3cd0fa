// csg_jpeg.h — baseline JPEG RGB files for csg_encode_jpeg (include/csg_api.h): the file
// format as plain sequential integer arithmetic (host + device, like csg_mask_png.h, so that the CPU
// harness tests/jpeg_host.cpp writes files from the same functions), and the host launcher of the
// kernels in csg_jpeg.hip.  writers.jpeg_bytes restates it in NumPy.
//
// The file is laid out as libjpeg writes a baseline file with one restart interval per MCU row: SOI,
// APP0 (JFIF 1.01, density 1:1, no thumbnail), DQT x 2, SOF0, DHT x 4 (DC0, AC0, DC1, AC1), DRI, SOS,
// entropy data, EOI.  Components Y, Cb, Cr (ids 1, 2, 3) interleaved in one scan, 4:4:4 (MCU 8 x 8:
// Y Cb Cr) or 4:2:0 (MCU 16 x 16: Y00 Y01 Y10 Y11 Cb Cr).  The image extends to whole MCUs by repeating
// its last column and row; 4:2:0 chroma is (a + b + c + d + 2) >> 2 of the extended image's 2 x 2 cells.
// A 4:2:0 luminance block that holds no pixel of the image (right of it or below it, in the last MCU
// column or row) is not transformed: it repeats the DC of the luminance block before it in its MCU and has
// no AC, so it costs a zero DC difference and an EOB, as in libjpeg's files (luma_source).
//
// Colour: JFIF's full-range BT.601 in 16-bit fixed point, one rounding per component:
//   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//   Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
// (each row of constants sums to 65536 or 0, so all three stay in 0..255); samples are level-shifted by
// -128 before the DCT.
//
// Forward DCT.  F = A f A^T with A[u][x] = c(u) / 2 * cos((2x + 1) u pi / 16), c(0) = 1 / sqrt(2), in
// int32: the seven constants k_j = round(2^14 * cos(j pi / 16) / 2) (|k_j - exact| <= 1/2, that is
// delta <= 2^-15 in units of A), rows first, then columns, each as the even / odd split of the matrix
// product (sums s_x = f_x + f_{7-x} feed the even outputs, differences d_x = f_x - f_{7-x} the odd ones).
//   rows:    t = sum k f exactly, |t| <= 2^14 * 2.83 * 128 < 2^23.  Its error from the constants is at
//            most delta * sum |f| <= 2^-15 * 8 * 128 = 2^-5.  t is rounded to 6 fraction bits,
//            t' = (t + 128) >> 8, which adds at most 2^-7: e_row <= 0.0391, and |t'| <= 23171.
//   columns: F' = sum k t' exactly, |F'| <= 8 * 5793 * 23171 < 2^31, at scale 2^20.  Its error is at most
//            sum |A| e_row + delta * sum |t| + delta * 8 * e_row
//            <= 2.83 * 0.0391 + 2^-15 * 8 * 362.1 + 0.00001 = 0.1106 + 0.0884 + 0.00001 < 0.2.
// So F' / 2^20 lies within 0.2 (< the 0.5 asked) of the exact real DCT of the same samples, and no
// rounding follows before the quantiser, which divides F' by q << 20 rounding half away from zero
// (|F'| + (q << 19) < 2^30 + 2^27: no overflow; quantise does it with a multiplication).  AC is clamped to +-1023, the DC difference to +-2047
// (category 11; with |DC| <= 1024 neither clamp is ever reached).
//
// Entropy coding: the four typical Huffman tables of Annex K.3.  The DC predictor of each component is 0
// at the start of every restart interval (one MCU row, DRI = MCUs per row); every interval is padded with
// 1-bits to a byte; RSTm (m counting mod 8) follows every interval but the last; a zero byte follows
// every 0xFF byte of entropy data.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "csg_deflate.h"   // CSG_HD

namespace csg {
namespace jpg {

constexpr uint32_t kHeadBytes = 629;       // SOI .. SOS header: the same for every size, quality and sampling
constexpr uint32_t kDctShift = 20;         // fdct8x8's results are coefficients * 2^20
constexpr uint32_t kMaxBlockBits = 1664;   // DC 9 + 11, AC 63 * (16 + 10): 1658, rounded up to whole dwords
constexpr uint32_t k444 = 0, k420 = 1;

constexpr int32_t kC1 = 8035, kC2 = 7568, kC3 = 6811, kC4 = 5793, kC5 = 4551, kC6 = 3135, kC7 = 1598;

// natural (row-major) index of the coefficient at zig-zag position i
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// What the kernels read of the format's tables, made on the host by build_tables: quantisers in zig-zag
// order with their reciprocals, Huffman codes as code | length << 16 by symbol, and the file's first kHeadBytes bytes.
struct Tables {
  uint16_t q[2][64];
  uint32_t rq[2][64];   // quant_recip of q
  uint32_t dc[2][12];
  uint32_t ac[2][256];
  uint8_t head[640];
};

struct Geometry {
  uint32_t mw, mh;   // MCU size in pixels
  uint32_t bpm;      // blocks per MCU
  uint32_t mx, my;   // MCUs per row, MCU rows (= restart intervals)
};

CSG_HD Geometry geometry(uint32_t W, uint32_t H, uint32_t sub) {
  Geometry g;
  g.mw = g.mh = sub == k420 ? 16u : 8u;
  g.bpm = sub == k420 ? 6u : 3u;
  g.mx = (W + g.mw - 1u) / g.mw;
  g.my = (H + g.mh - 1u) / g.mh;
  return g;
}

// Component (0 Y, 1 Cb, 2 Cr) of block k of an MCU, and how far back in the interval's block order the
// previous block of the same component lies.
CSG_HD uint32_t block_comp(uint32_t sub, uint32_t k) { return sub == k420 ? (k < 4u ? 0u : k - 3u) : k; }
CSG_HD uint32_t pred_distance(uint32_t sub, uint32_t k) { return sub == k420 ? (k == 0u ? 3u : k < 4u ? 1u : 6u) : 3u; }

// Block k (0..3) of a 4:2:0 MCU at MCU column m, MCU row r: k itself where the block holds a pixel of the
// W x H image, else the block of the MCU whose DC it repeats (the nearest one before it that holds one).
CSG_HD uint32_t luma_source(uint32_t W, uint32_t H, uint32_t m, uint32_t r, uint32_t k) {
  const bool col = m * 16u + 8u < W, row = r * 16u + 8u < H;   // the MCU's right column / lower row of blocks
  const uint32_t s1 = col ? 1u : 0u;
  if (k == 1u) return s1;
  if (k >= 2u && !row) return s1;
  return k == 3u && !col ? 2u : k;
}

CSG_HD void ycc(uint32_t r, uint32_t g, uint32_t b, uint32_t& y, uint32_t& cb, uint32_t& cr) {
  const int32_t R = (int32_t)r, G = (int32_t)g, B = (int32_t)b;
  y = (uint32_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
  cb = (uint32_t)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16);
  cr = (uint32_t)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16);
}

// One 8-point pass over a[0], a[s], .. a[7 s], in place; `round` is added and `shift` taken off.
CSG_HD void dct8(int32_t* a, int s, int32_t round, int shift) {
  const int32_t s0 = a[0] + a[7 * s], s1 = a[s] + a[6 * s], s2 = a[2 * s] + a[5 * s], s3 = a[3 * s] + a[4 * s];
  const int32_t d0 = a[0] - a[7 * s], d1 = a[s] - a[6 * s], d2 = a[2 * s] - a[5 * s], d3 = a[3 * s] - a[4 * s];
  a[0] = (kC4 * (s0 + s1 + s2 + s3) + round) >> shift;
  a[4 * s] = (kC4 * (s0 - s1 - s2 + s3) + round) >> shift;
  a[2 * s] = (kC2 * (s0 - s3) + kC6 * (s1 - s2) + round) >> shift;
  a[6 * s] = (kC6 * (s0 - s3) - kC2 * (s1 - s2) + round) >> shift;
  a[s] = (kC1 * d0 + kC3 * d1 + kC5 * d2 + kC7 * d3 + round) >> shift;
  a[3 * s] = (kC3 * d0 - kC7 * d1 - kC1 * d2 - kC5 * d3 + round) >> shift;
  a[5 * s] = (kC5 * d0 - kC1 * d1 + kC7 * d2 + kC3 * d3 + round) >> shift;
  a[7 * s] = (kC7 * d0 - kC5 * d1 + kC3 * d2 - kC1 * d3 + round) >> shift;
}

// v: 64 level-shifted samples (-128 .. 127), row-major; on return coefficient (v, u) * 2^kDctShift at 8 v + u.
CSG_HD void fdct8x8(int32_t* v) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 8; ++r) dct8(v + 8 * r, 1, 128, 8);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int c = 0; c < 8; ++c) dct8(v + c, 8, 0, 0);
}

// F (a coefficient * 2^kDctShift) over quantiser q (1..255), rounded half away from zero:
// (|F| + d / 2) / d with d = q << 20.  Without a division: floor(n / (q << 20)) = floor((n >> 20) / q), and
// for a = n >> 20 < 2^11 and rq = ceil(2^20 / q) (quant_recip) floor(a / q) = (a * rq) >> 20 exactly, because
// a * (rq * q - 2^20) < 2^11 * 255 < 2^20; a * rq < 2^31.
CSG_HD uint32_t quant_recip(uint32_t q) { return ((1u << 20) + q - 1u) / q; }
CSG_HD int32_t quantise(int32_t F, uint32_t q, uint32_t rq) {
  const uint32_t a = ((uint32_t)(F < 0 ? -F : F) + (q << (kDctShift - 1u))) >> kDctShift, m = (a * rq) >> 20;
  return F < 0 ? -(int32_t)m : (int32_t)m;
}
CSG_HD int32_t clamp_ac(int32_t v) { return v < -1023 ? -1023 : v > 1023 ? 1023 : v; }
CSG_HD int32_t clamp_dc_diff(int32_t v) { return v < -2047 ? -2047 : v > 2047 ? 2047 : v; }

// Bits of |v|: the size category of a coefficient.
CSG_HD uint32_t category(int32_t v) {
  const uint32_t m = (uint32_t)(v < 0 ? -v : v);
  return m ? 32u - (uint32_t)__builtin_clz(m) : 0u;
}

// A block's symbols through put(value, nbits), at most 26 bits each: the DC difference, then run / size
// symbols with ZRL and EOB over coef(1) .. coef(63) (zig-zag order).
template <class Coef, class Put>
CSG_HD void block_codes(Coef&& coef, int32_t dc_diff, const uint32_t* dc, const uint32_t* ac, Put&& put) {
  {
    const uint32_t s = category(dc_diff), c = dc[s];
    const uint32_t ex = (uint32_t)(dc_diff < 0 ? dc_diff - 1 : dc_diff) & ((1u << s) - 1u);
    put(((c & 0xFFFFu) << s) | ex, (c >> 16) + s);
  }
  uint32_t run = 0;
  for (uint32_t i = 1; i < 64u; ++i) {
    const int32_t v = coef(i);
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run >= 16u; run -= 16u) put(ac[0xF0] & 0xFFFFu, ac[0xF0] >> 16);
    const uint32_t s = category(v), c = ac[(run << 4) | s];
    put(((c & 0xFFFFu) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), (c >> 16) + s);
    run = 0;
  }
  if (run) put(ac[0] & 0xFFFFu, ac[0] >> 16);
}

// Bits of a block's AC symbols.
CSG_HD uint32_t ac_bits(const int16_t* zz, const uint32_t* ac) {
  uint32_t bits = 0, run = 0;
  for (uint32_t i = 1; i < 64u; ++i) {
    const int32_t v = zz[i];
    if (v == 0) {
      ++run;
      continue;
    }
    bits += (run >> 4) * (ac[0xF0] >> 16);
    const uint32_t s = category(v);
    bits += (ac[((run & 15u) << 4) | s] >> 16) + s;
    run = 0;
  }
  return bits + (run ? ac[0] >> 16 : 0u);
}
CSG_HD uint32_t dc_bits(int32_t dc_diff, const uint32_t* dc) {
  const uint32_t s = category(dc_diff);
  return (dc[s] >> 16) + s;
}

// Bytes of one interval's staging slot: its blocks at their most bits, a whole number of dwords.
CSG_HD uint32_t slot_bytes(const Geometry& g) { return g.mx * g.bpm * (kMaxBlockBits / 8u); }

// Bytes of a file whose intervals take `entropy` bytes in all (padding and stuffing included).
CSG_HD uint64_t file_bytes(const Geometry& g, uint64_t entropy) { return kHeadBytes + entropy + 2ull * (g.my - 1u) + 2u; }

// ---- tables (host) -------------------------------------------------------------------------------------------

namespace detail {
// Annex K.1 and K.2, row-major
static const uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
     69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
     81, 104, 113, 92, 49, 64, 78,  87,  103, 121, 120, 101, 72, 92, 95,  98,  112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3: codes per length 1..16, then the symbols in code order
static const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// Canonical codes (Annex C) of a table whose symbols are vals[0 .. n): code | length << 16 at codes[symbol].
inline void canonical(const uint8_t* bits, const uint8_t* vals, uint32_t* codes) {
  uint32_t code = 0, k = 0;
  for (uint32_t len = 1; len <= 16u; ++len) {
    for (uint32_t i = 0; i < bits[len - 1u]; ++i) codes[vals[k++]] = code++ | (len << 16);
    code <<= 1;
  }
}
}  // namespace detail

// libjpeg's quality rule on an Annex K base value.
inline uint32_t scaled_q(uint32_t base, uint32_t quality) {
  const uint32_t s = quality < 50u ? 5000u / quality : 200u - 2u * quality;
  const uint32_t t = (base * s + 50u) / 100u;
  return t < 1u ? 1u : t > 255u ? 255u : t;
}

// Fills t for a W x H file at `quality` (1..100) and sampling `sub`; t.head gets the kHeadBytes bytes
// SOI .. SOS header.  Returns the bytes written to t.head.
inline uint32_t build_tables(Tables& t, uint32_t W, uint32_t H, uint32_t quality, uint32_t sub) {
  using namespace detail;
  const Geometry g = geometry(W, H, sub);
  t = Tables{};
  for (uint32_t c = 0; c < 2u; ++c)
    for (uint32_t i = 0; i < 64u; ++i) {
      t.q[c][i] = (uint16_t)scaled_q(kBaseQ[c][kZigzag[i]], quality);
      t.rq[c][i] = quant_recip(t.q[c][i]);
    }
  static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  for (uint32_t c = 0; c < 2u; ++c) {
    canonical(kDcBits[c], dc_vals, t.dc[c]);
    canonical(kAcBits[c], kAcVals[c], t.ac[c]);
  }
  uint32_t n = 0;
  auto put = [&](uint32_t b) { t.head[n++] = (uint8_t)b; };
  auto put16 = [&](uint32_t v) {
    put(v >> 8);
    put(v & 255u);
  };
  put16(0xFFD8);
  put16(0xFFE0);
  put16(16);
  for (const char* s = "JFIF"; *s; ++s) put((uint8_t)*s);
  put(0);
  put16(0x0101);   // version 1.01
  put(0);          // density unit: aspect ratio only
  put16(1);
  put16(1);
  put16(0);        // no thumbnail
  for (uint32_t c = 0; c < 2u; ++c) {
    put16(0xFFDB);
    put16(67);
    put(c);
    for (uint32_t i = 0; i < 64u; ++i) put(t.q[c][i]);
  }
  put16(0xFFC0);
  put16(17);
  put(8);
  put16(H);
  put16(W);
  put(3);
  for (uint32_t c = 0; c < 3u; ++c) {
    put(c + 1u);
    put(c == 0u && sub == k420 ? 0x22u : 0x11u);
    put(c ? 1u : 0u);
  }
  for (uint32_t k = 0; k < 4u; ++k) {   // DC0, AC0, DC1, AC1
    const uint32_t c = k >> 1, is_ac = k & 1u, nv = is_ac ? 162u : 12u;
    put16(0xFFC4);
    put16(19u + nv);
    put((is_ac << 4) | c);
    for (uint32_t i = 0; i < 16u; ++i) put(is_ac ? kAcBits[c][i] : kDcBits[c][i]);
    for (uint32_t i = 0; i < nv; ++i) put(is_ac ? kAcVals[c][i] : dc_vals[i]);
  }
  put16(0xFFDD);
  put16(4);
  put16(g.mx);
  put16(0xFFDA);
  put16(12);
  put(3);
  for (uint32_t c = 0; c < 3u; ++c) {
    put(c + 1u);
    put(c ? 0x11u : 0x00u);
  }
  put(0);
  put(63);
  put(0);
  return n;
}

}  // namespace jpg

#if defined(__HIPCC__)
// A csg_jpeg_job with the pass's scratch, for one range of frames; all pointers are device memory.
struct JpegArgs {
  uint32_t W, H, sub;
  uint32_t first, n;           // the range: frames first .. first + n - 1
  jpg::Geometry g;
  uint32_t slot;               // bytes of one interval's staging slot (jpg::slot_bytes)
  const jpg::Tables* tables;
  const uint8_t* rgb;          // [all frames][H][W][3]
  int16_t* coef;               // [n][my][mx * bpm][64] scratch: quantised coefficients, zig-zag order, DC absolute
  uint32_t* abits;             // [n][my][mx * bpm] scratch: bits of each block's AC symbols
  uint8_t* zbuf;               // [n][my][slot] scratch: each interval's padded, unstuffed stream
  uint32_t* isize;             // [n][my] scratch: each interval's bytes, unstuffed
  uint32_t* ipos;              // [n][my] scratch: each interval's stuffed bytes, then its offset in the entropy data
  uint64_t* fsize;             // [n] scratch: bytes of each file
  uint8_t* out;
  uint64_t out_capacity;
  uint64_t* file_offsets;      // [all frames + 1]
};

// Enqueues one range: blocks, emit, layout, offsets, pack.
void launch_jpeg(const JpegArgs& a, hipStream_t st);
#endif

}  // namespace csg
