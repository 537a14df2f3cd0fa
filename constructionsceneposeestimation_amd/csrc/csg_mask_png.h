// csg_mask_png.h — per-object mask PNGs for csg_encode_span_masks (include/csg_api.h):
// the file format as plain sequential arithmetic (host + device, like csg_deflate.h, so that the CPU
// harness tests/mask_png_host.cpp writes files from the same functions), and the host launchers of the
// kernels in csg_mask_png.hip.
//
// The file: an 8-bit grey PNG (0 / 255), filter None on every row, one zlib stream (78 01) holding one
// fixed-Huffman deflate block (RFC 1951 3.2.6) of literals and distance-1 matches, split into IDAT
// chunks of dfl::kIdatBytes.  Each row's 1 + W bytes (the filter byte joins a leading run of zeros) are
// cut into maximal runs of equal bytes and each run is emitted with dfl::run_tokens.  A mask has two byte
// values, so the tokens need no histogram and no code construction: two walks (sizes, emit) suffice.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "csg_deflate.h"

namespace csg {
namespace mpng {

constexpr uint32_t kHeadBits = 19;   // 78 01, then BFINAL = 1 and BTYPE = 01: the tokens start at this bit
constexpr uint32_t kHeadWord = 0x0178u | (3u << 16);
constexpr uint32_t kEobBits = 7;     // the end-of-block code: seven zero bits
constexpr uint32_t kDistBits = 5;    // distance code 0 (distance 1): five zero bits
constexpr uint32_t kSigIhdrBytes = 33;   // signature, IHDR chunk
constexpr uint32_t kIendBytes = 12;

// Fixed code of literal / length symbol s, as dfl::canonical_codes packs one: reversed code | length << 16.
CSG_HD uint32_t fixed_code(uint32_t s) {
  uint32_t v, l;
  if (s < 144u) {
    v = 0x30u + s;
    l = 8;
  } else if (s < 256u) {
    v = 0x190u + (s - 144u);
    l = 9;
  } else if (s < 280u) {
    v = s - 256u;
    l = 7;
  } else {
    v = 0xC0u + (s - 280u);
    l = 8;
  }
  uint32_t r = 0;
  for (uint32_t k = 0; k < l; ++k) r |= ((v >> k) & 1u) << (l - 1u - k);
  return r | (l << 16);
}

// The maximal runs of one row's 1 + W bytes, in order: run(b, pos, len) with b = 0 or 255 and pos the
// index of the run's first byte in the row.  word(k) holds pixels 32k .. 32k + 31 of the row (bit j is
// pixel 32k + j, set = 255); bits at or beyond W are ignored.
template <class Word, class Run>
CSG_HD void row_runs(uint32_t W, Word&& word, Run&& run) {
  uint32_t v = 0, pos = 0, len = 1;   // the filter byte opens a run of zeros
  for (uint32_t k = 0; k * 32u < W; ++k) {
    uint32_t n = W - k * 32u < 32u ? W - k * 32u : 32u;
    uint32_t x = word(k) ^ (0u - v);   // set: a pixel that differs from the open run's value
    if (n < 32u) x &= (1u << n) - 1u;
    while (x) {
      const uint32_t t = (uint32_t)__builtin_ctz(x);   // < n
      len += t;
      run(v * 255u, pos, len);
      pos += len;
      len = 0;
      v ^= 1u;
      n -= t;
      x = ~(x >> t);   // against the new value: bit 0 is clear
      if (n < 32u) x &= (1u << n) - 1u;
    }
    len += n;
  }
  run(v * 255u, pos, len);
}

// Bits of a run's tokens.
CSG_HD uint32_t run_bits(uint32_t b, uint32_t len) {
  uint32_t bits = 0;
  const uint32_t lit_bits = b < 144u ? 8u : 9u;
  dfl::run_tokens(b, len, [&](uint32_t) { bits += lit_bits; },
                  [&](uint32_t l) {
                    uint32_t sym, ne, ex;
                    dfl::length_code(l, sym, ne, ex);
                    bits += (sym < 280u ? 7u : 8u) + ne + kDistBits;
                  });
  return bits;
}

// A run's tokens through put(value, nbits), LSB first.
template <class Put>
CSG_HD void run_emit(uint32_t b, uint32_t len, Put&& put) {
  const uint32_t lc = fixed_code(b);
  dfl::run_tokens(b, len, [&](uint32_t) { put(lc & 0xFFFFu, lc >> 16); },
                  [&](uint32_t l) {
                    uint32_t sym, ne, ex;
                    dfl::length_code(l, sym, ne, ex);
                    const uint32_t c = fixed_code(sym);
                    put((c & 0xFFFFu) | (ex << (c >> 16)), (c >> 16) + ne + kDistBits);   // <= 8 + 5 + 5 bits
                  });
}

// What a row adds to the stream: its token bits and its terms of the stream's Adler-32 sums.  With
// n = 1 + W bytes per row and N = H * n in all, the checksum is a = 1 + sum of bytes and
// b = N + sum of byte_i * (N - i); a byte at position p of row r weighs (n - p) + (H - 1 - r) * n, so the
// sums over rows of `a` and `b` below, folded once with dfl::adler_cat, are the stream's.
struct RowSums {
  uint32_t bits, a, b;   // a, b mod 65521
};

template <class Word>
CSG_HD RowSums row_sums(uint32_t W, uint32_t H, uint32_t r, Word&& word) {
  const uint32_t n = 1u + W;
  uint32_t bits = 0;
  uint64_t cnt = 0, wsum = 0;   // 255-bytes of the row, and the sum of their (n - p): < 2^27
  row_runs(W, word, [&](uint32_t b, uint32_t pos, uint32_t len) {
    bits += run_bits(b, len);
    if (b) {
      cnt += len;
      wsum += (uint64_t)len * (n - pos) - (uint64_t)len * (len - 1u) / 2u;
    }
  });
  const uint64_t a = 255u * cnt % dfl::kAdlerMod, below = (uint64_t)(H - 1u - r) * n % dfl::kAdlerMod;
  return RowSums{bits, (uint32_t)a, (uint32_t)((255u * wsum + a * below) % dfl::kAdlerMod)};
}

CSG_HD uint32_t stream_adler(uint32_t W, uint32_t H, uint32_t sum_a, uint32_t sum_b) {
  uint32_t a = 1, b = 0;
  dfl::adler_cat(a, b, sum_a % dfl::kAdlerMod, sum_b % dfl::kAdlerMod, (uint64_t)H * (1u + W));
  return (b << 16) | a;
}

// Bytes of the zlib stream whose tokens take `token_bits`, and of the file around it.
CSG_HD uint32_t zlib_bytes(uint64_t token_bits) { return (uint32_t)((kHeadBits + token_bits + kEobBits + 7u) / 8u) + 4u; }
CSG_HD uint32_t idat_chunks(uint32_t zbytes) { return (zbytes + dfl::kIdatBytes - 1u) / dfl::kIdatBytes; }
CSG_HD uint64_t file_bytes(uint32_t zbytes) {
  return (uint64_t)kSigIhdrBytes + 12ull * idat_chunks(zbytes) + zbytes + kIendBytes;
}
// The most token bits a row can take (every pixel a run of its own, nine bits each), and so the most
// bytes of one stream: 8192 x 8192 stays below 2^26 bytes and 2^30 bits, so 32-bit positions hold.
CSG_HD uint32_t max_zlib_bytes(uint32_t W, uint32_t H) { return zlib_bytes((uint64_t)H * (1u + W) * 9u); }

// The 17 bytes the IHDR chunk's CRC covers: the tag, W, H, bit depth 8, then colour type 0 (grey),
// compression, filter and interlace 0.  (No table: a dynamically indexed one lives in scratch memory.)
CSG_HD uint32_t ihdr_byte(uint32_t k, uint32_t W, uint32_t H) {
  if (k < 4u) return (0x52444849u >> (8u * k)) & 255u;   // "IHDR"
  if (k < 8u) return (W >> (8u * (7u - k))) & 255u;
  if (k < 12u) return (H >> (8u * (11u - k))) & 255u;
  return k == 12u ? 8u : 0u;
}

}  // namespace mpng

#if defined(__HIPCC__)
struct SpanRec;

// One mask file to make: the layout of csg_mask_item (include/csg_api.h).
struct MaskItem {
  uint32_t frame, label;
};

// What k_mp_layout leaves per item of a range.
struct MaskFile {
  uint64_t fsize;    // bytes of the file
  uint64_t zoff;     // its zlib stream's byte offset in the staging, a multiple of 4
  uint32_t zbytes;   // bytes of the zlib stream
  uint32_t adler;
};

// A csg_mask_png_job with the pass's scratch, for one range of items; all pointers are device memory.
struct MaskPngArgs {
  uint32_t W, H;
  uint32_t L, C;              // labels and span records per frame of the span arrays
  uint32_t KW;                // plane words per row: 2 * ceil(W / 64)
  uint32_t first, n;          // the range: items first .. first + n - 1
  const SpanRec* spans;       // [frames][C]
  const uint32_t* offsets;    // [frames][L + 1]
  const MaskItem* items;      // [all items]
  uint32_t* planes;           // [n][KW][H] scratch: word k of row y of item i at (i * KW + k) * H + y
  uint32_t* rows;             // [3][n][H] scratch: token bits (then their bit position), Adler a and b terms
  MaskFile* files;            // [n] scratch
  uint8_t* zbuf;              // staging of the range's zlib streams, zcap bytes (a multiple of 16)
  uint64_t zcap;
  uint8_t* out;
  uint64_t out_capacity;
  uint64_t* file_offsets;     // [all items + 1]
};

// Enqueues one range: paint, rows, layout, zero, emit, pack.
void launch_mask_png(const MaskPngArgs& a, hipStream_t st);
#endif

}  // namespace csg
