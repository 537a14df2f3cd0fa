// mask_png_host.cpp — a one-thread encoder of the mask PNG of csg_encode_span_masks, built from
// csrc/csg_mask_png.h: the same row walker, token sizes, token bits, Adler-32 terms and layout arithmetic
// the GPU kernels use, in the kernels' order (sizes, layout, emit into zeroed words, pack).
// tests/test_mask_png.py compares its files with writers.mask_png_bytes byte for byte.
//
//   mask_png_host W H mask.raw out.png     mask.raw: H * W bytes, row-major, non-zero = set
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../constructionsceneposeestimation_amd/csrc/csg_mask_png.h"

using namespace csg;

static void be32(std::vector<uint8_t>& o, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s));
}

static void chunk(std::vector<uint8_t>& o, const char* tag, const uint8_t* data, uint32_t n) {
  be32(o, n);
  uint32_t c = 0xFFFFFFFFu;
  for (int k = 0; k < 4; ++k) {
    o.push_back((uint8_t)tag[k]);
    c = dfl::crc_entry((c ^ (uint8_t)tag[k]) & 255u) ^ (c >> 8);
  }
  for (uint32_t k = 0; k < n; ++k) {
    o.push_back(data[k]);
    c = dfl::crc_entry((c ^ data[k]) & 255u) ^ (c >> 8);
  }
  be32(o, c ^ 0xFFFFFFFFu);
}

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: mask_png_host W H mask.raw out.png\n");
    return 2;
  }
  const uint32_t W = (uint32_t)atoi(argv[1]), H = (uint32_t)atoi(argv[2]);
  if (W < 1 || W > 8192 || H < 1 || H > 8192) return 2;
  std::vector<uint8_t> mask((size_t)W * H);
  FILE* fh = fopen(argv[3], "rb");
  if (!fh || fread(mask.data(), 1, mask.size(), fh) != mask.size()) return 1;
  fclose(fh);
  // the bit plane, as the painter lays it out: word k of row y at k * H + y
  const uint32_t KW = 2u * ((W + 63u) / 64u);
  std::vector<uint32_t> plane((size_t)KW * H, 0u);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x)
      if (mask[(size_t)y * W + x]) plane[(size_t)(x >> 5) * H + y] |= 1u << (x & 31u);
  // sizes and Adler-32 terms per row, then the layout
  std::vector<uint32_t> pos(H);
  uint64_t bits = 0;
  uint32_t sum_a = 0, sum_b = 0;
  for (uint32_t y = 0; y < H; ++y) {
    const mpng::RowSums s = mpng::row_sums(W, H, y, [&](uint32_t k) { return plane[(size_t)k * H + y]; });
    pos[y] = (uint32_t)(mpng::kHeadBits + bits);
    bits += s.bits;
    sum_a = (sum_a + s.a) % dfl::kAdlerMod;
    sum_b = (sum_b + s.b) % dfl::kAdlerMod;
  }
  const uint32_t zbytes = mpng::zlib_bytes(bits), adler = mpng::stream_adler(W, H, sum_a, sum_b);
  if (zbytes > mpng::max_zlib_bytes(W, H)) return 3;
  // emit: each row's tokens at its own bit position into zeroed words
  std::vector<uint32_t> words((zbytes + 3u) / 4u + 1u, 0u);
  words[0] |= mpng::kHeadWord;
  for (uint32_t y = 0; y < H; ++y) {
    uint32_t at = pos[y];
    mpng::row_runs(W, [&](uint32_t k) { return plane[(size_t)k * H + y]; },
                   [&](uint32_t b, uint32_t, uint32_t len) {
                     mpng::run_emit(b, len, [&](uint32_t v, uint32_t nb) {
                       const uint64_t sv = (uint64_t)v << (at & 31u);
                       words[at >> 5] |= (uint32_t)sv;
                       if ((at & 31u) + nb > 32u) words[(at >> 5) + 1u] |= (uint32_t)(sv >> 32);
                       at += nb;
                     });
                   });
    if (at != (y + 1u < H ? pos[y + 1u] : (uint32_t)(mpng::kHeadBits + bits))) return 4;   // sizes and emit disagree
  }
  std::vector<uint8_t> z(zbytes);
  for (uint32_t k = 0; k < zbytes - 4u; ++k) z[k] = (uint8_t)(words[k >> 2] >> (8u * (k & 3u)));
  for (uint32_t k = 0; k < 4u; ++k) z[zbytes - 4u + k] = (uint8_t)(adler >> (8u * (3u - k)));
  // pack
  std::vector<uint8_t> o = {137, 80, 78, 71, 13, 10, 26, 10};
  uint8_t ihdr[13];
  for (uint32_t k = 0; k < 13u; ++k) ihdr[k] = (uint8_t)mpng::ihdr_byte(4u + k, W, H);
  chunk(o, "IHDR", ihdr, 13u);
  for (uint32_t ch = 0; ch < mpng::idat_chunks(zbytes); ++ch) {
    const uint32_t n = zbytes - ch * dfl::kIdatBytes < dfl::kIdatBytes ? zbytes - ch * dfl::kIdatBytes : dfl::kIdatBytes;
    chunk(o, "IDAT", z.data() + (size_t)ch * dfl::kIdatBytes, n);
  }
  chunk(o, "IEND", nullptr, 0u);
  if (o.size() != mpng::file_bytes(zbytes)) return 5;
  fh = fopen(argv[4], "wb");
  if (!fh || fwrite(o.data(), 1, o.size(), fh) != o.size()) return 1;
  fclose(fh);
  return 0;
}
