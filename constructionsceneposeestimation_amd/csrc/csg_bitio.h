// csg_bitio.h — the device-side writers the GPU file encoders share (csg_encode.hip, csg_mask_png.hip):
// bits into zeroed staging words, bytes to an arbitrary offset, and the CRC-32 step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csg {

// LSB-first bits into zeroed staging words from bit `pos`: the first word
// (possibly shared with the previous row) and the last (possibly shared with
// the next) with atomicOr, words in between with plain stores.
struct WordBits {
  uint32_t* w;
  uint64_t acc;
  uint32_t n, wi;
  bool first;
  __device__ void init(uint32_t* words, uint32_t pos) {
    w = words;
    wi = pos >> 5;
    n = pos & 31u;
    acc = 0;
    first = true;
  }
  __device__ __forceinline__ void put(uint32_t v, uint32_t len) {
    acc |= (uint64_t)v << n;
    n += len;
    if (n >= 32u) {
      const uint32_t word = (uint32_t)acc;
      if (first) atomicOr(&w[wi], word);
      else w[wi] = word;
      first = false;
      ++wi;
      acc >>= 32;
      n -= 32u;
    }
  }
  __device__ void finish() {
    if (n) atomicOr(&w[wi], (uint32_t)acc);
  }
};

// Bytes to an arbitrary offset: byte stores up to a dword boundary, then
// whole dwords, the tail again as bytes.
struct ByteOut {
  uint8_t* base;
  uint64_t pos;
  uint32_t acc, na;
  __device__ void init(uint8_t* b, uint64_t p) {
    base = b;
    pos = p;
    acc = 0;
    na = 0;
  }
  __device__ __forceinline__ void put(uint32_t c) {
    if (na == 0 && (pos & 3u)) {
      base[pos++] = (uint8_t)c;
      return;
    }
    acc |= (c & 255u) << (8u * na);
    ++pos;
    if (++na == 4u) {
      *reinterpret_cast<uint32_t*>(base + pos - 4u) = acc;
      acc = 0;
      na = 0;
    }
  }
  __device__ void be32(uint32_t v) {
    put(v >> 24);
    put((v >> 16) & 255u);
    put((v >> 8) & 255u);
    put(v & 255u);
  }
  __device__ void finish() {
    for (uint32_t k = 0; k < na; ++k) base[pos - na + k] = (uint8_t)(acc >> (8u * k));
    na = 0;
    acc = 0;
  }
};

struct Crc {
  const uint32_t* T;
  uint32_t c;
  __device__ __forceinline__ void add(uint32_t b) { c = T[(c ^ b) & 255u] ^ (c >> 8); }
};

}  // namespace csg
