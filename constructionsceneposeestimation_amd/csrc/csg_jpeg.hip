// csg_jpeg.hip — baseline JPEG RGB files for csg_encode_jpeg: rgb[F][H][W][3] on the device becomes
// finished, packed .jpg files without leaving the GPU.  The file format is csg_jpeg.h's,
// restated in NumPy by writers.jpeg_bytes.  Integer arithmetic only.
//
//   k_jpg_blocks   per (128-pixel strip of an MCU row): colour conversion with edge extension into LDS planes,
//                  then one lane per 8 x 8 block: chroma mean, DCT, quantiser, zig-zag, AC bits
//   k_jpg_emit     per restart interval (MCU row), 1024 threads: DC differences, the blocks' bit positions (block scan), their
//                  codes into the interval's staging slot, the 1-bit padding, and the count of 0xFF bytes
//   k_jpg_layout   per frame: the intervals' offsets in the file's entropy data (block scan), the file's size
//   k_jpg_offsets  the range's file offsets, continued in 64 bits from the previous range
//   k_jpg_pack     per restart interval: the slot's bytes into the file with a zero behind every 0xFF, then RSTm
//                  or EOI; the frame's first interval also writes the header
//
// No global atomics and no memset: k_jpg_emit's threads own consecutive blocks, so a thread stores every
// byte that lies whole inside its bits itself, and the at most two bytes it shares with its neighbours go
// through LDS to the one thread that owns the byte's first bit.  Every byte of a slot below the interval's
// size is stored exactly once, so the staging is a pure function of the input.
//
// Bounds.  RGB is read at clamped coordinates only.  Coefficients, bit counts and sizes are indexed by
// (frame of the range, MCU row, block) below the counts the scratch was sized with.  A slot holds its
// interval's blocks at jpg::kMaxBlockBits each, more than any block can take; its stores are checked
// against the slot all the same.  File stores stay inside [foff, foff + fsize), which is checked against
// out_capacity: a file that does not fit is not written at all.
#include "csg_jpeg.h"

#include <algorithm>

#include "csg_bitio.h"

namespace csg {

using namespace jpg;

namespace {

constexpr uint32_t kStripPx = 128;      // pixels of an MCU row one wave converts: 16 MCUs of 8, or 8 of 16
constexpr uint32_t kStripBlocks = 48;   // ... and their blocks: 16 * 3 or 8 * 6

// grid (strips, MCU rows, frames of the range), one wave per workgroup
__global__ __launch_bounds__(64) void k_jpg_blocks(JpegArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t plane[3][16 * kStripPx];
  const uint32_t lane = threadIdx.x, strip = blockIdx.x, r = blockIdx.y, f = blockIdx.z;
  const uint32_t W = a.W, H = a.H, mh = a.g.mh;
  const uint8_t* img = a.rgb + (size_t)(a.first + f) * H * W * 3u;
  const uint32_t x0 = strip * kStripPx, y0 = r * mh;
  for (uint32_t p = lane; p < mh * kStripPx; p += 64u) {   // the image's only read: adjacent lanes, adjacent pixels
    const uint32_t x = min(x0 + (p & (kStripPx - 1u)), W - 1u), y = min(y0 + p / kStripPx, H - 1u);
    const uint8_t* px = img + ((size_t)y * W + x) * 3u;
    uint32_t yy, cb, cr;
    ycc(px[0], px[1], px[2], yy, cb, cr);
    plane[0][p] = (uint8_t)yy;
    plane[1][p] = (uint8_t)cb;
    plane[2][p] = (uint8_t)cr;
  }
  __syncthreads();
  const bool sub = a.sub == k420;
  const uint32_t bpm = a.g.bpm, ml = lane / bpm, k = lane - ml * bpm;
  const uint32_t m = strip * (kStripPx / a.g.mw) + ml;
  if (lane >= kStripBlocks || m >= a.g.mx) return;
  const uint32_t comp = block_comp(a.sub, k);
  const uint32_t src = sub && comp == 0u ? luma_source(W, H, m, r, k) : k;
  int32_t v[64];
  if (sub && comp) {   // 2 x 2 means of the MCU's 16 x 16 chroma samples
    const uint8_t* p = plane[comp] + ml * 16u;
#pragma unroll
    for (uint32_t y = 0; y < 8u; ++y) {
      const uint4 t = *reinterpret_cast<const uint4*>(p + (2u * y) * kStripPx);
      const uint4 b = *reinterpret_cast<const uint4*>(p + (2u * y + 1u) * kStripPx);
      const uint32_t tw[4] = {t.x, t.y, t.z, t.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (uint32_t x = 0; x < 8u; ++x) {
        const uint32_t tt = tw[x >> 1] >> (16u * (x & 1u)), bb = bw[x >> 1] >> (16u * (x & 1u));
        v[8u * y + x] = (int32_t)(((tt & 255u) + ((tt >> 8) & 255u) + (bb & 255u) + ((bb >> 8) & 255u) + 2u) >> 2) - 128;
      }
    }
  } else {
    const uint8_t* p = sub ? plane[0] + ((src >> 1) * 8u) * kStripPx + ml * 16u + (src & 1u) * 8u : plane[comp] + ml * 8u;
#pragma unroll
    for (uint32_t y = 0; y < 8u; ++y) {
      const uint2 t = *reinterpret_cast<const uint2*>(p + y * kStripPx);
#pragma unroll
      for (uint32_t x = 0; x < 8u; ++x) v[8u * y + x] = (int32_t)(((x < 4u ? t.x : t.y) >> (8u * (x & 3u))) & 255u) - 128;
    }
  }
  fdct8x8(v);
  const uint16_t* q = a.tables->q[comp ? 1 : 0];
  const uint32_t* rq = a.tables->rq[comp ? 1 : 0];
  const uint32_t* ac = a.tables->ac[comp ? 1 : 0];
  const bool keep_ac = src == k;
  uint32_t w[32];   // the block's 64 int16 coefficients in zig-zag order
  uint32_t bits = 0, run = 0;
#pragma unroll
  for (uint32_t i = 0; i < 64u; ++i) {
    int32_t c = quantise(v[kZigzag[i]], q[i], rq[i]);
    if (i) {
      c = keep_ac ? clamp_ac(c) : 0;
      if (c == 0) {
        ++run;
      } else {   // as jpg::ac_bits counts them
        bits += (run >> 4) * (ac[0xF0] >> 16);
        const uint32_t s = category(c);
        bits += (ac[((run & 15u) << 4) | s] >> 16) + s;
        run = 0;
      }
    }
    if (i & 1u) w[i >> 1] |= (uint32_t)(uint16_t)c << 16;
    else w[i >> 1] = (uint32_t)(uint16_t)c;
  }
  if (run) bits += ac[0] >> 16;
  const size_t blk = ((size_t)f * a.g.my + r) * a.g.mx * bpm + (size_t)m * bpm + k;
  uint4* dst = reinterpret_cast<uint4*>(a.coef + blk * 64u);
#pragma unroll
  for (uint32_t i = 0; i < 8u; ++i) dst[i] = make_uint4(w[4u * i], w[4u * i + 1u], w[4u * i + 2u], w[4u * i + 3u]);
  a.abits[blk] = bits;
}

constexpr uint32_t kNone = 0xFFFFFFFFu;

// MSB-first bits from bit `pos` of a slot as whole bytes.  A byte whose first bit is another thread's (the
// one `pos` lies in, unless pos is a multiple of 8) is kept in `head`; the bits left at the end, a byte
// whose first bit is this thread's, in `tail`.  ff counts the 0xFF bytes stored.
struct SlotBits {
  uint8_t* z;
  uint32_t cap;
  uint64_t acc;
  uint32_t cnt, at;                // bits held in acc (the first byte's foreign bits included); next byte
  uint32_t head, head_at, tail, tail_at, ff;
  bool in_head;
  __device__ void init(uint8_t* slot, uint32_t slot_bytes, uint32_t pos) {
    z = slot;
    cap = slot_bytes;
    acc = 0;
    cnt = pos & 7u;
    at = pos >> 3;
    in_head = cnt != 0u;
    head = tail = 0;
    head_at = tail_at = kNone;
    ff = 0;
  }
  __device__ __forceinline__ void put(uint32_t v, uint32_t n) {   // n <= 26, cnt < 8 before
    acc = (acc << n) | v;
    cnt += n;
    while (cnt >= 8u) {
      cnt -= 8u;
      const uint32_t b = (uint32_t)(acc >> cnt) & 255u;
      if (in_head) {
        head = b;
        head_at = at;
        in_head = false;
      } else {
        if (at < cap) z[at] = (uint8_t)b;
        ff += b == 255u;
      }
      ++at;
    }
    acc &= 255u;   // only the low cnt < 8 bits are still held
  }
  __device__ void finish() {
    if (cnt == 0u) return;
    const uint32_t b = (uint32_t)(acc << (8u - cnt)) & 255u;
    if (in_head) {   // all of this thread's bits lie inside one byte that another thread owns
      head = b;
      head_at = at;
    } else {
      tail = b;
      tail_at = at;
    }
  }
};

constexpr uint32_t kEmitThreads = 1024;   // a 1080p interval's 720 blocks get a thread each

// grid (MCU rows, frames of the range)
__global__ __launch_bounds__(kEmitThreads) void k_jpg_emit(JpegArgs a) {
  __shared__ uint32_t part[kEmitThreads];
  __shared__ uint32_t head[kEmitThreads], head_at[kEmitThreads];
  const uint32_t tid = threadIdx.x, r = blockIdx.x, f = blockIdx.y;
  const uint32_t nb = a.g.mx * a.g.bpm, bpm = a.g.bpm;
  const uint32_t per = (nb + kEmitThreads - 1u) / kEmitThreads, lo = min(tid * per, nb), hi = min(lo + per, nb);
  const size_t interval = (size_t)f * a.g.my + r, blk0 = interval * nb;
  const int16_t* coef = a.coef + blk0 * 64u;
  const uint32_t* abits = a.abits + blk0;
  const Tables* t = a.tables;
  uint32_t bits = 0;
  for (uint32_t j = lo; j < hi; ++j) {
    const uint32_t k = j % bpm, back = pred_distance(a.sub, k), tb = block_comp(a.sub, k) ? 1u : 0u;
    const int32_t pred = j >= back ? coef[(size_t)(j - back) * 64u] : 0;
    bits += dc_bits(clamp_dc_diff(coef[(size_t)j * 64u] - pred), t->dc[tb]) + abits[j];
  }
  part[tid] = bits;
  __syncthreads();
  for (uint32_t d = 1; d < kEmitThreads; d <<= 1) {
    const uint32_t o = tid >= d ? part[tid - d] : 0u;
    __syncthreads();
    part[tid] += o;
    __syncthreads();
  }
  const uint32_t total = part[kEmitThreads - 1u], nbytes = (total + 7u) >> 3;
  uint8_t* slot = a.zbuf + interval * a.slot;
  SlotBits sb;
  sb.init(slot, a.slot, part[tid] - bits);
  for (uint32_t j = lo; j < hi; ++j) {
    const uint32_t k = j % bpm, back = pred_distance(a.sub, k), tb = block_comp(a.sub, k) ? 1u : 0u;
    const int32_t pred = j >= back ? coef[(size_t)(j - back) * 64u] : 0;
    const int16_t* zz = coef + (size_t)j * 64u;
    block_codes([&](uint32_t i) { return (int32_t)zz[i]; }, clamp_dc_diff(zz[0] - pred), t->dc[tb], t->ac[tb],
                [&](uint32_t v, uint32_t n) { sb.put(v, n); });
  }
  sb.finish();
  __syncthreads();   // part[] has been read
  head[tid] = sb.head;
  head_at[tid] = lo < hi ? sb.head_at : kNone;
  __syncthreads();
  uint32_t ff = sb.ff;
  if (lo < hi && sb.tail_at != kNone) {   // the byte's owner gathers the bits of the threads behind it
    uint32_t b = sb.tail;
    for (uint32_t u = tid + 1u; u < kEmitThreads && head_at[u] == sb.tail_at; ++u) b |= head[u];
    if (sb.tail_at == (total >> 3)) b |= (1u << (8u - (total & 7u))) - 1u;   // the interval's padding
    if (sb.tail_at < a.slot) slot[sb.tail_at] = (uint8_t)b;
    ff += b == 255u;
  }
  __syncthreads();
  part[tid] = ff;
  __syncthreads();
  for (uint32_t d = kEmitThreads / 2u; d > 0; d >>= 1) {
    if (tid < d) part[tid] += part[tid + d];
    __syncthreads();
  }
  if (tid == 0) {
    a.isize[interval] = nbytes;
    a.ipos[interval] = nbytes + part[0];
  }
}

// One workgroup per frame of the range: the intervals' stuffed sizes become their offsets in the file's
// entropy data (the RSTm markers between them included), and their sum gives the file's size.
__global__ __launch_bounds__(256) void k_jpg_layout(JpegArgs a) {
  __shared__ uint64_t part[256];
  const uint32_t tid = threadIdx.x, f = blockIdx.x, my = a.g.my;
  const uint32_t per = (my + 255u) / 256u, lo = min(tid * per, my), hi = min(lo + per, my);
  uint32_t* ipos = a.ipos + (size_t)f * my;
  uint64_t s = 0;
  for (uint32_t r = lo; r < hi; ++r) s += ipos[r] + (r + 1u < my ? 2u : 0u);
  part[tid] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint64_t o = tid >= d ? part[tid - d] : 0ull;
    __syncthreads();
    part[tid] += o;
    __syncthreads();
  }
  // a file's entropy data stays below 2^32 bytes: 8192 x 8192 pixels at 4:4:4 are 3 * 2^20 blocks of at
  // most 2 * 208 stuffed bytes
  uint64_t run = part[tid] - s;
  for (uint32_t r = lo; r < hi; ++r) {
    const uint32_t n = ipos[r];
    ipos[r] = (uint32_t)run;
    run += n + (r + 1u < my ? 2u : 0u);
  }
  if (tid == 255) a.fsize[f] = kHeadBytes + part[255] + 2u;
}

// One workgroup: the range's file offsets, continued from the previous range's last one.  64-bit throughout.
__global__ __launch_bounds__(256) void k_jpg_offsets(JpegArgs a) {
  __shared__ uint64_t part[256];
  const uint32_t tid = threadIdx.x, n = a.n;
  const uint32_t per = (n + 255u) / 256u, lo = min(tid * per, n), hi = min(lo + per, n);
  const uint64_t base = a.first ? a.file_offsets[a.first] : 0ull;
  uint64_t o = 0;
  for (uint32_t i = lo; i < hi; ++i) o += a.fsize[i];
  part[tid] = o;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint64_t v = tid >= d ? part[tid - d] : 0ull;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint64_t run = base + part[tid] - o;
  for (uint32_t i = lo; i < hi; ++i) {
    a.file_offsets[a.first + i] = run;
    run += a.fsize[i];
  }
  if (tid == 255) a.file_offsets[a.first + n] = base + part[255];
}

// grid (MCU rows, frames of the range)
__global__ __launch_bounds__(256) void k_jpg_pack(JpegArgs a) {
  __shared__ uint32_t part[256];
  const uint32_t tid = threadIdx.x, r = blockIdx.x, f = blockIdx.y, my = a.g.my;
  const uint64_t foff = a.file_offsets[a.first + f], fsize = a.fsize[f];
  if (fsize > a.out_capacity || foff > a.out_capacity - fsize) return;   // the file does not fit: none of it is written
  const size_t interval = (size_t)f * my + r;
  const uint32_t nbytes = min(a.isize[interval], a.slot);
  const uint8_t* slot = a.zbuf + interval * a.slot;
  // ByteOut stores whole dwords where its position is a multiple of 4: positions count from the dword
  // at or below `out`, and start at or above `out`
  const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(a.out) & 3u);
  uint8_t* base = a.out - mis;
  const uint64_t file = mis + foff;
  ByteOut o;
  if (r == 0) {   // the header, 4 bytes a thread
    for (uint32_t k = tid * 4u; k < kHeadBytes; k += 1024u) {
      o.init(base, file + k);
      for (uint32_t j = k; j < min(k + 4u, kHeadBytes); ++j) o.put(a.tables->head[j]);
      o.finish();
    }
  }
  // each thread copies a run of whole dwords of the slot; the 0xFF bytes before it shift it
  const uint32_t per = ((nbytes + 255u) / 256u + 3u) & ~3u, lo = min(tid * per, nbytes), hi = min(lo + per, nbytes);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(slot + lo);   // slots are whole dwords, lo a multiple of 4
  uint32_t ff = 0;
  for (uint32_t k = lo; k < hi; k += 4u) {
    const uint32_t v = words[(k - lo) >> 2], nv = min(4u, hi - k);
    for (uint32_t s = 0; s < nv; ++s) ff += ((v >> (8u * s)) & 255u) == 255u;
  }
  part[tid] = ff;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t v = tid >= d ? part[tid - d] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const uint64_t at = file + kHeadBytes + a.ipos[interval];
  o.init(base, at + lo + (part[tid] - ff));
  for (uint32_t k = lo; k < hi; k += 4u) {
    const uint32_t v = words[(k - lo) >> 2], nv = min(4u, hi - k);
    for (uint32_t s = 0; s < nv; ++s) {
      const uint32_t b = (v >> (8u * s)) & 255u;
      o.put(b);
      if (b == 255u) o.put(0u);
    }
  }
  o.finish();
  if (tid == 255) {   // RSTm, or EOI behind the last interval
    o.init(base, at + nbytes + part[255]);
    o.put(255u);
    o.put(r + 1u < my ? 0xD0u + (r & 7u) : 0xD9u);
    o.finish();
  }
}

}  // namespace

void launch_jpeg(const JpegArgs& a, hipStream_t st) {
  const uint32_t strips = (a.g.mx * a.g.mw + kStripPx - 1u) / kStripPx;
  hipLaunchKernelGGL(k_jpg_blocks, dim3(strips, a.g.my, a.n), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_jpg_emit, dim3(a.g.my, a.n), dim3(kEmitThreads), 0, st, a);
  hipLaunchKernelGGL(k_jpg_layout, dim3(a.n), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_jpg_offsets, dim3(1), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_jpg_pack, dim3(a.g.my, a.n), dim3(256), 0, st, a);
}

}  // namespace csg
