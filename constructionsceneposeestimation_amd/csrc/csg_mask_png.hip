// csg_mask_png.hip — per-object mask PNGs for csg_encode_span_masks: the run-length spans of
// csg_mask_spans / csg_amodal_spans become finished 8-bit grey PNG files without leaving the GPU.  The
// file format is csg_mask_png.h's, restated in Python by writers.mask_png_bytes.
// Integer arithmetic only.
//
//   k_mp_paint    per (item, 64 columns): the label's vertical spans transposed into a bit plane
//   k_mp_rows     per (item, row): the row's token bits and Adler-32 terms
//   k_mp_layout   per item: row bit positions (block scan), stream and file size, Adler-32
//   k_mp_offsets  the range's staging offsets, and file_offsets continued in 64 bits
//   k_mp_zero     zeroes the staging the range uses
//   k_mp_emit     per (item, row): the row's tokens at its bit position; row 0 adds header and Adler-32
//   k_mp_pack     per (item, IDAT chunk): chunk framing and CRC-32 into the file; signature, IHDR, IEND
//
// The plane is stored word-column-major, planes[item][k][y] = pixels 32k .. 32k + 31 of row y: the
// painter, whose wave owns 64 columns and walks down the rows, keeps each row's ballot in the lane of
// that row and stores 64 rows at once, and the row kernels, one thread per row, read word k of 64
// adjacent rows in one access.  Every plane word is written, so the plane needs no memset and is a pure
// function of the input.
//
// Bounds.  Span records are read only below min(off, C) of the item's frame; a record is used only when
// it lies whole inside its column.  Staging stores stay inside an item's [zoff, zoff + zbytes rounded up
// to 4), which is checked against the staging's size; file stores stay inside [foff, foff + fsize),
// which is checked against out_capacity.  An item that fails either check is not written at all.
#include "csg_mask_png.h"

#include <algorithm>

#include "csg_bitio.h"
#include "csg_spans.h"

namespace csg {

using namespace dfl;
using namespace mpng;

namespace {

__device__ __forceinline__ uint32_t round4(uint32_t v) { return (v + 3u) & ~3u; }

// grid (G, items of the range), one wave per workgroup
__global__ __launch_bounds__(64) void k_mp_paint(MaskPngArgs a) {
  const uint32_t lane = threadIdx.x, g = blockIdx.x, i = blockIdx.y, H = a.H;
  const MaskItem it = a.items[a.first + i];
  const uint32_t x = g * 64u + lane, key = x * H, col_end = key + H;   // < 2^27
  const uint32_t* off = a.offsets + (size_t)it.frame * (a.L + 1u);
  const SpanRec* rec = a.spans + (size_t)it.frame * a.C;
  const uint32_t lo = min(off[it.label], a.C);
  const uint32_t hi = x < a.W ? max(min(off[it.label + 1u], a.C), lo) : lo;
  uint32_t r = lo, q = hi;   // the first record at or behind the column's first pixel
  while (r < q) {
    const uint32_t m = (r + q) >> 1;
    if (rec[m].start < key) r = m + 1u;
    else q = m;
  }
  uint32_t* w0 = a.planes + ((size_t)i * a.KW + 2u * g) * H;
  uint32_t* w1 = w0 + H;
  const bool any = r < hi && rec[r].start < col_end;
  if (__ballot(any) == 0ull) {   // wave-uniform: none of the 64 columns has a span
    for (uint32_t y = lane; y < H; y += 64u) {
      w0[y] = 0u;
      w1[y] = 0u;
    }
    return;
  }
  uint32_t end = 0;            // the column's pixels from the last record's first row to end - 1 are set
  uint32_t keep0 = 0, keep1 = 0;
  SpanRec s = r < hi ? rec[r] : SpanRec{col_end, 0u};   // the next record, loaded once
  for (uint32_t y = 0; y < H; ++y) {
    while (s.start < col_end) {   // take in the column's records that start at or above row y
      const uint32_t y0 = s.start - key;
      if (s.start >= key && y0 > y) break;
      if (s.start >= key && s.len != 0u && s.len <= H - y0) end = max(end, y0 + s.len);
      ++r;
      s = r < hi ? rec[r] : SpanRec{col_end, 0u};
    }
    const unsigned long long row = __ballot(y < end);
    if ((y & 63u) == lane) {
      keep0 = (uint32_t)row;
      keep1 = (uint32_t)(row >> 32);
    }
    if ((y & 63u) == 63u || y == H - 1u) {   // wave-uniform: the lanes store the rows they kept
      const uint32_t yr = (y & ~63u) + lane;
      if (yr <= y) {
        w0[yr] = keep0;
        w1[yr] = keep1;
      }
    }
  }
}

// grid (ceil(H / 256), items of the range)
__global__ __launch_bounds__(256) void k_mp_rows(MaskPngArgs a) {
  const uint32_t y = blockIdx.x * 256u + threadIdx.x, i = blockIdx.y, H = a.H;
  if (y >= H) return;
  const uint32_t* p = a.planes + (size_t)i * a.KW * H + y;
  const RowSums s = row_sums(a.W, H, y, [&](uint32_t k) { return p[(size_t)k * H]; });
  const size_t at = (size_t)i * H + y, plane = (size_t)a.n * H;
  a.rows[at] = s.bits;
  a.rows[plane + at] = s.a;
  a.rows[2u * plane + at] = s.b;
}

// One workgroup per item: the rows' bit counts become their bit positions in the stream (8192 rows of
// at most 9 * 8193 bits: below 2^30), and the sums give the stream's size and Adler-32.
__global__ __launch_bounds__(256) void k_mp_layout(MaskPngArgs a) {
  __shared__ uint32_t part[256];
  __shared__ uint32_t sum_a[256], sum_b[256];
  const uint32_t tid = threadIdx.x, i = blockIdx.x, H = a.H;
  const uint32_t per = (H + 255u) / 256u, lo = min(tid * per, H), hi = min(lo + per, H);
  const size_t plane = (size_t)a.n * H;
  uint32_t* bits = a.rows + (size_t)i * H;
  uint32_t s = 0, sa = 0, sb = 0;   // at most 32 rows per thread: sums of residues stay below 2^21
  for (uint32_t y = lo; y < hi; ++y) {
    s += bits[y];
    sa += bits[plane + y];
    sb += bits[2u * plane + y];
  }
  part[tid] = s;
  sum_a[tid] = sa;
  sum_b[tid] = sb;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t o = tid >= d ? part[tid - d] : 0u;
    const uint32_t oa = tid >= d ? sum_a[tid - d] : 0u, ob = tid >= d ? sum_b[tid - d] : 0u;
    __syncthreads();
    part[tid] += o;
    sum_a[tid] = (sum_a[tid] + oa) % kAdlerMod;
    sum_b[tid] = (sum_b[tid] + ob) % kAdlerMod;
    __syncthreads();
  }
  uint32_t run = kHeadBits + part[tid] - s;
  for (uint32_t y = lo; y < hi; ++y) {
    const uint32_t v = bits[y];
    bits[y] = run;
    run += v;
  }
  if (tid == 255) {
    MaskFile f;
    f.zbytes = zlib_bytes(part[255]);
    f.fsize = file_bytes(f.zbytes);
    f.zoff = 0;
    f.adler = stream_adler(a.W, H, sum_a[255], sum_b[255]);
    a.files[i] = f;
  }
}

// One workgroup: where each stream of the range starts in the staging (files[n].zoff is their total), and
// the range's file offsets, continued from the previous range's last one.  64-bit throughout.
__global__ __launch_bounds__(256) void k_mp_offsets(MaskPngArgs a) {
  __shared__ uint64_t part_z[256], part_o[256];
  const uint32_t tid = threadIdx.x, n = a.n;
  const uint32_t per = (n + 255u) / 256u, lo = min(tid * per, n), hi = min(lo + per, n);
  const uint64_t base = a.first ? a.file_offsets[a.first] : 0ull;
  uint64_t z = 0, o = 0;
  for (uint32_t i = lo; i < hi; ++i) {
    z += round4(a.files[i].zbytes);
    o += a.files[i].fsize;
  }
  part_z[tid] = z;
  part_o[tid] = o;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint64_t vz = tid >= d ? part_z[tid - d] : 0ull, vo = tid >= d ? part_o[tid - d] : 0ull;
    __syncthreads();
    part_z[tid] += vz;
    part_o[tid] += vo;
    __syncthreads();
  }
  uint64_t rz = part_z[tid] - z, ro = base + part_o[tid] - o;
  for (uint32_t i = lo; i < hi; ++i) {
    a.file_offsets[a.first + i] = ro;
    a.files[i].zoff = rz;
    ro += a.files[i].fsize;
    rz += round4(a.files[i].zbytes);
  }
  if (tid == 255) {
    a.file_offsets[a.first + n] = base + part_o[255];
    a.files[n].zoff = part_z[255];
  }
}

__global__ __launch_bounds__(256) void k_mp_zero(MaskPngArgs a) {
  const uint64_t n16 = min((a.files[a.n].zoff + 15ull) / 16ull, a.zcap / 16ull);
  uint4* z = reinterpret_cast<uint4*>(a.zbuf);
  for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < n16; k += (uint64_t)gridDim.x * 256u)
    z[k] = make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ bool staging_holds(const MaskPngArgs& a, const MaskFile& f) {
  return f.zoff + round4(f.zbytes) <= a.zcap;
}

// grid (ceil(H / 256), items of the range)
__global__ __launch_bounds__(256) void k_mp_emit(MaskPngArgs a) {
  const uint32_t y = blockIdx.x * 256u + threadIdx.x, i = blockIdx.y, H = a.H;
  const MaskFile f = a.files[i];
  if (y >= H || !staging_holds(a, f)) return;
  uint32_t* words = reinterpret_cast<uint32_t*>(a.zbuf + f.zoff);
  const uint32_t* p = a.planes + (size_t)i * a.KW * H + y;
  WordBits wb;
  wb.init(words, a.rows[(size_t)i * H + y]);
  row_runs(a.W, [&](uint32_t k) { return p[(size_t)k * H]; },
           [&](uint32_t b, uint32_t, uint32_t len) { run_emit(b, len, [&](uint32_t v, uint32_t nb) { wb.put(v, nb); }); });
  wb.finish();
  if (y == 0) {   // the stream's first 19 bits, and its Adler-32 (big-endian) behind the padding
    atomicOr(&words[0], kHeadWord);
    const uint32_t at = f.zbytes - 4u;
    const uint64_t sv = (uint64_t)__builtin_bswap32(f.adler) << (8u * (at & 3u));
    atomicOr(&words[at >> 2], (uint32_t)sv);
    if (at & 3u) atomicOr(&words[(at >> 2) + 1u], (uint32_t)(sv >> 32));
  }
}

// grid (chunk blocks, items of the range): one thread per IDAT chunk, striding over the item's chunks
__global__ __launch_bounds__(64) void k_mp_pack(MaskPngArgs a) {
  __shared__ uint32_t T[256];
  for (uint32_t k = threadIdx.x; k < 256u; k += 64) T[k] = crc_entry(k);
  __syncthreads();
  const uint32_t i = blockIdx.y;
  const MaskFile f = a.files[i];
  const uint64_t foff = a.file_offsets[a.first + i];
  if (!staging_holds(a, f) || foff + f.fsize > a.out_capacity) return;
  // ByteOut stores whole dwords where its position is a multiple of 4: positions count from the dword
  // at or below `out`, and start at or above `out`
  const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(a.out) & 3u);
  uint8_t* base = a.out - mis;
  const uint64_t file = mis + foff;
  const uint32_t zb = f.zbytes, nch = idat_chunks(zb);
  for (uint32_t ch = blockIdx.x * 64u + threadIdx.x; ch < nch; ch += gridDim.x * 64u) {
    const uint32_t n = min(kIdatBytes, zb - ch * kIdatBytes);
    ByteOut o;
    if (ch == 0) {   // signature + IHDR
      o.init(base, file);
      const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
      for (int k = 0; k < 8; ++k) o.put(sig[k]);
      o.be32(13u);
      Crc c{T, 0xFFFFFFFFu};
      for (uint32_t k = 0; k < 17u; ++k) {
        const uint32_t b = ihdr_byte(k, a.W, a.H);
        o.put(b);
        c.add(b);
      }
      o.be32(c.c ^ 0xFFFFFFFFu);
      o.finish();
    }
    o.init(base, file + kSigIhdrBytes + (uint64_t)ch * (kIdatBytes + 12u));
    o.be32(n);
    Crc c{T, 0xFFFFFFFFu};
    const uint8_t idat[4] = {'I', 'D', 'A', 'T'};
    for (int k = 0; k < 4; ++k) {
      o.put(idat[k]);
      c.add(idat[k]);
    }
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.zbuf + f.zoff + (size_t)ch * kIdatBytes);
    const uint32_t nw = (n + 3u) >> 2;   // the stream's last word is whole in the staging
    for (uint32_t k = 0; k < nw; ++k) {
      const uint32_t v = src[k], nb = min(4u, n - 4u * k);
      for (uint32_t s = 0; s < nb; ++s) {
        const uint32_t b = (v >> (8u * s)) & 255u;
        o.put(b);
        c.add(b);
      }
    }
    o.be32(c.c ^ 0xFFFFFFFFu);
    if (ch == nch - 1u) {   // IEND
      o.be32(0u);
      const uint8_t iend[8] = {'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
      for (int k = 0; k < 8; ++k) o.put(iend[k]);
    }
    o.finish();
  }
}

}  // namespace

void launch_mask_png(const MaskPngArgs& a, hipStream_t st) {
  const uint32_t row_blocks = (a.H + 255u) / 256u;
  const uint32_t chunk_blocks = std::min(64u, (idat_chunks(max_zlib_bytes(a.W, a.H)) + 63u) / 64u);
  hipLaunchKernelGGL(k_mp_paint, dim3(a.KW / 2u, a.n), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_mp_rows, dim3(row_blocks, a.n), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_mp_layout, dim3(a.n), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_mp_offsets, dim3(1), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_mp_zero, dim3(512), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_mp_emit, dim3(row_blocks, a.n), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_mp_pack, dim3(chunk_blocks, a.n), dim3(64), 0, st, a);
}

}  // namespace csg
