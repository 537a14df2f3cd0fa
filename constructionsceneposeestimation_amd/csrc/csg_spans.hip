// csg_spans.hip — per-object run-length masks for csg_mask_spans: the vertical
// runs ("spans") of every label of an instance image, in COCO's column-major
// order, made from the ids a render wrote without leaving the GPU.  The
// definition is the spec of include/csg_api.h, restated in
// NumPy by tests/test_mask_rle.py.  Integer arithmetic only.
//
//   k_span_count  per (frame, group of 64 columns): the spans of each label
//   k_span_scan   per frame: the exclusive scan of those counts, label-major,
//                 which is each (label, group)'s first record, and span_offsets
//   k_span_emit   per (frame, group): every span record at its final position
//
// A wave owns 64 adjacent columns and walks down the rows, so each step reads
// one contiguous 256-byte row segment; a lane compares its id with the id above
// to find where spans start and end.  What a lane knows about its column lives
// in an LDS table tab[label][lane] that only that lane touches (no barriers, no
// atomics, stride-1 across lanes: no bank conflicts).  A record's position is
//   first record of (label, group)             -- k_span_scan
//   + spans of the label in lower columns of the group  -- a wave scan of the table
//   + spans of the label higher up in the column        -- the running table entry
// which is the spec's order (label, then start = x * H + y0) by construction:
// the result does not depend on how waves are scheduled.
#include "csg_spans.h"

namespace csg {

namespace {

constexpr uint32_t kSpanRows = 8;   // rows a lane loads before it looks at them (loads in flight)

// Walks the lane's column.  tab[l * 64 + lane] is the lane's running entry of
// label l: every span start reads it (the span's position when kEmit) and adds
// one.  Ids outside [0, L) belong to no label and never index the table.
template <bool kEmit>
__device__ __forceinline__ void span_walk(const SpanArgs& a, const int32_t* __restrict__ col, bool live, uint32_t x,
                                          uint32_t lane, uint32_t* tab, SpanRec* out) {
  const uint32_t H = a.H, W = a.W, L = a.L, C = a.C;
  int32_t prev = -1;
  uint32_t y0 = 0, pos = 0;
  for (uint32_t yb = 0; yb < H; yb += kSpanRows) {
    int32_t v[kSpanRows];
#pragma unroll
    for (uint32_t t = 0; t < kSpanRows; ++t) v[t] = (live && yb + t < H) ? col[(size_t)(yb + t) * W] : -1;
#pragma unroll
    for (uint32_t t = 0; t < kSpanRows; ++t) {
      const uint32_t y = yb + t;
      if (y >= H) break;   // wave-uniform
      const int32_t cur = (uint32_t)v[t] < L ? v[t] : -1;
      if (cur != prev) {
        if (kEmit && prev >= 0 && pos < C) out[pos] = SpanRec{x * H + y0, y - y0};
        if (cur >= 0) {
          uint32_t* e = tab + (uint32_t)cur * 64u + lane;
          pos = *e;
          *e = pos + 1u;
          y0 = y;
        }
        prev = cur;
      }
    }
  }
  if (kEmit && prev >= 0 && pos < C) out[pos] = SpanRec{x * H + y0, H - y0};
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

// grid (groups, frames), one wave per workgroup, L * 256 bytes of dynamic LDS
__global__ __launch_bounds__(64) void k_span_count(SpanArgs a, uint32_t f0) {
  extern __shared__ __attribute__((aligned(16))) uint32_t span_tab[];
  const uint32_t lane = threadIdx.x, g = blockIdx.x, f = f0 + blockIdx.y;
  const uint32_t x = g * 64u + lane;
  const bool live = x < a.W;
  for (uint32_t l = 0; l < a.L; ++l) span_tab[l * 64u + lane] = 0u;
  span_walk<false>(a, a.instance + (size_t)f * a.H * a.W + (live ? x : 0u), live, x, lane, span_tab, nullptr);
  uint32_t* cnt = a.cnt + (size_t)f * a.L * a.G + g;
  for (uint32_t l = 0; l < a.L; ++l) {
    uint32_t v = span_tab[l * 64u + lane];
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) cnt[(size_t)l * a.G] = v;
  }
}

// One workgroup per frame: the counts [L][G] become their exclusive scan in
// place (a span total is at most W * H / 2 <= 2^25), offsets[l] is the scan at
// (l, group 0) and offsets[L] the total.  A thread owns a contiguous piece.
__global__ __launch_bounds__(256) void k_span_scan(SpanArgs a) {
  __shared__ uint32_t part[256];
  const uint32_t tid = threadIdx.x, f = blockIdx.x;
  const uint32_t M = a.L * a.G, per = (M + 255u) / 256u;
  const uint32_t lo = min(tid * per, M), hi = min(lo + per, M);
  uint32_t* c = a.cnt + (size_t)f * M;
  uint32_t* off = a.offsets + (size_t)f * (a.L + 1u);
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; ++i) s += c[i];
  part[tid] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t o = tid >= d ? part[tid - d] : 0u;
    __syncthreads();
    part[tid] += o;
    __syncthreads();
  }
  uint32_t run = part[tid] - s;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t v = c[i];
    c[i] = run;
    if (i % a.G == 0) off[i / a.G] = run;
    run += v;
  }
  if (tid == 255) off[a.L] = part[255];
}

// grid (groups, frames), as k_span_count: counts again into the table, turns
// each entry into the lane's first position of that label, and walks a second
// time writing the records.  Positions at or beyond C are dropped (the frame
// overflowed: its total in offsets says so), so no store leaves the frame's slots.
__global__ __launch_bounds__(64) void k_span_emit(SpanArgs a, uint32_t f0) {
  extern __shared__ __attribute__((aligned(16))) uint32_t span_tab[];
  const uint32_t lane = threadIdx.x, g = blockIdx.x, f = f0 + blockIdx.y;
  const uint32_t x = g * 64u + lane;
  const bool live = x < a.W;
  const int32_t* col = a.instance + (size_t)f * a.H * a.W + (live ? x : 0u);
  for (uint32_t l = 0; l < a.L; ++l) span_tab[l * 64u + lane] = 0u;
  span_walk<false>(a, col, live, x, lane, span_tab, nullptr);
  const uint32_t* base = a.cnt + (size_t)f * a.L * a.G + g;
  for (uint32_t l = 0; l < a.L; ++l) {
    const uint32_t v = span_tab[l * 64u + lane];
    if (__ballot(v != 0u) == 0ull) continue;   // wave-uniform: no lane will look this label up
    span_tab[l * 64u + lane] = base[(size_t)l * a.G] + wave_inclusive_scan(v, lane) - v;
  }
  span_walk<true>(a, col, live, x, lane, span_tab, a.spans + (size_t)f * a.C);
}

}  // namespace

void launch_span_count(const SpanArgs& a, uint32_t n, hipStream_t st) {
  for (uint32_t f0 = 0; f0 < n; f0 += 65535u) {   // grid y limit
    const uint32_t nf = n - f0 < 65535u ? n - f0 : 65535u;
    hipLaunchKernelGGL(k_span_count, dim3(a.G, nf), dim3(64), a.L * 256u, st, a, f0);
  }
}

void launch_span_scan(const SpanArgs& a, uint32_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_span_scan, dim3(n), dim3(256), 0, st, a);
}

void launch_span_emit(const SpanArgs& a, uint32_t n, hipStream_t st) {
  for (uint32_t f0 = 0; f0 < n; f0 += 65535u) {   // grid y limit
    const uint32_t nf = n - f0 < 65535u ? n - f0 : 65535u;
    hipLaunchKernelGGL(k_span_emit, dim3(a.G, nf), dim3(64), a.L * 256u, st, a, f0);
  }
}

}  // namespace csg
