// csg_amodal_spans.hip — full-frame amodal object masks as run-length spans for
// csg_amodal_spans: per label, the pixels SOME triangle of the label covers,
// with the depth range and the alpha test but without a depth test (BOP's
// `mask` next to `mask_visib`), as the vertical runs csg_mask_spans makes of the
// visible ids.  The definition is the spec of include/csg_api.h (DESIGN.md
// §13.5), restated by tests/test_amodal_rle.py from the oracle's amodal image.
//
//   k_amodal_plane  per (chunk of an eligible label, frame): ORs the pixels its
//                   triangles cover into the label's bit plane
//   k_aplane_init   the empty value of every amodal_stats entry
//   k_aplane_count  per (64 columns, label, frame): the spans that start in the
//                   wave's columns, and the label's pixel count and box
//   k_span_scan     (csg_spans.hip, as it is) the counts' exclusive scan and span_offsets
//   k_aplane_emit   per (64 columns, label, frame): every span record at its rank
//
// A plane packs 32 rows to a word, word-row major: plane[y >> 5][x], bit y & 31.
// A vertical run is then a run of bits inside a word (continued through bit 31
// into bit 0 of the word below), and a wave that reads 64 adjacent columns of one
// word row reads 256 contiguous bytes.  The accumulate kernel walks a triangle's
// pixel box column by column with the rows inside: a lane gathers up to 32 rows
// of one column in a register and issues ONE device-scope atomicOr per non-zero
// (column, word), never one per hit.  OR is order-free and the spans' positions
// are ranks (label, then column, then row), so the result does not depend on how
// blocks and waves are scheduled.
#include "csg_amodal_spans.h"

#include "csg_raster_math.h"

namespace csg {

namespace {

// ORs `bits` into word (wr, x) of a plane.  The plain read in front may be stale, which only ever shows
// fewer bits: it can cost an atomic, never drop one (the planes are zeroed before the kernel starts).
// Device scope: the blocks of a label run on different XCDs.
#ifndef CSG_AMODAL_COUNT_ATOMICS
#define CSG_AMODAL_COUNT_ATOMICS 0   // 1: a debug build that counts the plane atomics (tools/amodal_rle_cost.py)
#endif
#if CSG_AMODAL_COUNT_ATOMICS
__device__ unsigned long long g_plane_atomics;
#endif

__device__ __forceinline__ void plane_or(uint32_t* plane, uint32_t W, uint32_t x, uint32_t wr, uint32_t bits) {
  uint32_t* g = plane + (size_t)wr * W + x;
  if ((*g & bits) != bits) {
    atomicOr(g, bits);
#if CSG_AMODAL_COUNT_ATOMICS
    atomicAdd(&g_plane_atomics, 1ull);
#endif
  }
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

constexpr uint32_t kAmBand = 256;   // columns of a band: four of the span kernels' column groups
static_assert(kAmQueue == 64, "one wave scans the queue's item counts");

// ---------------------------------------------------------------------------
// k_amodal_plane: grid (item, frame, band), an item being one chunk (<= 256 triangles
// of one instance) of an eligible label with that label's plane -- the host
// builds the item list, so no block discovers its label from device data and
// labels that are not eligible have no block at all.  Thread 0 forms the
// instance's clip rows as k_clip does; the chunk's AABB is culled against the
// frustum with k_setup's test; then one triangle per thread goes through
// k_setup's arithmetic (csg_amodal_tri.inc, shared with k_amodal) and each raster
// sub-triangle's pixel box, which make_rec clipped to the frame, is tested with
// amodal_hit<false>: exact edge functions, 1/W in [1/far, 1/near], alpha test.
// A box of at most kAmSerial pixels is finished by its own lane; a larger one
// (up to the whole frame) is queued in LDS, and the (word row, column) items of
// ALL queued boxes of a round are spread over the block through a prefix sum of
// their counts (a box of 20 x 20 pixels has 20 or 40 items: box after box, most
// of the block would idle), neighbouring threads on neighbouring columns of one
// word row, so the one-atomic-per-word rule holds there too.  A block only
// takes the columns of its band (kAmBand columns of the frame): every pixel box
// is clipped to it, so a triangle that covers the whole frame is shared by
// ceil(W / kAmBand) blocks instead of keeping one block busy while the GPU
// drains (measured), at the price of the triangle setup once
// per band.  A (column, word) still belongs to exactly one block and lane.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_amodal_plane(SceneDev s, AmodalSpanDev a) {
  __shared__ float clipm[12];
  __shared__ AmTri queue[kAmQueue];
  __shared__ uint32_t qn, qpre[kAmQueue + 1];
  const uint32_t f = blockIdx.y, p = a.item_plane[blockIdx.x];
  const FrameDev& fr = a.frames[f];
  const uint32_t set = fr.xform_set;
  if (set >= a.n_sets) return;   // block-uniform: a set the tables do not hold draws nothing
  const Chunk& ch = a.chunks[a.item_chunk[blockIdx.x]];
  const uint32_t inst = ch.inst;
  const int tid = threadIdx.x;
  if (tid == 0) {   // the instance's clip rows, as k_clip forms them
    const float* M = a.models + ((size_t)set * s.n_inst + inst) * 16;
    float m[16], vm[16], c[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) m[q] = M[q];
    mat4_mul(fr.view, m, vm);
    mat4_mul(fr.proj, vm, c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      clipm[q] = c[q];
      clipm[4 + q] = c[4 + q];
      clipm[8 + q] = c[12 + q];
    }
  }
  __syncthreads();
  {   // k_setup's chunk cull: every wave evaluates the 8 corners (lanes 0-7); the block leaves together
    const CullOut o = corner_out(s, ch, clipm, tid & 7);
    const uint64_t m8 = 0xFFull;
    const bool cull = ((__ballot(o.n) & m8) == m8) || ((__ballot(o.f) & m8) == m8) ||
                      ((__ballot(o.l) & m8) == m8) || ((__ballot(o.r) & m8) == m8) ||
                      ((__ballot(o.t) & m8) == m8) || ((__ballot(o.b) & m8) == m8);
    if (cull) return;
  }
  uint32_t* plane = a.planes + ((size_t)f * a.P + p) * a.HW * a.W;
  const uint32_t W = a.W;
  const int32_t band_lo = (int32_t)(blockIdx.z * kAmBand), band_hi = (int32_t)min(blockIdx.z * kAmBand + kAmBand, W);

  // columns [i0, i0 + ni) x rows [j0, j0 + nj): the record's pixel box (inside the frame: make_rec) in the band
#define CSG_AM_COL(v) ((uint32_t)min(max((int32_t)(v), band_lo), band_hi))
#define CSG_AM_ROW(v) ((uint32_t)(v))
#include "csg_amodal_tri.inc"
#undef CSG_AM_COL
#undef CSG_AM_ROW

  bool any = false;
  // rows [ylo, yhi) of column x, all in word row wr: one atomic at most
  auto column_word = [&](const AmTri& t, uint32_t x, uint32_t wr, uint32_t ylo, uint32_t yhi) {
    uint32_t bits = 0u;
#pragma clang loop unroll(disable)
    for (uint32_t y = ylo; y < yhi; ++y) {
      uint32_t key = 0u;
      if (amodal_hit<false>(s, t, (int32_t)x, (int32_t)y, key)) bits |= 1u << (y & 31u);
    }
    if (bits) {
      plane_or(plane, W, x, wr, bits);
      any = true;
    }
  };
  // small boxes: the lane's own loop, column by column
  auto serial = [&](const AmTri& t) {
    const uint32_t yend = t.j0 + t.nj;
#pragma clang loop unroll(disable)
    for (uint32_t ii = 0; ii < t.ni; ++ii) {
#pragma clang loop unroll(disable)
      for (uint32_t y = t.j0; y < yend;) {
        const uint32_t stop = min(yend, (y | 31u) + 1u);
        column_word(t, t.i0 + ii, y >> 5, y, stop);
        y = stop;
      }
    }
  };
  bool p0 = nrec > 0 && t0.ni * t0.nj > kAmSerial, p1 = nrec > 1 && t1.ni * t1.nj > kAmSerial;
  if (nrec > 0 && !p0) serial(t0);
  if (nrec > 1 && !p1) serial(t1);
  // large ones: queued, their (word row, column) items spread over the block (block-uniform loop)
  for (;;) {
    if (tid == 0) qn = 0u;
    __syncthreads();
    if (p0) {
      const uint32_t at = atomicAdd(&qn, 1u);
      if (at < kAmQueue) { queue[at] = t0; p0 = false; }
    }
    if (p1) {
      const uint32_t at = atomicAdd(&qn, 1u);
      if (at < kAmQueue) { queue[at] = t1; p1 = false; }
    }
    __syncthreads();
    const uint32_t n = min(qn, kAmQueue);
    if (tid < 64) {   // the first wave: qpre[e] = items of the boxes before box e
      uint32_t c = 0u;
      if ((uint32_t)tid < n) {
        const AmTri& t = queue[tid];
        c = t.ni * ((((t.j0 + t.nj - 1u) >> 5) - (t.j0 >> 5)) + 1u);   // <= W * ceil(H / 32) < 2^24
      }
      qpre[tid + 1] = wave_inclusive_scan(c, (uint32_t)tid);
      if (tid == 0) qpre[0] = 0u;
    }
    __syncthreads();
    const uint32_t total = qpre[n];
    for (uint32_t q = tid; q < total; q += kBlock) {
      uint32_t e = 0u, hi = n;   // the box of item q: the last e with qpre[e] <= q
#pragma clang loop unroll(disable)
      while (hi - e > 1u) {
        const uint32_t mid = (e + hi) >> 1;
        if (qpre[mid] <= q) e = mid; else hi = mid;
      }
      const AmTri& t = queue[e];
      const uint32_t ni = t.ni, yend = t.j0 + t.nj, wr0 = t.j0 >> 5, local = q - qpre[e];
      const uint32_t rr = local / ni, ii = local - rr * ni, wr = wr0 + rr;
      column_word(t, t.i0 + ii, wr, max(t.j0, wr << 5), min(yend, (wr + 1u) << 5));
    }
    if (!__syncthreads_or((int)(p0 || p1))) break;   // also orders this round's queue reads before the next writes
  }
  // planes no block touched cost the span kernels one word (same value from every block: order-free)
  if (__syncthreads_or((int)any) && tid == 0) atomicOr(&a.touched[(size_t)f * a.P + p], 1u);
}

// the empty value of inst_stats for every (frame, label)
__global__ __launch_bounds__(256) void k_aplane_init(uint32_t* stats, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t* st = stats + (size_t)i * 5;
  st[0] = 0u;
  st[1] = 0xFFFFFFFFu;
  st[2] = 0xFFFFFFFFu;
  st[3] = 0u;
  st[4] = 0u;
}

// span starts of a word: set bits whose neighbour above (bit 31 of the word above for bit 0) is clear
__device__ __forceinline__ uint32_t word_starts(uint32_t w, uint32_t carry) {
  return (uint32_t)__popc(w & ~((w << 1) | carry));
}

// The plane of (frame f, label l), or null when the label is not eligible or no block touched its plane
// (wave-uniform).
__device__ __forceinline__ const uint32_t* live_plane(const AmodalSpanDev& a, uint32_t f, uint32_t l) {
  const uint32_t p = a.plane_of[l];
  if (p == kNoPlane || a.touched[(size_t)f * a.P + p] == 0u) return nullptr;
  return a.planes + ((size_t)f * a.P + p) * a.HW * a.W;
}

// ---------------------------------------------------------------------------
// k_aplane_count: grid (groups, labels, frames), one wave per workgroup; lane =
// column.  cnt[f][l][g] is the layout k_span_scan scans.  The label's pixel
// count and box are reduced over the wave and then into amodal_stats (integer
// add, min and max: order-free).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_aplane_count(AmodalSpanDev a) {
  const uint32_t lane = threadIdx.x, g = blockIdx.x, l = blockIdx.y, f = blockIdx.z;
  uint32_t* cnt = a.cnt + ((size_t)f * a.L + l) * a.G + g;
  const uint32_t* plane = live_plane(a, f, l);
  if (!plane) {
    if (lane == 0) *cnt = 0u;
    return;
  }
  const uint32_t x = g * 64u + lane;
  const bool live = x < a.W;
  const uint32_t* col = plane + (live ? x : 0u);
  uint32_t starts = 0u, px = 0u, carry = 0u, miny = 0xFFFFFFFFu, maxy = 0u;
#pragma unroll 4
  for (uint32_t r = 0; r < a.HW; ++r) {
    const uint32_t w = live ? col[(size_t)r * a.W] : 0u;
    starts += word_starts(w, carry);
    carry = w >> 31;
    px += (uint32_t)__popc(w);
    if (w) {
      miny = min(miny, r * 32u + (uint32_t)__ffs(w) - 1u);
      maxy = r * 32u + 31u - (uint32_t)__clz(w);
    }
  }
  uint32_t minx = px ? x : 0xFFFFFFFFu, maxx = px ? x : 0u;
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    starts += __shfl_xor(starts, off);
    px += __shfl_xor(px, off);
    minx = min(minx, (uint32_t)__shfl_xor(minx, off));
    miny = min(miny, (uint32_t)__shfl_xor(miny, off));
    maxx = max(maxx, (uint32_t)__shfl_xor(maxx, off));
    maxy = max(maxy, (uint32_t)__shfl_xor(maxy, off));
  }
  if (lane == 0) {
    *cnt = starts;
    if (a.stats && px) {
      uint32_t* st = a.stats + ((size_t)f * a.L + l) * 5;
      atomicAdd(&st[0], px);
      atomicMin(&st[1], minx);
      atomicMin(&st[2], miny);
      atomicMax(&st[3], maxx);
      atomicMax(&st[4], maxy);
    }
  }
}

// ---------------------------------------------------------------------------
// k_aplane_emit: the grid of k_aplane_count.  A record's position is
//   first record of (label, group)              -- k_span_scan
//   + spans of the label in lower columns of the group  -- a wave scan
//   + spans higher up in the column                     -- the lane's running count
// which is the spec's order by construction.  Positions at or beyond C are
// dropped (the frame overflowed: its total in the offsets says so), so no store
// leaves the frame's slots.  No atomics, no sort.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_aplane_emit(AmodalSpanDev a) {
  const uint32_t lane = threadIdx.x, g = blockIdx.x, l = blockIdx.y, f = blockIdx.z;
  const uint32_t* plane = live_plane(a, f, l);
  if (!plane) return;
  const uint32_t x = g * 64u + lane, H = a.H, C = a.C;
  const bool live = x < a.W;
  const uint32_t* col = plane + (live ? x : 0u);
  uint32_t starts = 0u, carry = 0u;
#pragma unroll 4
  for (uint32_t r = 0; r < a.HW; ++r) {
    const uint32_t w = live ? col[(size_t)r * a.W] : 0u;
    starts += word_starts(w, carry);
    carry = w >> 31;
  }
  uint32_t pos = a.cnt[((size_t)f * a.L + l) * a.G + g] + wave_inclusive_scan(starts, lane) - starts;
  if (starts == 0u) return;   // (after the scan's shuffles)
  SpanRec* out = a.spans + (size_t)f * C;
  bool open = false;          // a run reached bit 31 of the word above
  uint32_t y0 = 0u;
  for (uint32_t r = 0; r < a.HW; ++r) {
    uint32_t m = col[(size_t)r * a.W];
    const uint32_t y = r * 32u;
    if (open) {
      if (m == 0xFFFFFFFFu) continue;
      const uint32_t ones = (uint32_t)__ffs(~m) - 1u;   // < 32
      if (pos < C) out[pos] = SpanRec{x * H + y0, y + ones - y0};
      ++pos;
      open = false;
      m &= ~((1u << ones) - 1u);
    }
    while (m) {
      const uint32_t s0 = (uint32_t)__ffs(m) - 1u;
      const uint32_t inv = ~(m >> s0);                  // bit 0 clear; zero bits above 32 - s0 read as "end"
      const uint32_t ones = min((uint32_t)__ffs(inv) - 1u, 32u - s0);
      if (s0 + ones == 32u) {
        open = true;
        y0 = y + s0;
        break;
      }
      if (pos < C) out[pos] = SpanRec{x * H + y + s0, ones};
      ++pos;
      m &= ~(((1u << ones) - 1u) << s0);
    }
  }
  if (open && pos < C) out[pos] = SpanRec{x * H + y0, H - y0};   // rows past H are never set: only if H % 32 == 0
}

}  // namespace

#if CSG_AMODAL_COUNT_ATOMICS
// debug builds only: the plane atomics issued since the last reset (synchronises the device)
extern "C" int csg_debug_amodal_atomics(unsigned long long* count, int reset) {
  const unsigned long long zero = 0;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (count && hipMemcpyFromSymbol(count, HIP_SYMBOL(g_plane_atomics), sizeof zero) != hipSuccess) return -1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_plane_atomics), &zero, sizeof zero) != hipSuccess) return -1;
  return 0;
}
#endif

void launch_amodal_spans(const SceneDev& s, const AmodalSpanDev& a, uint32_t n, hipStream_t st) {
  if (a.n_items)
    hipLaunchKernelGGL(k_amodal_plane, dim3(a.n_items, n, (a.W + kAmBand - 1u) / kAmBand), dim3(kBlock), 0, st, s, a);
  if (a.stats) hipLaunchKernelGGL(k_aplane_init, dim3((n * a.L + 255u) / 256u), dim3(256), 0, st, a.stats, n * a.L);
  hipLaunchKernelGGL(k_aplane_count, dim3(a.G, a.L, n), dim3(64), 0, st, a);
  SpanArgs sa{};
  sa.W = a.W;
  sa.H = a.H;
  sa.L = a.L;
  sa.G = a.G;
  sa.C = a.C;
  sa.spans = a.spans;
  sa.offsets = a.offsets;
  sa.cnt = a.cnt;
  launch_span_scan(sa, n, st);
  hipLaunchKernelGGL(k_aplane_emit, dim3(a.G, a.L, n), dim3(64), 0, st, a);
}

}  // namespace csg
