// csg_voxels.hip — voxel-downsampled labelled point clouds for csg_voxel_cloud: the points a render
// wrote, binned on a world-fixed grid per (cell, id), as one record per voxel (centroid, mean colour,
// label, count), without leaving the GPU.  The definition is the spec of include/csg_api.h (DESIGN.md
// §13.10), restated in NumPy by tests/test_voxel_cloud.py.  Everything summed is an integer, and a
// voxel's place in the output is the rank of its lowest pixel: no result depends on scheduling or on
// the hash.
//
//   k_vx_init    per slot and bitmap word of the range: the empty table, zero sums, zero counters
//   k_vx_insert  per pixel: key; find or claim the key's slot (64-bit compare-and-swap, linear probing);
//                atomicMin of the pixel index, integer atomic adds of n, S and R into the slot (the six
//                64-bit sums of eight slots in one wave instruction, a lane per sum)
//   k_vx_mark    per slot: the bit of the voxel's lowest pixel in the frame's bitmap
//   k_vx_scan    per frame: set bits before every bitmap word; V; vx_total and vx_dropped
//   k_vx_emit    per slot: rank = set bits below the voxel's lowest pixel; the record.  Per row >= V: the fill
//
// A wave holds 64 consecutive row-major pixels, which mostly share a voxel.  With `combine` the lanes
// of a run of equal keys sum their contributions in registers (a segmented scan over the ballot of
// "key differs from the lane below") and the run's last lane issues the atomics once.
//
// Overflow.  A workgroup counts the empty slots its threads claim and adds the count to the frame's at
// its end; the add that makes the frame's count pass Ceff sets the frame's flag, and a probe looks at
// the flag at its first step and every eighth.  A frame that fits claims at most Ceff <= T / 2 slots,
// so each of its probes meets its key or an empty slot.  Only a frame with more than Ceff voxels can
// fill its table; there a probe ends at the flag or after T steps at the latest, and sets the flag.
#include "csg_voxels.h"

namespace csg {

namespace {

constexpr uint32_t kVxBlock = 256;
constexpr uint32_t kVxScanBlock = 1024;

__device__ __forceinline__ uint32_t vx_hash(uint64_t k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}

__device__ __forceinline__ uint32_t vx_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t vx_load(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(max(T, BW) / 256), n)
__global__ __launch_bounds__(kVxBlock) void k_vx_init(VoxelArgs a) {
  const uint32_t f = blockIdx.y, i = blockIdx.x * kVxBlock + threadIdx.x;
  if (i < a.T) {
    VxSlot e{};
    e.key = kVxEmpty;
    e.minpix = 0xFFFFFFFFu;
    a.slots[(size_t)f * a.T + i] = e;
  }
  if (i < a.BW) a.bitmap[(size_t)f * a.BW + i] = 0u;
  if (i == 0) a.frames[f] = VxFrame{0u, 0u, 0u, 0u};
}

// One axis of a point: t = fl32(p * r), c = floorf(t); false when the point is dropped.
__device__ __forceinline__ bool vx_axis(float p, float r, uint32_t* cell, uint32_t* q) {
  const float t = p * r;
  const float c = floorf(t);
  if (!__builtin_isfinite(t) || !(c >= -131072.0f) || !(c < 131072.0f)) return false;
  *cell = (uint32_t)((int32_t)c + 131072);       // 18 bits
  // t - c is exact and in [0, 1) but for t in (-0.5, 0), where t + 1 rounds (up to 1.0 above -2^-25): the clamp
  *q = min((uint32_t)((t - c) * 65536.0f), 65535u);
  return true;
}

// grid (ceil(P / 256), n): a lane per pixel, a wave per 64 consecutive pixels
template <bool kCombine>
__global__ __launch_bounds__(kVxBlock) void k_vx_insert(VoxelArgs a) {
  const uint32_t f = blockIdx.y, p = blockIdx.x * kVxBlock + threadIdx.x, lane = threadIdx.x & 63u;
  VxFrame* fr = a.frames + f;
  __shared__ uint32_t blk_claims;   // slots this workgroup claimed
  if (threadIdx.x == 0) blk_claims = 0u;
  __syncthreads();
  uint64_t key = kVxEmpty;
  uint32_t q0 = 0, q1 = 0, q2 = 0, r0 = 0, r1 = 0, r2 = 0;
  bool dropped = false;
  if (p < a.P) {
    const size_t gp = (size_t)(a.first + f) * a.P + p;
    const float x = a.points[gp * 3u], y = a.points[gp * 3u + 1u], z = a.points[gp * 3u + 2u];
    const int32_t id = a.instance ? a.instance[gp] : -1;
    if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z) && id >= -1 && id < (int32_t)a.L) {
      uint32_t c0, c1, c2;
      const bool in0 = vx_axis(x, a.r, &c0, &q0), in1 = vx_axis(y, a.r, &c1, &q1), in2 = vx_axis(z, a.r, &c2, &q2);
      if (in0 && in1 && in2) {
        key = (uint64_t)c0 << 45 | (uint64_t)c1 << 27 | (uint64_t)c2 << 9 | (uint64_t)(uint32_t)(id + 1);
        if (a.rgb) r0 = a.rgb[gp * 3u], r1 = a.rgb[gp * 3u + 1u], r2 = a.rgb[gp * 3u + 2u];
      } else {
        dropped = true;
      }
    }
  }
  const uint64_t db = __ballot(dropped);   // exact whether or not the frame overflows
  if (db && lane == 0) atomicAdd(&fr->dropped, (uint32_t)__popcll(db));
  uint32_t n = key != kVxEmpty ? 1u : 0u, minp = p;
  if (kCombine) {
    // runs of equal keys: a run of at most 64 lanes sums to q < 2^22, n < 2^7, colour < 2^14
    const uint64_t lower = __shfl_up(key, 1);
    const uint64_t heads = __ballot(lane == 0 || lower != key);
    const uint32_t hl = 63u - (uint32_t)__builtin_clzll(heads & ((2ull << lane) - 1ull));   // my run's first lane
    uint32_t w0 = q0 | n << 22, w1 = q1, w2 = q2, w3 = r0 | r1 << 16, w4 = r2;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t u0 = __shfl_up(w0, d), u1 = __shfl_up(w1, d), u2 = __shfl_up(w2, d), u3 = __shfl_up(w3, d),
                     u4 = __shfl_up(w4, d);
      if (lane >= hl + d) w0 += u0, w1 += u1, w2 += u2, w3 += u3, w4 += u4;
    }
    const bool tail = lane == 63u || (heads >> (lane + 1u) & 1ull);
    if (!tail) key = kVxEmpty;   // the run's last lane carries the run
    q0 = w0 & 0x3FFFFFu, n = w0 >> 22, q1 = w1, q2 = w2, r0 = w3 & 0xFFFFu, r1 = w3 >> 16, r2 = w4;
    minp = p - (lane - hl);
  }
  bool claimed = false, lost = false;
  VxSlot* found = nullptr;   // the slot of this lane's run
  if (key != kVxEmpty) {
    VxSlot* tab = a.slots + (size_t)f * a.T;
    const uint32_t mask = a.T - 1u;
    uint32_t h = vx_hash(key) & mask;
    VxSlot* s = nullptr;
    for (uint32_t i = 0; i < a.T; ++i, h = (h + 1u) & mask) {   // at most T steps, whatever the table holds
      if ((i & 7u) == 0u && vx_load(&fr->overflow)) break;
      uint64_t k = vx_load(&tab[h].key);
      if (k == kVxEmpty) {
        k = atomicCAS(reinterpret_cast<unsigned long long*>(&tab[h].key), kVxEmpty, key);
        if (k == kVxEmpty) claimed = true, k = key;
      }
      if (k == key) {
        s = &tab[h];
        break;
      }
    }
    if (s) {
      atomicMin(&s->minpix, minp);
      atomicAdd(&s->n, n);
      found = s;
    } else {
      lost = true;   // the flag was seen, or the table is full: more than Ceff voxels either way
    }
  }
  // The six 64-bit sums of a slot are 48 contiguous bytes: eight slots a turn, a lane per sum, so one
  // wave instruction carries a slot's adds to its line instead of six instructions a line each.
  {
    const uint32_t sub = lane >> 3, w = lane & 7u, words = a.rgb ? 6u : 3u;
    const uint32_t plo = (uint32_t)reinterpret_cast<uintptr_t>(found), phi = (uint32_t)(reinterpret_cast<uintptr_t>(found) >> 32);
    uint64_t todo = __ballot(found != nullptr);
    while (todo) {   // wave-uniform
      int src = -1;
#pragma unroll
      for (uint32_t k = 0; k < 8u; ++k) {
        if (todo) {
          const int l = __ffsll((unsigned long long)todo) - 1;
          todo &= todo - 1ull;
          if (sub == k) src = l;
        }
      }
      const int from = src < 0 ? (int)lane : src;
      const uint32_t lo = __shfl(plo, from), hi = __shfl(phi, from);
      const uint32_t v0 = __shfl(q0, from), v1 = __shfl(q1, from), v2 = __shfl(q2, from), v3 = __shfl(r0, from),
                     v4 = __shfl(r1, from), v5 = __shfl(r2, from);
      const uint32_t v = w == 0u ? v0 : w == 1u ? v1 : w == 2u ? v2 : w == 3u ? v3 : w == 4u ? v4 : v5;
      if (src >= 0 && w < words) {
        VxSlot* slot = reinterpret_cast<VxSlot*>((uintptr_t)hi << 32 | (uintptr_t)lo);
        unsigned long long* sum = reinterpret_cast<unsigned long long*>(w < 3u ? &slot->S[w] : &slot->R[w - 3u]);
        atomicAdd(sum, (unsigned long long)v);
      }
    }
  }
  // The frame's claims are counted once per workgroup (one counter per frame: an atomic per claim
  // serialises on its address), the flag is set by the add that passes Ceff or by a lost point.
  const uint64_t cb = __ballot(claimed), lb = __ballot(lost);
  if (cb && lane == (uint32_t)__ffsll((unsigned long long)cb) - 1u) atomicAdd(&blk_claims, (uint32_t)__popcll(cb));
  if (lb && lane == (uint32_t)__ffsll((unsigned long long)lb) - 1u) atomicExch(&fr->overflow, 1u);
  __syncthreads();
  if (threadIdx.x == 0 && blk_claims) {
    if (atomicAdd(&fr->claimed, blk_claims) + blk_claims > a.Ceff) atomicExch(&fr->overflow, 1u);
  }
}

// grid (ceil(T / 256), n)
__global__ __launch_bounds__(kVxBlock) void k_vx_mark(VoxelArgs a) {
  const uint32_t f = blockIdx.y, i = blockIdx.x * kVxBlock + threadIdx.x;
  if (i >= a.T || a.frames[f].overflow) return;
  const VxSlot& s = a.slots[(size_t)f * a.T + i];
  if (s.key == kVxEmpty || s.minpix >= a.P) return;
  atomicOr(&a.bitmap[(size_t)f * a.BW + (s.minpix >> 5)], 1u << (s.minpix & 31u));
}

// grid (n), 1,024 threads: the exclusive scan of the bitmap words' set bits, the frame's V, vx_total and
// vx_dropped.  A thread owns a contiguous piece of the words; its loads do not depend on each other.
__global__ __launch_bounds__(kVxScanBlock) void k_vx_scan(VoxelArgs a) {
  __shared__ uint32_t part[kVxScanBlock];
  const uint32_t f = blockIdx.x, tid = threadIdx.x;
  const uint32_t* __restrict__ bm = a.bitmap + (size_t)f * a.BW;
  uint32_t* __restrict__ wp = a.wprefix + (size_t)f * a.BW;
  const uint32_t per = (a.BW + kVxScanBlock - 1u) / kVxScanBlock;
  const uint32_t lo = min(tid * per, a.BW), hi = min(lo + per, a.BW);
  uint32_t sum = 0;
#pragma unroll 8
  for (uint32_t i = lo; i < hi; ++i) sum += (uint32_t)__popc(bm[i]);
  part[tid] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < kVxScanBlock; d <<= 1) {
    const uint32_t o = tid >= d ? part[tid - d] : 0u;
    __syncthreads();
    part[tid] += o;
    __syncthreads();
  }
  uint32_t first = part[tid] - sum;
#pragma unroll 8
  for (uint32_t i = lo; i < hi; ++i) {
    wp[i] = first;
    first += (uint32_t)__popc(bm[i]);
  }
  if (tid == 0) {
    VxFrame* fr = a.frames + f;
    const uint32_t V = part[kVxScanBlock - 1u];
    fr->V = V;
    a.vx_total[a.first + f] = fr->overflow ? 0xFFFFFFFFu : V;
    if (a.vx_dropped) a.vx_dropped[a.first + f] = fr->dropped;
  }
}

// grid (ceil(max(T, C) / 256), n): thread i finishes slot i and fills row i
__global__ __launch_bounds__(kVxBlock) void k_vx_emit(VoxelArgs a) {
  const uint32_t f = blockIdx.y, i = blockIdx.x * kVxBlock + threadIdx.x;
  const VxFrame fr = a.frames[f];
  if (fr.overflow) return;   // the frame's rows are unspecified
  const size_t row0 = (size_t)(a.first + f) * a.C;
  if (i >= fr.V && i < a.C) {
    const size_t o = row0 + i;
    if (a.vx_xyz) {
      const float nan = __uint_as_float(0x7FC00000u);
      a.vx_xyz[o * 3u] = nan, a.vx_xyz[o * 3u + 1u] = nan, a.vx_xyz[o * 3u + 2u] = nan;
    }
    if (a.vx_rgb) a.vx_rgb[o * 3u] = 0, a.vx_rgb[o * 3u + 1u] = 0, a.vx_rgb[o * 3u + 2u] = 0;
    if (a.vx_label) a.vx_label[o] = -1;
    if (a.vx_count) a.vx_count[o] = 0u;
  }
  if (i >= a.T) return;
  const VxSlot s = a.slots[(size_t)f * a.T + i];
  if (s.key == kVxEmpty || s.minpix >= a.P || s.n == 0u) return;
  const uint32_t w = s.minpix >> 5;
  const uint32_t rank = a.wprefix[(size_t)f * a.BW + w] +
                        (uint32_t)__popc(a.bitmap[(size_t)f * a.BW + w] & ((1u << (s.minpix & 31u)) - 1u));
  if (rank >= fr.V || rank >= a.C) return;   // (cannot happen: V <= Ceff <= C)
  const size_t o = row0 + rank;
  const uint64_t n = s.n;
  if (a.vx_xyz) {
    const uint32_t cell[3] = {(uint32_t)(s.key >> 45) & 0x3FFFFu, (uint32_t)(s.key >> 27) & 0x3FFFFu,
                              (uint32_t)(s.key >> 9) & 0x3FFFFu};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t m = (uint32_t)((2ull * s.S[k] + n) / (2ull * n));
      const float c = (float)((int32_t)cell[k] - 131072);
      a.vx_xyz[o * 3u + k] = (c + ((float)m + 0.5f) * (1.0f / 65536.0f)) * a.s;
    }
  }
  if (a.vx_rgb) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.vx_rgb[o * 3u + k] = (uint8_t)((2ull * s.R[k] + n) / (2ull * n));
  }
  if (a.vx_label) a.vx_label[o] = (int32_t)(s.key & 0x1FFu) - 1;
  if (a.vx_count) a.vx_count[o] = s.n;
}

}  // namespace

void launch_voxels(const VoxelArgs& a, hipStream_t st) {
  const auto blocks = [](uint32_t items) { return (items + kVxBlock - 1u) / kVxBlock; };
  hipLaunchKernelGGL(k_vx_init, dim3(blocks(a.T > a.BW ? a.T : a.BW), a.n), dim3(kVxBlock), 0, st, a);
  if (a.combine) hipLaunchKernelGGL(k_vx_insert<true>, dim3(blocks(a.P), a.n), dim3(kVxBlock), 0, st, a);
  else hipLaunchKernelGGL(k_vx_insert<false>, dim3(blocks(a.P), a.n), dim3(kVxBlock), 0, st, a);
  hipLaunchKernelGGL(k_vx_mark, dim3(blocks(a.T), a.n), dim3(kVxBlock), 0, st, a);
  hipLaunchKernelGGL(k_vx_scan, dim3(a.n), dim3(kVxScanBlock), 0, st, a);
  hipLaunchKernelGGL(k_vx_emit, dim3(blocks(a.T > a.C ? a.T : a.C), a.n), dim3(kVxBlock), 0, st, a);
}

}  // namespace csg
