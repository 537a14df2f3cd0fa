// csg_points.hip — fixed-size per-object point samples for csg_sample_object_points:
// N pixels of every slot's label, their image indices, camera-frame points,
// colours and object coordinates, made from the arrays a render wrote without
// leaving the GPU.  The definition is the spec of include/csg_api.h (DESIGN.md
// §13.6), restated in NumPy by tests/test_object_points.py.  Which pixel a sample
// takes is integer arithmetic only; the one float expression is the camera point.
//
//   k_pts_count  per (frame, chunk of 4096 row-major pixels): the pixels of each wanted label
//   k_pts_scan   per (frame, slot): the exclusive scan of a label's counts over the chunks,
//                which is the rank of its first pixel in each chunk; M; pt_count; and the
//                fill of the slots without pixels
//   k_pts_emit   per (frame, chunk): every pixel of a wanted label knows its rank r among the
//                label's pixels, decides from (r, M, N, seed, key, label) alone which samples
//                it is, and writes them for every slot that names the label
//
// A wave owns a chunk and walks it 64 x V ids a step (V = 4: one 16-byte load per lane; V = 1
// where the frame's pixel count or the pointer does not allow that).  A pixel's rank is
//   rank of the label's first pixel in the chunk         -- k_pts_scan
//   + the label's pixels in earlier steps of the chunk    -- the running LDS entry run[label]
//   + those in lower lanes, and in the lane's lower components  -- ballots
// which is the row-major order of the spec by construction: no atomic decides a position and
// the result does not depend on how waves are scheduled.  A "wanted" label is one a live slot
// names; slots[label] is the 64-bit set of those slots (K <= 64), so ids outside [0, L) and
// labels nobody asked for never index a table and cost one comparison.
#include "csg_points.h"

namespace csg {

namespace {

__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// slots[l] = the set of live slots of frame f that name label l (0: nobody wants l).
__device__ __forceinline__ void pts_slot_sets(const PointArgs& a, uint32_t f, uint32_t lane, uint64_t* slots) {
  for (uint32_t l = lane; l < a.L; l += 64u) slots[l] = 0ull;
  __syncthreads();
  int32_t lab = -1;
  if (lane < a.K) {
    const CropSlot sl{a.info[(size_t)f * a.K + lane].label, 0u, 0.f, 0.f, 0.f, 0u, {0u, 0u}};
    if (crop_label_live(sl, a.L)) lab = sl.label;
  }
  uint64_t pend = __ballot(lab >= 0);
  while (pend) {   // wave-uniform: one turn per distinct label
    const int32_t l = __builtin_amdgcn_readlane(lab, __ffsll((unsigned long long)pend) - 1);
    const uint64_t m = __ballot(lab == l);
    if (lane == 0) slots[l] = m;
    pend &= ~m;
  }
  __syncthreads();
}

// The V ids of a lane at pixel p of the frame; lanes at or past the chunk's end p1 load nothing.
template <int V>
__device__ __forceinline__ void pts_load(const int32_t* __restrict__ ids, uint32_t p, uint32_t p1, int32_t (&v)[V]) {
  if constexpr (V == 4) {   // p and p1 are multiples of 4 here, so p < p1 covers p + 3
    int4 q = make_int4(-1, -1, -1, -1);
    if (p < p1) q = *reinterpret_cast<const int4*>(ids + p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = p < p1 ? ids[p] : -1;
  }
}

// What k_pts_emit knows about its frame.
struct PtFrame {
  uint32_t f, fk;            // the frame, fmix32(seed ^ key)
  float fx, fy, cx, cy;
};

// Pixel p of frame f is the pixel of rank r among the M pixels of label l: writes the samples it is.
__device__ __forceinline__ void pts_emit_pixel(const PointArgs& a, const PtFrame& fr, uint32_t l, uint32_t r,
                                               uint32_t M, uint32_t p, uint64_t slot_set) {
  const uint32_t N = a.N;
  if (r >= M) return;   // (the ids changed between the passes: nothing is written out of place)
  uint32_t s0 = r, step = M;   // M <= N: samples r, r + M, ... (np.pad 'wrap')
  if (M > N) {
    // the stratum of r: the largest s with (s * M) / N <= r, that is ((r + 1) * N - 1) / M; a float
    // estimate made exact by multiply-compare (the products stay below 2^41)
    const uint64_t t = (uint64_t)(r + 1u) * N - 1u;
    uint32_t s = (uint32_t)fminf((float)t * __builtin_amdgcn_rcpf((float)M), (float)(N - 1u));
    while ((uint64_t)s * M > t) --s;
    while ((uint64_t)(s + 1u) * M <= t) ++s;
    // lo_s = (s * M) / N with M = qN * N + rN: s * qN + (s * rN) / N, all below 2^32
    const uint32_t qN = M / N, rN = M - qN * N;
    const uint32_t lo = s * qN + (s * rN) / N, hi = (s + 1u) * qN + ((s + 1u) * rN) / N;
    const uint32_t h = fmix32(fmix32(fr.fk ^ l) ^ (s * 0x9E3779B9u));
    if (r != lo + (uint32_t)(((uint64_t)h * (hi - lo)) >> 32)) return;
    s0 = s;
    step = N;
  }
  const size_t gp = (size_t)fr.f * a.P + p;
  float X = 0.f, Y = 0.f, Z = 0.f;
  if (a.pt_xyz) {
    const uint32_t py = p / a.W, px = p - py * a.W;
    const float d = a.depth[gp];
    X = ((((float)px + 0.5f) - fr.cx) * d) / fr.fx;
    Y = ((((float)py + 0.5f) - fr.cy) * d) / fr.fy;
    Z = d;
    if (X != X) X = __uint_as_float(0x7FC00000u);   // the one NaN of the spec
    if (Y != Y) Y = __uint_as_float(0x7FC00000u);
  }
  uint8_t c0 = 0, c1 = 0, c2 = 0;
  if (a.pt_rgb) c0 = a.rgb[gp * 3u], c1 = a.rgb[gp * 3u + 1u], c2 = a.rgb[gp * 3u + 2u];
  uint16_t o0 = 0, o1 = 0, o2 = 0;
  if (a.pt_coords) o0 = a.obj_coords[gp * 3u], o1 = a.obj_coords[gp * 3u + 1u], o2 = a.obj_coords[gp * 3u + 2u];
  for (uint32_t s = s0; s < N; s += step) {
    for (uint64_t m = slot_set; m; m &= m - 1ull) {
      const uint32_t k = (uint32_t)__ffsll((unsigned long long)m) - 1u;
      const size_t i = ((size_t)fr.f * a.K + k) * N + s;
      if (a.pt_choose) a.pt_choose[i] = p;
      if (a.pt_xyz) a.pt_xyz[i * 3u] = X, a.pt_xyz[i * 3u + 1u] = Y, a.pt_xyz[i * 3u + 2u] = Z;
      if (a.pt_rgb) a.pt_rgb[i * 3u] = c0, a.pt_rgb[i * 3u + 1u] = c1, a.pt_rgb[i * 3u + 2u] = c2;
      if (a.pt_coords) a.pt_coords[i * 3u] = o0, a.pt_coords[i * 3u + 1u] = o1, a.pt_coords[i * 3u + 2u] = o2;
    }
  }
}

// Walks the wave's chunk.  run[l] is the running count of wanted label l: every step reads it
// (the rank of the step's first pixel of l when kEmit) and adds the step's pixels of l.
template <int V, bool kEmit>
__device__ __forceinline__ void pts_walk(const PointArgs& a, const PtFrame& fr, uint32_t chunk, uint32_t lane,
                                         const uint64_t* slots, uint32_t* run, const uint32_t* tot) {
  const uint32_t L = a.L;
  const int32_t* ids = a.instance + (size_t)fr.f * a.P;
  const uint32_t p0 = chunk * kPointChunk, p1 = min(p0 + kPointChunk, a.P);
  const uint64_t below_me = (1ull << lane) - 1ull;
  int32_t nxt[V];
  pts_load<V>(ids, p0 + lane * V, p1, nxt);
  for (uint32_t b = p0; b < p1; b += 64u * V) {   // wave-uniform
    int32_t cur[V];
    uint32_t rank[V];
    uint32_t pend = 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const int32_t id = nxt[c];
      bool wanted = false;
      if ((uint32_t)id < L) wanted = slots[id] != 0ull;
      cur[c] = wanted ? id : -1;
      rank[c] = 0;
      pend |= (wanted ? 1u : 0u) << c;
    }
    pts_load<V>(ids, b + 64u * V + lane * V, p1, nxt);   // the next step's ids are in flight meanwhile
    for (;;) {   // wave-uniform: one turn per distinct wanted label of the step
      const uint64_t open = __ballot(pend != 0u);
      if (!open) break;
      int32_t mine = -1;
#pragma unroll
      for (int c = V - 1; c >= 0; --c)
        if (pend >> c & 1u) mine = cur[c];
      const int32_t l = __builtin_amdgcn_readlane(mine, __ffsll((unsigned long long)open) - 1);
      const uint32_t before = run[l];
      uint32_t all = 0, lower = 0;   // the step's pixels of l; those in lower lanes (every component)
#pragma unroll
      for (int c = 0; c < V; ++c) {   // (a label's pixels are all open until its turn: cur == l is enough)
        const uint64_t bal = __ballot(cur[c] == l);
        all += (uint32_t)__popcll(bal);
        lower += (uint32_t)__popcll(bal & below_me);
      }
#pragma unroll
      for (int c = 0; c < V; ++c) {
        if (cur[c] != l) continue;
        if (kEmit) rank[c] = before + lower++;   // ... and in the lane's lower components
        pend &= ~(1u << c);
      }
      __syncthreads();   // every lane has read run[l]
      if (lane == 0) run[l] = before + all;
      __syncthreads();
    }
    if (kEmit) {
#pragma unroll
      for (int c = 0; c < V; ++c)
        if (cur[c] >= 0)
          pts_emit_pixel(a, fr, (uint32_t)cur[c], rank[c], tot[cur[c]], b + lane * V + c, slots[cur[c]]);
    }
  }
}

// grid (chunks, frames), one wave per workgroup
template <int V>
__global__ __launch_bounds__(64) void k_pts_count(PointArgs a, uint32_t f0) {
  __shared__ uint64_t slots[kPointMaxLabels];
  __shared__ uint32_t run[kPointMaxLabels];
  const uint32_t lane = threadIdx.x, chunk = blockIdx.x, f = f0 + blockIdx.y;
  pts_slot_sets(a, f, lane, slots);
  for (uint32_t l = lane; l < a.L; l += 64u) run[l] = 0u;
  __syncthreads();
  PtFrame fr{};
  fr.f = f;
  pts_walk<V, false>(a, fr, chunk, lane, slots, run, nullptr);
  for (uint32_t l = lane; l < a.L; l += 64u)
    if (slots[l]) a.cnt[((size_t)f * a.L + l) * a.CH + chunk] = run[l];
}

// grid (K, frames).  The block of slot k scans the chunk counts of the slot's label in place, unless a
// lower slot names the same label (that slot's block does it), and finishes every slot of the label:
// pt_count, and the empty values where the label has no pixel.  A dead slot's block writes its own.
__global__ __launch_bounds__(256) void k_pts_scan(PointArgs a, uint32_t f0) {
  __shared__ uint32_t part[256];
  const uint32_t tid = threadIdx.x, k = blockIdx.x, f = f0 + blockIdx.y;
  const CropSlot* info = a.info + (size_t)f * a.K;
  const int32_t lab = info[k].label;
  const bool live = lab >= 0 && (uint32_t)lab < a.L;
  uint32_t M = 0;
  if (live) {
    for (uint32_t j = 0; j < k; ++j)
      if (info[j].label == lab) return;   // uniform over the block
    const uint32_t per = (a.CH + 255u) / 256u;
    const uint32_t lo = min(tid * per, a.CH), hi = min(lo + per, a.CH);
    uint32_t* c = a.cnt + ((size_t)f * a.L + (uint32_t)lab) * a.CH;
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
    uint32_t first = part[tid] - s;
    for (uint32_t i = lo; i < hi; ++i) {
      const uint32_t v = c[i];
      c[i] = first;
      first += v;
    }
    M = part[255];   // at most W * H <= 2^26
    if (tid == 0) a.total[(size_t)f * a.L + (uint32_t)lab] = M;
  }
  for (uint32_t j = k; j < (live ? a.K : k + 1u); ++j) {
    if (j != k && info[j].label != lab) continue;
    const size_t slot = (size_t)f * a.K + j;
    if (tid == 0 && a.pt_count) a.pt_count[slot] = M;
    if (M) continue;
    for (uint32_t s = tid; s < a.N; s += 256u) {
      const size_t i = slot * a.N + s;
      if (a.pt_choose) a.pt_choose[i] = 0xFFFFFFFFu;
      if (a.pt_xyz) {
        const float nan = __uint_as_float(0x7FC00000u);
        a.pt_xyz[i * 3u] = nan, a.pt_xyz[i * 3u + 1u] = nan, a.pt_xyz[i * 3u + 2u] = nan;
      }
      if (a.pt_rgb) a.pt_rgb[i * 3u] = 0, a.pt_rgb[i * 3u + 1u] = 0, a.pt_rgb[i * 3u + 2u] = 0;
      if (a.pt_coords) a.pt_coords[i * 3u] = 0, a.pt_coords[i * 3u + 1u] = 0, a.pt_coords[i * 3u + 2u] = 0;
    }
  }
}

// grid (chunks, frames), as k_pts_count
template <int V>
__global__ __launch_bounds__(64) void k_pts_emit(PointArgs a, uint32_t f0) {
  __shared__ uint64_t slots[kPointMaxLabels];
  __shared__ uint32_t run[kPointMaxLabels];
  __shared__ uint32_t tot[kPointMaxLabels];
  const uint32_t lane = threadIdx.x, chunk = blockIdx.x, f = f0 + blockIdx.y;
  pts_slot_sets(a, f, lane, slots);
  for (uint32_t l = lane; l < a.L; l += 64u) {
    if (!slots[l]) continue;
    run[l] = a.cnt[((size_t)f * a.L + l) * a.CH + chunk];
    tot[l] = a.total[(size_t)f * a.L + l];
  }
  __syncthreads();
  PtFrame fr{};
  fr.f = f;
  fr.fk = fmix32(a.seed ^ (a.frame_keys ? a.frame_keys[f] : f));
  if (a.pt_xyz) {
    const float* in = a.intrinsics + (size_t)f * 4u;
    fr.fx = in[0], fr.fy = in[1], fr.cx = in[2], fr.cy = in[3];
  }
  pts_walk<V, true>(a, fr, chunk, lane, slots, run, tot);
}

bool pts_vector_ids(const PointArgs& a) { return (a.P & 3u) == 0u && ((uintptr_t)a.instance & 15u) == 0u; }

}  // namespace

void launch_pts_count(const PointArgs& a, uint32_t n, hipStream_t st) {
  for (uint32_t f0 = 0; f0 < n; f0 += 65535u) {   // grid y limit
    const uint32_t nf = n - f0 < 65535u ? n - f0 : 65535u;
    if (pts_vector_ids(a)) hipLaunchKernelGGL(k_pts_count<4>, dim3(a.CH, nf), dim3(64), 0, st, a, f0);
    else hipLaunchKernelGGL(k_pts_count<1>, dim3(a.CH, nf), dim3(64), 0, st, a, f0);
  }
}

void launch_pts_scan(const PointArgs& a, uint32_t n, hipStream_t st) {
  for (uint32_t f0 = 0; f0 < n; f0 += 65535u) {
    const uint32_t nf = n - f0 < 65535u ? n - f0 : 65535u;
    hipLaunchKernelGGL(k_pts_scan, dim3(a.K, nf), dim3(256), 0, st, a, f0);
  }
}

void launch_pts_emit(const PointArgs& a, uint32_t n, hipStream_t st) {
  for (uint32_t f0 = 0; f0 < n; f0 += 65535u) {
    const uint32_t nf = n - f0 < 65535u ? n - f0 : 65535u;
    if (pts_vector_ids(a)) hipLaunchKernelGGL(k_pts_emit<4>, dim3(a.CH, nf), dim3(64), 0, st, a, f0);
    else hipLaunchKernelGGL(k_pts_emit<1>, dim3(a.CH, nf), dim3(64), 0, st, a, f0);
  }
}

}  // namespace csg
