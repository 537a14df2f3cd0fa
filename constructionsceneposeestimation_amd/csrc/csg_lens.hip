// csg_lens.hip — lens distortion for csg_lens_remap and csg_lens_points: pinhole frames in device memory
// resampled by a per-lens map into the frames of a camera with Brown-Conrady distortion, with their ids,
// depth, object coordinates, per-label statistics and keypoints.  The definition is the spec of
// include/csg_api.h, restated in NumPy by tests/lens_ref.py.  Everything is an integer
// or a bit copy: no result depends on scheduling.
//
//   k_ln_init    lens_stats to inst_stats' empty value and lens_count to 0, ahead of the atomics
//   k_ln_remap   a 64 x 16 tile of output pixels per workgroup, a wave per row of 64 (the row's gathers
//                fall into one or two source rows): the map as 8-byte entries, ids / depth / validity
//                stored directly, the 3-byte RGB and 6-byte coordinate rows staged in LDS and stored as
//                dwords, the labels' statistics and the causes' counts reduced in LDS, then one integer
//                atomic per touched value and workgroup
//   k_ln_points  a thread per keypoint: the forward model in float32
#include "csg_lens.h"

namespace csg {

namespace {

constexpr uint32_t kLnBlock = 256;
constexpr uint32_t kLnTileW = 64, kLnTileH = 16;   // pixels of a k_ln_remap workgroup
constexpr uint32_t kLnMaxLabels = 256;              // CSG_SPAN_MAX_LABELS
constexpr uint32_t kLnRgbWords = 50;                // a staged row: 3 bytes of phase + 64 * 3, in dwords
constexpr uint32_t kLnCrdWords = 98;                // 2 bytes of phase + 64 * 6
constexpr uint32_t kLnEmpty = 0xFFFFFFFFu;

// grid-stride over the two arrays
__global__ __launch_bounds__(kLnBlock) void k_ln_init(uint32_t* stats, size_t n_stats, uint32_t* count, size_t n_count) {
  const size_t step = (size_t)gridDim.x * kLnBlock;
  for (size_t i = (size_t)blockIdx.x * kLnBlock + threadIdx.x; i < n_stats; i += step) {
    const uint32_t k = (uint32_t)(i % 5u);
    stats[i] = (k == 1u || k == 2u) ? kLnEmpty : 0u;
  }
  for (size_t i = (size_t)blockIdx.x * kLnBlock + threadIdx.x; i < n_count; i += step) count[i] = 0u;
}

// The `len` bytes staged in `row` behind `phase` = start & 3 spare bytes, to base[start ..]: whole dwords
// where the destination holds them, single bytes at the two ends.  `base` is 4-byte aligned.
__device__ __forceinline__ void ln_store_row(uint8_t* base, size_t start, uint32_t len, const uint32_t* row, uint32_t lane) {
  const uint32_t phase = (uint32_t)(start & 3u), end = phase + len, nd = (end + 3u) >> 2;
  uint8_t* g0 = base + start - phase;
  const uint8_t* rb = reinterpret_cast<const uint8_t*>(row);
  for (uint32_t k = lane; k < nd; k += 64u) {
    const uint32_t lo = 4u * k;
    if (lo >= phase && lo + 4u <= end) {
      reinterpret_cast<uint32_t*>(g0)[k] = row[k];
    } else {
      const uint32_t b1 = min(lo + 4u, end);
      for (uint32_t b = max(lo, phase); b < b1; ++b) g0[b] = rb[b];
    }
  }
}

// grid (ceil(W / 64), ceil(H / 16), n): thread (lane, w) of 64 x 4 does the tile's pixels (lane, w + 4 k)
__global__ __launch_bounds__(kLnBlock) void k_ln_remap(LensArgs a, uint32_t first) {
  __shared__ uint32_t s_rgb[kLnTileH][kLnRgbWords];
  __shared__ uint32_t s_crd[kLnTileH][kLnCrdWords];
  __shared__ uint32_t s_stats[kLnMaxLabels * 5u];
  __shared__ uint32_t s_count[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const size_t f = (size_t)first + blockIdx.z;
  const uint32_t x0 = blockIdx.x * kLnTileW, y0 = blockIdx.y * kLnTileH;
  const uint32_t n_stats = a.lens_stats ? a.n_labels * 5u : 0u;   // n_labels <= kLnMaxLabels (host check)
  for (uint32_t k = tid; k < n_stats; k += kLnBlock) {
    const uint32_t m = k % 5u;
    s_stats[k] = (m == 1u || m == 2u) ? kLnEmpty : 0u;
  }
  if (tid < 4u) s_count[tid] = 0u;
  __syncthreads();
  const uint32_t x = x0 + lane;
  const bool inx = x < a.W;
  const size_t SP = (size_t)a.SW * a.SH;
  uint32_t mine = 0;   // this thread's pixels per cause, 10 bits a cause (a wave has at most 256 pixels)
#pragma unroll
  for (uint32_t k = 0; k < kLnTileH / 4u; ++k) {
    const uint32_t ty = w + 4u * k, y = y0 + ty;
    if (y >= a.H) continue;   // the whole wave
    const size_t row0 = (f * a.H + y) * a.W + x0;   // the tile row's first pixel
    int32_t label = -1;
    if (inx) {
      const int2 q = reinterpret_cast<const int2*>(a.map)[(size_t)y * a.W + x];
      const int32_t px = q.x >> 8, py = q.y >> 8;
      uint32_t cause;
      if (q.x == INT32_MIN) cause = q.y == 1 ? 1u : 2u;
      else cause = (px < 0 || px >= (int32_t)a.SW || py < 0 || py >= (int32_t)a.SH) ? 2u : 0u;
      int32_t id = -1;
      uint32_t dbits = 0x7F800000u;   // +inf
      uint32_t c0 = 0, c1 = 0, c2 = 0, r = 0, g = 0, b = 0;
      if (cause == 0u) {
        const size_t s = f * SP + (size_t)py * a.SW + (uint32_t)px;
        if (a.instance) id = a.instance[s];
        if (a.lens_depth) dbits = reinterpret_cast<const uint32_t*>(a.depth)[s];
        if (a.lens_coords) {
          const uint16_t* c = a.obj_coords + s * 3u;
          c0 = c[0];
          c1 = c[1];
          c2 = c[2];
        }
        if (a.lens_rgb) {
          if (a.nearest) {
            const uint8_t* c = a.rgb + s * 3u;
            r = c[0];
            g = c[1];
            b = c[2];
          } else {
            const int32_t tx = q.x - 128, tyq = q.y - 128;   // q >= 0 here
            const uint32_t fx8 = (uint32_t)tx & 255u, fy8 = (uint32_t)tyq & 255u;
            const int32_t xa = tx >> 8, ya = tyq >> 8;
            const uint32_t xl = (uint32_t)max(xa, 0), xr = (uint32_t)min(xa + 1, (int32_t)a.SW - 1);
            const uint32_t yt = (uint32_t)max(ya, 0), yb = (uint32_t)min(ya + 1, (int32_t)a.SH - 1);
            const uint8_t* img = a.rgb + f * SP * 3u;
            const uint8_t* t00 = img + ((size_t)yt * a.SW + xl) * 3u;
            const uint8_t* t01 = img + ((size_t)yt * a.SW + xr) * 3u;
            const uint8_t* t10 = img + ((size_t)yb * a.SW + xl) * 3u;
            const uint8_t* t11 = img + ((size_t)yb * a.SW + xr) * 3u;
            const uint32_t w00 = (256u - fx8) * (256u - fy8), w01 = fx8 * (256u - fy8), w10 = (256u - fx8) * fy8,
                           w11 = fx8 * fy8;
            r = (w00 * t00[0] + w01 * t01[0] + w10 * t10[0] + w11 * t11[0] + 32768u) >> 16;
            g = (w00 * t00[1] + w01 * t01[1] + w10 * t10[1] + w11 * t11[1] + 32768u) >> 16;
            b = (w00 * t00[2] + w01 * t01[2] + w10 * t10[2] + w11 * t11[2] + 32768u) >> 16;
          }
        }
        if (id >= 0 && (uint32_t)id < a.n_labels) label = id;
      }
      const size_t o = row0 + lane;
      if (a.lens_instance) a.lens_instance[o] = id;
      if (a.lens_depth) reinterpret_cast<uint32_t*>(a.lens_depth)[o] = dbits;
      if (a.lens_valid) a.lens_valid[o] = (uint8_t)cause;
      if (a.lens_rgb) {
        uint8_t* p = reinterpret_cast<uint8_t*>(s_rgb[ty]) + (uint32_t)((row0 * 3u) & 3u) + lane * 3u;
        p[0] = (uint8_t)r;
        p[1] = (uint8_t)g;
        p[2] = (uint8_t)b;
      }
      if (a.lens_coords) {
        uint16_t* p = reinterpret_cast<uint16_t*>(s_crd[ty]) + (uint32_t)(((row0 * 6u) & 3u) >> 1) + lane * 3u;
        p[0] = (uint16_t)c0;
        p[1] = (uint16_t)c1;
        p[2] = (uint16_t)c2;
      }
      mine += 1u << (10u * cause);
    }
    if (a.lens_stats) {   // a wave of one label (the usual case) adds its row once
      const int32_t l0 = __shfl(label, 0);
      if (__ballot(label == l0) == ~0ull) {
        if (l0 >= 0 && lane == 0u) {
          uint32_t* s = s_stats + (uint32_t)l0 * 5u;
          atomicAdd(s, 64u);
          atomicMin(s + 1, x0);
          atomicMin(s + 2, y);
          atomicMax(s + 3, x0 + 63u);
          atomicMax(s + 4, y);
        }
      } else if (label >= 0) {
        uint32_t* s = s_stats + (uint32_t)label * 5u;
        atomicAdd(s, 1u);
        atomicMin(s + 1, x);
        atomicMin(s + 2, y);
        atomicMax(s + 3, x);
        atomicMax(s + 4, y);
      }
    }
  }
  __syncthreads();
  const uint32_t tw = min(kLnTileW, a.W - x0);
#pragma unroll
  for (uint32_t k = 0; k < kLnTileH / 4u; ++k) {
    const uint32_t ty = w + 4u * k, y = y0 + ty;
    if (y >= a.H) continue;
    const size_t row0 = (f * a.H + y) * a.W + x0;
    if (a.lens_rgb) ln_store_row(a.lens_rgb, row0 * 3u, tw * 3u, s_rgb[ty], lane);
    if (a.lens_coords) ln_store_row(reinterpret_cast<uint8_t*>(a.lens_coords), row0 * 6u, tw * 6u, s_crd[ty], lane);
  }
  if (a.lens_count) {
#pragma unroll
    for (uint32_t s = 32u; s > 0u; s >>= 1) mine += __shfl_xor(mine, s);
    if (lane == 0u) {
#pragma unroll
      for (uint32_t c = 0; c < kLnCauses; ++c) {
        const uint32_t v = (mine >> (10u * c)) & 0x3FFu;
        if (v) atomicAdd(&s_count[c], v);
      }
    }
  }
  __syncthreads();
  if (a.lens_count && tid < kLnCauses && s_count[tid]) atomicAdd(&a.lens_count[f * kLnCauses + tid], s_count[tid]);
  if (a.lens_stats) {
    for (uint32_t l = tid; l < a.n_labels; l += kLnBlock) {
      const uint32_t* s = s_stats + l * 5u;
      if (!s[0]) continue;
      uint32_t* g = a.lens_stats + (f * a.n_labels + l) * 5u;
      atomicAdd(g, s[0]);
      atomicMin(g + 1, s[1]);
      atomicMin(g + 2, s[2]);
      atomicMax(g + 3, s[3]);
      atomicMax(g + 4, s[4]);
    }
  }
}

// grid (ceil(total / 256))
__global__ __launch_bounds__(kLnBlock) void k_ln_points(LensPointArgs m) {
  const uint32_t i = blockIdx.x * kLnBlock + threadIdx.x;
  if (i >= m.total) return;
  const float u = m.uv[2u * (size_t)i], v = m.uv[2u * (size_t)i + 1u];
  const float x = (u - m.scx) / m.sfx, y = (v - m.scy) / m.sfy;
  const float xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2;
  const float N = 1.0f + ((m.k1 * r2 + m.k2 * r4) + m.k3 * r6), D = 1.0f + ((m.k4 * r2 + m.k5 * r4) + m.k6 * r6);
  const float Np = (m.k1 + (2.0f * m.k2) * r2) + (3.0f * m.k3) * r4, Dp = (m.k4 + (2.0f * m.k5) * r2) + (3.0f * m.k6) * r4;
  const float R = N / D, Rp = (Np * D - N * Dp) / (D * D);
  const float xd = (x * R + (2.0f * m.p1) * xy) + m.p2 * (r2 + 2.0f * xx);
  const float yd = (y * R + m.p1 * (r2 + 2.0f * yy)) + (2.0f * m.p2) * xy;
  const float a = ((R + (2.0f * xx) * Rp) + (2.0f * m.p1) * y) + (6.0f * m.p2) * x;
  const float b = ((2.0f * xy) * Rp + (2.0f * m.p1) * x) + (2.0f * m.p2) * y;
  const float d = ((R + (2.0f * yy) * Rp) + (6.0f * m.p1) * y) + (2.0f * m.p2) * x;
  float uo = m.fx * xd + m.cx, vo = m.fy * yd + m.cy;
  int32_t vis = m.vis[i];
  if (!(__builtin_isfinite(uo) && __builtin_isfinite(vo) && __builtin_isfinite(a) && __builtin_isfinite(b) &&
        __builtin_isfinite(d))) {
    uo = 0.0f;
    vo = 0.0f;
    vis = 0;
  } else if (!(uo >= 0.0f && uo < m.W && vo >= 0.0f && vo < m.H) || !(a * d - b * b > 0.0f && a + d > 0.0f)) {
    vis = 0;
  }
  m.lens_uv[2u * (size_t)i] = uo;
  m.lens_uv[2u * (size_t)i + 1u] = vo;
  m.lens_vis[i] = vis;
}

}  // namespace

void launch_lens(const LensArgs& a, hipStream_t st) {
  if (a.lens_stats || a.lens_count) {
    const size_t n_stats = a.lens_stats ? (size_t)a.n * a.n_labels * 5u : 0u, n_count = a.lens_count ? (size_t)a.n * kLnCauses : 0u;
    const size_t most = n_stats > n_count ? n_stats : n_count;
    const uint32_t blocks = (uint32_t)((most + kLnBlock - 1u) / kLnBlock < 2048u ? (most + kLnBlock - 1u) / kLnBlock : 2048u);
    hipLaunchKernelGGL(k_ln_init, dim3(blocks), dim3(kLnBlock), 0, st, a.lens_stats, n_stats, a.lens_count, n_count);
  }
  constexpr uint32_t kRange = 65535u;   // grid z limit
  for (uint32_t f0 = 0; f0 < a.n; f0 += kRange) {
    const uint32_t n = a.n - f0 < kRange ? a.n - f0 : kRange;
    hipLaunchKernelGGL(k_ln_remap, dim3((a.W + kLnTileW - 1u) / kLnTileW, (a.H + kLnTileH - 1u) / kLnTileH, n),
                       dim3(kLnBlock), 0, st, a, f0);
  }
}

void launch_lens_points(const LensPointArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_ln_points, dim3((a.total + kLnBlock - 1u) / kLnBlock), dim3(kLnBlock), 0, st, a);
}

}  // namespace csg
