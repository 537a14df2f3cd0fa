// csg_sensor.hip — simulated stereo-camera depth for csg_sensor_depth: an ideal depth image as a stereo
// depth camera registered to the colour camera would return it (half-occlusion holes, window erosion,
// quantised and noisy disparity), with the cause of every missing value, without leaving the GPU.  The
// definition is the spec of include/csg_api.h, restated in NumPy by
// tests/depth_sensor_ref.py.  Everything past the one division per pixel is an integer in 1/256 px of
// disparity: no result depends on scheduling.
//
//   k_sn_rows    a wave per row: dq and the rules 1-4 of every pixel, the half-occlusion test as an
//                exclusive running minimum along the row, into one int32 of state per pixel
//   k_sn_match   a 64 x 16 tile of the state image in LDS with a halo of r: the window count, the hash,
//                the noise and the one division; sensor_depth, sensor_cause, the causes' counts
//   k_sn_counts  the frames' counts from the scratch to sensor_count
//
// The scan.  For b > 0 a pixel is hidden iff some surface pixel to its right has u' <= u, for b < 0 iff one
// to its left has u' >= u.  With v = u for b > 0 and v = -u for b < 0, and the row walked from the side
// the second camera is on, both are "the minimum of v over the surface pixels walked before is <= v".
// A wave walks its row in chunks of 64 columns: lane l of chunk c holds column W - 1 - (64 c + l) for
// b > 0 and 64 c + l for b < 0, so the chunk is 256 contiguous bytes either way.  The chunk's inclusive
// prefix minimum is six shuffle steps; the minimum of the chunks before is carried in a wave-uniform
// register.
#include "csg_sensor.h"

namespace csg {

namespace {

constexpr uint32_t kSnBlock = 256;
constexpr uint32_t kSnTileW = 64, kSnTileH = 16;   // pixels of a k_sn_match workgroup
constexpr uint32_t kSnMaxR = 4;
constexpr uint32_t kSnLdsW = kSnTileW + 2 * kSnMaxR, kSnLdsH = kSnTileH + 2 * kSnMaxR;   // 72 x 24 words
constexpr int32_t kSnNone = 0x7FFFFFFF;            // the minimum over no pixel

__device__ __forceinline__ uint32_t sn_fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// grid (ceil(H / 4), n): a wave per row
__global__ __launch_bounds__(kSnBlock) void k_sn_rows(SensorArgs a) {
  const uint32_t f = blockIdx.y, lane = threadIdx.x & 63u, y = blockIdx.x * (kSnBlock / 64u) + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x < kSnCountStride) a.counts[(size_t)f * kSnCountStride + threadIdx.x] = 0u;
  if (y >= a.H) return;   // the whole wave
  const float fb = a.intrinsics[(size_t)(a.first + f) * 4u] * a.abs_b;
  const float* __restrict__ row = a.depth + ((size_t)(a.first + f) * a.H + y) * a.W;
  int32_t* __restrict__ srow = a.state + ((size_t)f * a.H + y) * a.W;
  const int32_t band = (int32_t)(256u * a.W);
  int32_t carry = kSnNone;   // min of v over the surface pixels of the chunks walked so far
  for (uint32_t i0 = 0; i0 < a.W; i0 += 64u) {
    const uint32_t i = i0 + lane;
    const bool in = i < a.W;
    const uint32_t x = in ? (a.right ? a.W - 1u - i : i) : 0u;
    const float d = row[x];
    const float D = fb / d;
    const bool surface = in && __builtin_isfinite(d) && d > 0.0f && D > 0.0f;
    uint32_t dq = 1u << 30;
    if (surface && !__builtin_isinf(D) && !(D >= 4194304.0f)) dq = (uint32_t)(D * 256.0f + 0.5f);
    const int32_t c = (int32_t)(256u * x + 128u);
    const int32_t u = a.right ? c - (int32_t)dq : c + (int32_t)dq;
    const int32_t v = a.right ? u : -u;
    int32_t incl = surface ? v : kSnNone;
#pragma unroll
    for (uint32_t s = 1; s < 64u; s <<= 1) {
      const int32_t t = __shfl_up(incl, s);
      if (lane >= s) incl = min(incl, t);
    }
    int32_t before = __shfl_up(incl, 1u);
    before = min(lane == 0u ? kSnNone : before, carry);
    carry = min(carry, __shfl(incl, 63));
    int32_t state;
    if (!surface) state = -1;
    else if (!(a.z_min <= d && d <= a.z_max)) state = -2;
    else if (before <= v) state = -3;
    else if (a.clip_band && (a.right ? u < 0 : u >= band)) state = -4;
    else state = (int32_t)dq;
    if (in) srow[x] = state;
  }
}

// The lit pixels of the (2R+1)^2 window around a lit centre whose dq is within tol of the centre's;
// `t` points at the centre's word of the LDS tile.
template <int R>
__device__ __forceinline__ uint32_t sn_support(const int32_t* t, int32_t c, uint32_t tol) {
  uint32_t n = 0;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      const int32_t v = t[dy * (int)kSnLdsW + dx];
      const uint32_t diff = v > c ? (uint32_t)(v - c) : (uint32_t)(c - v);
      n += (v >= 0 && diff <= tol) ? 1u : 0u;
    }
  }
  return n;
}

// grid (ceil(W / 64), ceil(H / 16), n): thread (tx, ty) of 64 x 4 does the tile's pixels (tx, ty + 4 k)
__global__ __launch_bounds__(kSnBlock) void k_sn_match(SensorArgs a) {
  __shared__ int32_t tile[kSnLdsH * kSnLdsW];
  __shared__ uint32_t blk_count[kSnCountStride];
  const uint32_t f = blockIdx.z, tid = threadIdx.x, r = a.r;
  const uint32_t x0 = blockIdx.x * kSnTileW, y0 = blockIdx.y * kSnTileH;
  const int32_t* __restrict__ st = a.state + (size_t)f * a.H * a.W;
  if (tid < kSnCountStride) blk_count[tid] = 0u;
  // tile cell (lx, ly) is pixel (x0 - r + lx, y0 - r + ly); cells outside the image are not lit
  const uint32_t tw = kSnTileW + 2u * r, th = kSnTileH + 2u * r;
  for (uint32_t k = tid; k < tw * th; k += kSnBlock) {
    const uint32_t ly = k / tw, lx = k - ly * tw;
    const int32_t gx = (int32_t)(x0 + lx) - (int32_t)r, gy = (int32_t)(y0 + ly) - (int32_t)r;
    int32_t v = -1;
    if (gx >= 0 && gx < (int32_t)a.W && gy >= 0 && gy < (int32_t)a.H) v = st[(size_t)gy * a.W + (uint32_t)gx];
    tile[ly * kSnLdsW + lx] = v;
  }
  __syncthreads();
  const uint32_t tx = tid & 63u, x = x0 + tx;
  const float fb256 = (a.intrinsics[(size_t)(a.first + f) * 4u] * a.abs_b) * 256.0f;
  const uint32_t key = a.frame_keys ? a.frame_keys[a.first + f] : a.first + f;
  const uint32_t base = sn_fmix32(a.seed ^ key);
  const size_t frame0 = (size_t)(a.first + f) * a.H * a.W;
  uint64_t mine = 0;   // this thread's pixels per cause, 9 bits a cause (a wave has at most 256 pixels)
#pragma unroll
  for (uint32_t k = 0; k < kSnTileH / 4u; ++k) {
    const uint32_t ty = (tid >> 6) + 4u * k, y = y0 + ty;
    if (x >= a.W || y >= a.H) continue;
    const int32_t* t = tile + (ty + r) * kSnLdsW + tx + r;
    const int32_t s = *t;
    uint32_t cause;
    float out = 0.0f;
    if (s < 0) {
      cause = (uint32_t)(-s);
    } else {
      uint32_t n;
      switch (r) {
        case 0: n = 1u; break;
        case 1: n = sn_support<1>(t, s, a.tol); break;
        case 2: n = sn_support<2>(t, s, a.tol); break;
        case 3: n = sn_support<3>(t, s, a.tol); break;
        default: n = sn_support<4>(t, s, a.tol); break;
      }
      if (n < a.min_support) {
        cause = 5u;
      } else {
        const uint32_t p = y * a.W + x;
        const uint32_t h1 = sn_fmix32(base ^ p), h2 = sn_fmix32(h1 ^ 0x9E3779B9u);
        const int64_t g = (int64_t)((h1 & 0xFFFFu) + (h1 >> 16) + (h2 & 0xFFFFu) + (h2 >> 16)) - 131070;
        const int32_t e = (int32_t)((g * (int64_t)a.noise_k + 32768) >> 16);   // |e| < 2^22
        const int32_t m = (s + e + (int32_t)((1u << a.sh) >> 1)) >> a.sh;       // s <= 2^30
        if (m <= 0) {
          cause = 6u;
        } else {
          cause = 0u;
          out = fb256 / (float)((uint32_t)m << a.sh);
        }
      }
    }
    const size_t o = frame0 + (size_t)y * a.W + x;
    if (a.sensor_depth) __builtin_nontemporal_store(out, a.sensor_depth + o);
    if (a.sensor_cause) a.sensor_cause[o] = (uint8_t)cause;
    mine += 1ull << (9u * cause);
  }
  if (!a.sensor_count) return;   // the same for every thread
  // integer sums: per wave in registers, per workgroup in LDS, one atomic per cause and workgroup
#pragma unroll
  for (uint32_t s = 32u; s > 0u; s >>= 1) mine += __shfl_xor(mine, s);
  if ((tid & 63u) == 0u) {
#pragma unroll
    for (uint32_t c = 0; c < kSnCauses; ++c) {
      const uint32_t v = (uint32_t)(mine >> (9u * c)) & 0x1FFu;
      if (v) atomicAdd(&blk_count[c], v);
    }
  }
  __syncthreads();
  if (tid < kSnCauses && blk_count[tid]) atomicAdd(&a.counts[(size_t)f * kSnCountStride + tid], blk_count[tid]);
}

// grid (ceil(n * 7 / 256))
__global__ __launch_bounds__(kSnBlock) void k_sn_counts(SensorArgs a) {
  const uint32_t i = blockIdx.x * kSnBlock + threadIdx.x;
  if (i >= a.n * kSnCauses) return;
  const uint32_t f = i / kSnCauses, c = i - f * kSnCauses;
  a.sensor_count[(size_t)(a.first + f) * kSnCauses + c] = a.counts[(size_t)f * kSnCountStride + c];
}

}  // namespace

void launch_sensor(const SensorArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sn_rows, dim3((a.H + 3u) / 4u, a.n), dim3(kSnBlock), 0, st, a);
  hipLaunchKernelGGL(k_sn_match, dim3((a.W + kSnTileW - 1u) / kSnTileW, (a.H + kSnTileH - 1u) / kSnTileH, a.n),
                     dim3(kSnBlock), 0, st, a);
  if (a.sensor_count)
    hipLaunchKernelGGL(k_sn_counts, dim3((a.n * kSnCauses + kSnBlock - 1u) / kSnBlock), dim3(kSnBlock), 0, st, a);
}

}  // namespace csg
