// csg_crops.hip — object crops (zoom-in patches) for csg_crop_objects and
// csg_crop_objects_filtered: the fixed-size patches around the largest visible
// objects of each frame that two-stage pose networks train on, cut on the GPU
// from the arrays a render wrote.  The arithmetic is the spec of
// include/csg_api.h, float32 with -ffp-contract=off,
// restated in NumPy by tests/test_object_crops.py and tests/test_crop_area.py.
//
//   k_crop_plan    per frame, the K labels with the most visible pixels and
//                  their padded square windows (deterministic top-K)
//   k_crop_sample  per slot, S x S samples of the window: nearest for mask,
//                  object coordinates and depth, integer-weight bilinear for RGB
//   k_crop_area    per minified slot under CSG_CROP_FILTER_AREA, the RGB as an
//                  exact box filter over each crop pixel's source footprint
#include "csg_crops.h"

#include <math.h>

namespace csg {

namespace {

typedef uint32_t v2u32 __attribute__((ext_vector_type(2)));
typedef uint32_t v3u32 __attribute__((ext_vector_type(3)));
typedef float v4f32 __attribute__((ext_vector_type(4)));

constexpr uint32_t kCropBlock = 256;
constexpr uint32_t kAreaBlock = 128;   // k_crop_area: threads of a workgroup,
constexpr uint32_t kAreaRows = 8;      // crop rows of a workgroup's band

// A live slot's liveness, as the spec of csg_api.h words it (NaN fails every comparison).
__device__ __forceinline__ bool slot_live(const CropArgs& a, const CropSlot& sl) {
  bool live = crop_label_live(sl, a.n_labels);
  if (a.explicit_boxes) live = live && crop_window_live(sl);
  return live;
}

// Whether k_crop_area (and not k_crop_sample) makes the RGB of a live slot:
// block-uniform, and the same expression in both kernels, so every RGB byte is
// written exactly once.  The bounds keep every edge below 2^29 in 1/256 pixel
// (a planned window may exceed them; it keeps its bilinear RGB).
__device__ __forceinline__ bool slot_area(const CropArgs& a, const CropSlot& sl) {
  return a.rgb_filter == 1u && a.crop_rgb && sl.side / (float)a.S > 1.0f && sl.side <= 32768.0f &&
         fabsf(sl.x0) <= 1048576.0f && fabsf(sl.y0) <= 1048576.0f;
}

// ---------------------------------------------------------------------------
// k_crop_plan: one workgroup per frame, K rounds of a block arg-max over the
// keys pixels << 32 | (0xFFFFFFFF - label): a larger key is more pixels, then
// the lower label, so "the largest key strictly below the previous winner" is
// the spec's order by construction -- no scratch, no atomics, and the result
// does not depend on how threads are scheduled.  Labels are visited in a
// strided loop (n_labels may exceed the block).  A candidate has pixels >=
// min_pixels >= 1, so key 0 means "none", and every later slot is empty too.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kCropBlock) void k_crop_plan(CropArgs a) {
  __shared__ unsigned long long wmax[kCropBlock / 64];
  const uint32_t f = blockIdx.x;
  const uint32_t* st = a.stats + (size_t)f * a.n_labels * 5;
  CropSlot* out = a.info + (size_t)f * a.K;
  unsigned long long prev = 0;
  for (uint32_t k = 0; k < a.K; ++k) {
    unsigned long long best = 0;
    if (k == 0 || prev != 0) {   // block-uniform
      for (uint32_t l = threadIdx.x; l < a.n_labels; l += kCropBlock) {
        const uint32_t px = st[5 * (size_t)l];
        if (px < a.min_pixels || (a.eligible && !a.eligible[l])) continue;
        const unsigned long long key = ((unsigned long long)px << 32) | (0xFFFFFFFFu - l);
        if ((k == 0 || key < prev) && key > best) best = key;
      }
#pragma unroll
      for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
      }
      if ((threadIdx.x & 63u) == 0) wmax[threadIdx.x >> 6] = best;
      __syncthreads();
      best = 0;
#pragma unroll
      for (uint32_t w = 0; w < kCropBlock / 64; ++w) best = wmax[w] > best ? wmax[w] : best;
      __syncthreads();           // wmax is rewritten by the next round
    }
    if (threadIdx.x == 0) {
      CropSlot s = {-1, 0u, 0.0f, 0.0f, 0.0f, 0u, {0u, 0u}};
      if (best) {
        const uint32_t l = 0xFFFFFFFFu - (uint32_t)best;
        const uint32_t* b = st + 5 * (size_t)l;
        const uint32_t minx = b[1], miny = b[2], maxx = b[3], maxy = b[4];
        const uint32_t w = maxx - minx + 1u, h = maxy - miny + 1u;
        const float cx = (float)(minx + maxx + 1u) * 0.5f, cy = (float)(miny + maxy + 1u) * 0.5f;
        const float side = a.pad * (float)(w > h ? w : h);
        s.label = (int32_t)l;
        s.pixels = (uint32_t)(best >> 32);
        s.x0 = cx - side * 0.5f;
        s.y0 = cy - side * 0.5f;
        s.side = side;
        s.frame = f;
      }
      out[k] = s;
    }
    prev = best;
  }
}

// ---------------------------------------------------------------------------
// k_crop_sample: grid (quads of a crop / 256, K, frames); one thread makes 4
// consecutive pixels of a crop row and stores them as k_raster and
// k_obj_coords store theirs: RGB as three dwords, the mask as one, the
// coordinates as three 8-B stores, the depth as one 16-B store, all
// non-temporal (written once, never read back here).  Source reads are direct
// global gathers: neighbouring lanes read neighbouring or identical pixels and
// a crop's window is reused across its rows from cache.  Sample positions are
// tested against the frame as floats before they become integers, so no window
// (NaN, infinite or far away) yields an index outside the frame.  Under the
// area filter the RGB of minified slots is k_crop_area's and is skipped here.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rgb_tap(const uint8_t* __restrict__ fr, int x, int y, uint32_t W, uint32_t H) {
  if ((uint32_t)x >= W || (uint32_t)y >= H) return 0u;
  const uint8_t* p = fr + ((size_t)y * W + (uint32_t)x) * 3;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

__device__ __forceinline__ uint32_t blend(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t wx, uint32_t wy,
                                          uint32_t shift) {
  const uint32_t top = ((a >> shift) & 255u) * (256u - wx) + ((b >> shift) & 255u) * wx;
  const uint32_t bot = ((c >> shift) & 255u) * (256u - wx) + ((d >> shift) & 255u) * wx;
  return (top * (256u - wy) + bot * wy + 32768u) >> 16;
}

__global__ __launch_bounds__(kCropBlock) void k_crop_sample(CropArgs a, uint32_t f0) {
  const uint32_t S = a.S, qrow = S >> 2;
  const uint32_t q = blockIdx.x * kCropBlock + threadIdx.x;
  if (q >= qrow * S) return;
  const uint32_t k = blockIdx.y, f = f0 + blockIdx.z;
  const size_t slot = (size_t)f * a.K + k;
  const CropSlot sl = a.info[slot];
  const size_t o = slot * S * S + 4u * (size_t)q;   // the thread's first crop pixel
  if (!slot_live(a, sl)) {   // block-uniform: the whole slot is zeros, its depth +inf
    if (a.crop_rgb) __builtin_nontemporal_store(v3u32{0u, 0u, 0u}, reinterpret_cast<v3u32*>(a.crop_rgb + o * 3));
    if (a.crop_mask) __builtin_nontemporal_store(0u, reinterpret_cast<uint32_t*>(a.crop_mask + o));
    if (a.crop_coords) {
#pragma unroll
      for (int t = 0; t < 3; ++t)
        __builtin_nontemporal_store(v2u32{0u, 0u}, reinterpret_cast<v2u32*>(a.crop_coords + o * 3 + 4 * t));
    }
    if (a.crop_depth)
      __builtin_nontemporal_store(v4f32{INFINITY, INFINITY, INFINITY, INFINITY},
                                  reinterpret_cast<v4f32*>(a.crop_depth + o));
    return;
  }
  const uint32_t W = a.W, H = a.H;
  const float fW = (float)W, fH = (float)H;
  const size_t fpx = (size_t)f * W * H;             // the frame's first pixel
  const uint32_t j = q / qrow, i0 = (q - j * qrow) * 4u;
  const float step = crop_step(sl, S);
  const float sy = crop_sample_pos(sl.y0, j, step);
  const bool yin = crop_sample_in(sy, fH);          // floorf(sy) in [0, H)
  const uint32_t py = yin ? (uint32_t)floorf(sy) : 0u;
  const float ty = sy - 0.5f;
  const bool yv = ty >= -1.0f && ty < fH;           // a tap row may lie in the frame
  const float yl = yv ? floorf(ty) : -2.0f;
  const uint32_t wy = yv ? (uint32_t)(int)((ty - yl) * 256.0f) : 0u;
  const bool own_rgb = a.crop_rgb && !slot_area(a, sl);   // block-uniform: k_crop_area makes the others
  const uint8_t* rgb = own_rgb ? a.rgb + fpx * 3 : nullptr;
  uint32_t c[4] = {0u, 0u, 0u, 0u}, m = 0u, h[12];
  float d[4];
#pragma unroll
  for (uint32_t t = 0; t < 4; ++t) {
    const float sx = crop_sample_pos(sl.x0, i0 + t, step);
    const bool in = yin && crop_sample_in(sx, fW);
    const size_t at = fpx + (size_t)py * W + (in ? (uint32_t)floorf(sx) : 0u);
    const bool hit = in && a.instance[at] == sl.label;
    m |= hit ? (255u << (8 * t)) : 0u;
    h[3 * t] = h[3 * t + 1] = h[3 * t + 2] = 0u;
    if (a.crop_coords && hit) {
      const uint16_t* u = a.obj_coords + at * 3;
      h[3 * t] = u[0];
      h[3 * t + 1] = u[1];
      h[3 * t + 2] = u[2];
    }
    d[t] = (a.crop_depth && hit) ? a.depth[at] : INFINITY;
    if (rgb) {
      const float tx = sx - 0.5f;
      const bool xv = yv && tx >= -1.0f && tx < fW;
      if (xv) {
        const float xl = floorf(tx);
        const uint32_t wx = (uint32_t)(int)((tx - xl) * 256.0f);
        const int x = (int)xl, y = (int)yl;
        const uint32_t p00 = rgb_tap(rgb, x, y, W, H), p10 = rgb_tap(rgb, x + 1, y, W, H);
        const uint32_t p01 = rgb_tap(rgb, x, y + 1, W, H), p11 = rgb_tap(rgb, x + 1, y + 1, W, H);
        c[t] = blend(p00, p10, p01, p11, wx, wy, 0) | (blend(p00, p10, p01, p11, wx, wy, 8) << 8) |
               (blend(p00, p10, p01, p11, wx, wy, 16) << 16);
      }
    }
  }
  if (own_rgb)
    __builtin_nontemporal_store(v3u32{c[0] | (c[1] << 24), (c[1] >> 8) | (c[2] << 16), (c[2] >> 16) | (c[3] << 8)},
                                reinterpret_cast<v3u32*>(a.crop_rgb + o * 3));
  if (a.crop_mask) __builtin_nontemporal_store(m, reinterpret_cast<uint32_t*>(a.crop_mask + o));
  if (a.crop_coords) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
      __builtin_nontemporal_store(v2u32{h[4 * t] | (h[4 * t + 1] << 16), h[4 * t + 2] | (h[4 * t + 3] << 16)},
                                  reinterpret_cast<v2u32*>(a.crop_coords + o * 3 + 4 * t));
  }
  if (a.crop_depth)
    __builtin_nontemporal_store(v4f32{d[0], d[1], d[2], d[3]}, reinterpret_cast<v4f32*>(a.crop_depth + o));
}

// ---------------------------------------------------------------------------
// k_crop_area: grid (bands of kAreaRows crop rows, K, frames); a workgroup owns
// one slot and one band, a thread the crop columns tid, tid + 128, ... of it.
// The workgroup walks the source rows of its band once: for each row every
// thread forms the horizontal sums sum_p wx(p) * c[r][p] of its columns (three
// channels, 32 bits) and adds them, weighted by wy, into the 64-bit accumulators
// of the crop row it is on.  A source row that straddles two crop rows is summed
// once and added to both (`rc` remembers the row the sums are of), so a window's
// in-frame pixels are loaded once per band and only a band's boundary rows
// twice.  Neighbouring lanes read neighbouring segments of the row straight
// from global memory (staging the segments in LDS behind two barriers per row
// took half as long again on the C3 crops).  All row and column ranges are clipped to the frame before
// their loops start: a slot costs its in-frame pixels plus its outputs, however
// large the window, and no index leaves the frame.  All control flow but the
// column ranges is block-uniform.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int32_t area_edge(float origin, uint32_t i, float step) {
  return (int32_t)floorf((origin + (float)i * step) * 256.0f);   // |.| < 2^29 under slot_area's bounds
}

// (num + (den >> 1)) / den for a quotient of at most 255: an f32 estimate is
// within 1 of it, and one 64-bit multiply and compare in each direction makes it exact.
__device__ __forceinline__ uint32_t area_round_div(uint64_t acc, uint64_t den) {
  const uint64_t num = acc + (den >> 1);
  uint32_t q = (uint32_t)((float)num * __builtin_amdgcn_rcpf((float)den));
  if ((uint64_t)q * den > num) --q;
  else if ((uint64_t)(q + 1u) * den <= num) ++q;
  return q;
}

template <uint32_t kCols>   // crop columns per thread: S <= kCols * kAreaBlock
__global__ __launch_bounds__(kAreaBlock) void k_crop_area(CropArgs a, uint32_t f0) {
  const uint32_t S = a.S, k = blockIdx.y, f = f0 + blockIdx.z;
  const size_t slot = (size_t)f * a.K + k;
  const CropSlot sl = a.info[slot];
  if (!slot_live(a, sl) || !slot_area(a, sl)) return;   // block-uniform: k_crop_sample makes this slot's RGB
  const int32_t W = (int32_t)a.W, H = (int32_t)a.H;
  const float step = sl.side / (float)S;
  const uint8_t* fr = a.rgb + (size_t)f * a.W * a.H * 3;
  uint8_t* out = a.crop_rgb + slot * S * S * 3;
  int32_t ex0[kCols], ex1[kCols], plo[kCols], phi[kCols];
  uint32_t h[kCols][3];
#pragma unroll
  for (uint32_t m = 0; m < kCols; ++m) {
    const uint32_t i = threadIdx.x + m * kAreaBlock;
    ex0[m] = ex1[m] = plo[m] = phi[m] = 0;
    h[m][0] = h[m][1] = h[m][2] = 0u;
    if (i < S) {
      ex0[m] = area_edge(sl.x0, i, step);
      ex1[m] = area_edge(sl.x0, i + 1u, step);
      plo[m] = max(ex0[m] >> 8, 0);
      phi[m] = min((ex1[m] + 255) >> 8, W);
    }
  }
  const uint32_t j0 = blockIdx.x * kAreaRows, j1 = min(j0 + kAreaRows, S);
  const uint32_t quad = threadIdx.x & 60u;   // first lane of the thread's 4 lanes (within its wave)
  int32_t rc = -1;                           // the source row h[][] holds the sums of
  int32_t ey0 = area_edge(sl.y0, j0, step);
  for (uint32_t j = j0; j < j1; ++j) {
    const int32_t ey1 = area_edge(sl.y0, j + 1u, step);
    const int32_t rlo = max(ey0 >> 8, 0), rhi = min((ey1 + 255) >> 8, H);
    uint64_t acc[kCols][3];
#pragma unroll
    for (uint32_t m = 0; m < kCols; ++m) acc[m][0] = acc[m][1] = acc[m][2] = 0u;
    for (int32_t r = rlo; r < rhi; ++r) {
      const uint8_t* row = fr + (size_t)r * a.W * 3;
      const uint32_t wy = (uint32_t)(min(ey1, (r + 1) << 8) - max(ey0, r << 8));
#pragma unroll
      for (uint32_t m = 0; m < kCols; ++m) {
        if (m * kAreaBlock >= S) break;   // block-uniform
        if (r != rc) {
          uint32_t s0 = 0u, s1 = 0u, s2 = 0u;
          for (int32_t p = plo[m]; p < phi[m]; ++p) {
            const uint32_t wx = (uint32_t)(min(ex1[m], (p + 1) << 8) - max(ex0[m], p << 8));
            const uint8_t* c = row + (size_t)p * 3;
            s0 += wx * c[0];
            s1 += wx * c[1];
            s2 += wx * c[2];
          }
          h[m][0] = s0;
          h[m][1] = s1;
          h[m][2] = s2;
        }
        acc[m][0] += (uint64_t)wy * h[m][0];
        acc[m][1] += (uint64_t)wy * h[m][1];
        acc[m][2] += (uint64_t)wy * h[m][2];
      }
      rc = r;
    }
    const int32_t dy = ey1 - ey0;
#pragma unroll
    for (uint32_t m = 0; m < kCols; ++m) {
      if (m * kAreaBlock >= S) break;     // block-uniform
      const uint32_t i = threadIdx.x + m * kAreaBlock;
      const int32_t dx = ex1[m] - ex0[m];
      uint32_t px = 0u;
      if (dx > 0 && dy > 0) {
        const uint64_t den = (uint64_t)(uint32_t)dx * (uint32_t)dy;
        px = area_round_div(acc[m][0], den) | (area_round_div(acc[m][1], den) << 8) |
             (area_round_div(acc[m][2], den) << 16);
      }
      // four lanes hold crop pixels i .. i + 3 (S is a multiple of 4): the first stores them as three dwords
      const uint32_t c0 = __shfl(px, quad), c1 = __shfl(px, quad + 1u), c2 = __shfl(px, quad + 2u),
                     c3 = __shfl(px, quad + 3u);
      if ((threadIdx.x & 3u) == 0u && i < S)
        __builtin_nontemporal_store(v3u32{c0 | (c1 << 24), (c1 >> 8) | (c2 << 16), (c2 >> 16) | (c3 << 8)},
                                    reinterpret_cast<v3u32*>(out + ((size_t)j * S + i) * 3));
    }
    ey0 = ey1;
  }
}

}  // namespace

void launch_crop_plan(const CropArgs& a, uint32_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_crop_plan, dim3(n), dim3(kCropBlock), 0, st, a);
}

void launch_crop_sample(const CropArgs& a, uint32_t n, hipStream_t st) {
  const uint32_t quads = a.S * a.S / 4u;
  for (uint32_t f0 = 0; f0 < n; f0 += 65535u) {   // grid z limit
    const uint32_t nf = n - f0 < 65535u ? n - f0 : 65535u;
    hipLaunchKernelGGL(k_crop_sample, dim3((quads + kCropBlock - 1) / kCropBlock, a.K, nf), dim3(kCropBlock), 0, st, a,
                       f0);
  }
}

void launch_crop_area(const CropArgs& a, uint32_t n, hipStream_t st) {
  const uint32_t bands = (a.S + kAreaRows - 1) / kAreaRows;
  for (uint32_t f0 = 0; f0 < n; f0 += 65535u) {   // grid z limit
    const uint32_t nf = n - f0 < 65535u ? n - f0 : 65535u;
    const dim3 grid(bands, a.K, nf);
    switch ((a.S + kAreaBlock - 1) / kAreaBlock) {   // columns per thread (S <= 512)
      case 1: hipLaunchKernelGGL(k_crop_area<1>, grid, dim3(kAreaBlock), 0, st, a, f0); break;
      case 2: hipLaunchKernelGGL(k_crop_area<2>, grid, dim3(kAreaBlock), 0, st, a, f0); break;
      case 3: hipLaunchKernelGGL(k_crop_area<3>, grid, dim3(kAreaBlock), 0, st, a, f0); break;
      default: hipLaunchKernelGGL(k_crop_area<4>, grid, dim3(kAreaBlock), 0, st, a, f0); break;
    }
  }
}

}  // namespace csg
