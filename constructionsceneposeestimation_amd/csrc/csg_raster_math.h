// csg_raster_math.h -- device code shared by the kernels that must land on the
// same fragments: the render (csg_kernels.hip: k_setup, k_raster, the crop
// amodal passes) and the full-frame amodal planes (csg_amodal_spans.hip).  The
// arithmetic follows DESIGN.md "Raster spec" and oracle/csg_oracle.c line by
// line; every translation unit that includes this is built with
// -ffp-contract=off.  Device only.
#pragma once
#include <math.h>

#include "csg_alpha_cut.h"
#include "csg_kernels.h"

namespace csg {

constexpr int kSmallCover = 4;   // records with at most 4 x 4 pixel centres get an exact cover test in k_setup
constexpr float kGuardPx = 1048576.0f;

// ---------------------------------------------------------------------------
// shared arithmetic (mirrors csg_oracle.c line by line)
// ---------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));   // packed FP32 pair (v_pk_*_f32)

__device__ __forceinline__ float dot4(const float* r, float x, float y, float z) {
  return ((r[0] * x + r[1] * y) + r[2] * z) + r[3];
}

__device__ __forceinline__ void mat4_mul(const float* a, const float* b, float* c) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      c[i * 4 + j] = ((a[i * 4 + 0] * b[0 * 4 + j] + a[i * 4 + 1] * b[1 * 4 + j]) + a[i * 4 + 2] * b[2 * 4 + j]) +
                     a[i * 4 + 3] * b[3 * 4 + j];
}

// 1.0f / x, bit-identical to the IEEE division for |x| in [2^-126, 2^126]:
// the hardware reciprocal (~1 ulp) plus one Newton step with an exact FMA
// residual, 3 VALU instead of the division's 11 (v_div_scale x2, v_rcp, 6 FMAs,
// v_div_fmas, v_div_fixup).  Checked exhaustively on the MI355X over every
// normal float of both signs (tools/rcp_check.hip, profiles/r04/rcp_check.json):
// the only differences are the 2 x (2^24 - 1) x with |x| > 2^126, whose
// reciprocal is subnormal.  k_raster's inverse depths lie in [1/far, 1/near],
// inside the range (csg_create keeps near / far clip in [2^-126, 2^126]).
// k_setup uses it for the per-vertex 1/W (W >= near_clip after near-plane
// clipping; setup -1.9%, profiles/r04/ab/setup_w_rcp.txt) and, range-checked,
// for 1/det (hom_setup: -0.5%, profiles/r04/ab/det_rcp.txt); the near-plane
// crossing is a true quotient and stays a division.  (Round 4's first
// attempt, every k_setup division range-checked at once, measured 3% slower:
// profiles/r04/ab/rcp_packed_smallcover.txt.)  CSG_FAST_RCP=0 builds the
// division (A/B).
#ifndef CSG_FAST_RCP
#define CSG_FAST_RCP 1
#endif
__device__ __forceinline__ float rcp_ieee(float x) {
#if CSG_FAST_RCP
  const float r0 = __builtin_amdgcn_rcpf(x);
  const float e = __builtin_fmaf(-x, r0, 1.0f);
  return __builtin_fmaf(e, r0, r0);
#else
  return 1.0f / x;
#endif
}

struct Cv3 { float x, y, w; };

struct Hom {
  float A[3], B[3], C[3];
  float invdet;
  bool ok;
};

__device__ __forceinline__ void hom_setup(const Cv3* v, Hom& h) {
  const int ea[3] = {1, 2, 0}, eb[3] = {2, 0, 1};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const Cv3 a = v[ea[k]], b = v[eb[k]];
    h.A[k] = a.y * b.w - a.w * b.y;
    h.B[k] = a.w * b.x - a.x * b.w;
    h.C[k] = a.x * b.y - a.y * b.x;
  }
  const float det = (v[0].x * h.A[0] + v[0].y * h.B[0]) + v[0].w * h.C[0];
  h.ok = det != 0.0f;
  // 1/det: the Newton reciprocal inside its proven range, the division outside
  const float ad = fabsf(det);
  h.invdet = !h.ok ? 0.0f : (ad >= 0x1p-126f && ad <= 0x1p126f) ? rcp_ieee(det) : 1.0f / det;
}

// Screen-space planes of the original triangle (spec §3.5-6), from its
// homogeneous edge rows: with e_k = A_k*x + B_k*y + C_k, 1/W = invdet * sum e_k
// and u/W = invdet * sum e_k u_k are affine in (x, y):
//   D = (((A0 + A1) + A2) * invdet, (B...) * invdet, (C...) * invdet)
//   U = (((A0*u0 + A1*u1) + A2*u2) * invdet, ...), V likewise with v.
// uv = u0 v0 u1 v1 u2 v2.
__device__ __forceinline__ void depth_plane(const float* A, const float* B, const float* C, float invdet, float* D) {
  D[0] = ((A[0] + A[1]) + A[2]) * invdet;
  D[1] = ((B[0] + B[1]) + B[2]) * invdet;
  D[2] = ((C[0] + C[1]) + C[2]) * invdet;
}
__device__ __forceinline__ void uv_planes(const float* A, const float* B, const float* C, float invdet,
                                          const float* uv, float* U, float* V) {
  U[0] = ((A[0] * uv[0] + A[1] * uv[2]) + A[2] * uv[4]) * invdet;
  U[1] = ((B[0] * uv[0] + B[1] * uv[2]) + B[2] * uv[4]) * invdet;
  U[2] = ((C[0] * uv[0] + C[1] * uv[2]) + C[2] * uv[4]) * invdet;
  V[0] = ((A[0] * uv[1] + A[1] * uv[3]) + A[2] * uv[5]) * invdet;
  V[1] = ((B[0] * uv[1] + B[1] * uv[3]) + B[2] * uv[5]) * invdet;
  V[2] = ((C[0] * uv[1] + C[1] * uv[3]) + C[2] * uv[5]) * invdet;
}

// A plane at pixel centre (fx, fy) = (px + 0.5, py + 0.5).
__device__ __forceinline__ float plane_at(float p0, float p1, float p2, float fx, float fy) {
  return (p0 * fx + p1 * fy) + p2;
}

// Bilinear RGBA8, repeat wrap, 8-bit fixed weights (v flipped: row 0 = top).
struct TexTap { uint32_t i00, i10, i01, i11; int wx, wy; };

// fu mod n in [0, n) for an integer-valued |fu| < 2^23, without an integer
// division: q may be off by one (approximate reciprocal), one correction fixes
// it; q*n and fu - q*n are integers below 2^24, so every step is exact.
__device__ __forceinline__ int wrap_index(float fu, int n) {
  const float nf = (float)n;
  // Texture coordinates inside one repeat (the usual case: uvs in [0, 1])
  // need no reduction; the branch is skipped when no lane of the wave wraps.
  if (fu >= 0.0f && fu < nf) return (int)fu;
  const float q = floorf(fu * __builtin_amdgcn_rcpf(nf));
  float r = fu - q * nf;
  r += r < 0.0f ? nf : 0.0f;
  r -= r >= nf ? nf : 0.0f;
  return (int)r;
}

// Texel coordinates (u * tw - 0.5, (1 - v) * th - 0.5) as one packed multiply and add
__device__ __forceinline__ f32x2 texel_coords(float u, float v, int tw, int th) {
  const f32x2 a = {u, 1.0f - v}, n = {(float)tw, (float)th};
  return a * n - 0.5f;
}

__device__ __forceinline__ TexTap tex_taps(int tw, int th, float u, float v) {   // tw, th <= 16384
  const f32x2 t2 = texel_coords(u, v, tw, th);
  float tu = t2.x, tv = t2.y;
  if (!(fabsf(tu) < 8388608.0f)) tu = 0.0f;
  if (!(fabsf(tv) < 8388608.0f)) tv = 0.0f;
  const float fu = floorf(tu), fv = floorf(tv);
  TexTap t;
  // tu - fu is exact and in [0, 1), so the weights are in [0, 255] and the
  // wrapped indices below 16384 (upload limit): the masks change no value,
  // they let the compiler use full-rate 24-bit multiplies
  t.wx = (int)((tu - fu) * 256.0f) & 255;
  t.wy = (int)((tv - fv) * 256.0f) & 255;
  tw &= 0x7FFF;
  const int x0 = wrap_index(fu, tw) & 0x3FFF, y0 = wrap_index(fv, th) & 0x3FFF;
  const int x1 = (x0 + 1 == tw) ? 0 : x0 + 1;
  const int y1 = (y0 + 1 == th) ? 0 : y0 + 1;
  const uint32_t r0 = __umul24((uint32_t)y0, (uint32_t)tw), r1 = __umul24((uint32_t)y1, (uint32_t)tw);
  t.i00 = r0 + (uint32_t)x0; t.i10 = r0 + (uint32_t)x1;
  t.i01 = r1 + (uint32_t)x0; t.i11 = r1 + (uint32_t)x1;
  return t;
}

// Operands are below 2^24 (channels <= 255, weights <= 256), so every
// product is a full-rate 24-bit multiply (a plain int multiply here becomes
// the quarter-rate v_mul_lo_u32).
__device__ __forceinline__ int bilerp8(uint32_t c00, uint32_t c10, uint32_t c01, uint32_t c11, int wx, int wy) {
  const uint32_t ax = 256u - (uint32_t)wx, ay = 256u - (uint32_t)wy;
  const uint32_t top = __umul24(c00, ax) + __umul24(c10, (uint32_t)wx);
  const uint32_t bot = __umul24(c01, ax) + __umul24(c11, (uint32_t)wx);
  return (int)((__umul24(top, ay) + __umul24(bot, (uint32_t)wy) + 32768u) >> 16);
}

// x / 255 for 0 <= x < 2^16 (exhaustively equal), one 24-bit multiply
__device__ __forceinline__ int div255(uint32_t x) { return (int)(__umul24(x, 32897u) >> 23); }

__device__ __forceinline__ int tex_channel(uint32_t c00, uint32_t c10, uint32_t c01, uint32_t c11, int sh, int wx,
                                           int wy) {
  return bilerp8((c00 >> sh) & 255u, (c10 >> sh) & 255u, (c01 >> sh) & 255u, (c11 >> sh) & 255u, wx, wy);
}

__device__ __forceinline__ void tex_sample(const SceneDev& s, int tid, float u, float v, int out[4]) {
  const TexDesc t = s.texd[tid];
  const TexTap k = tex_taps((int)t.width, (int)t.height, u, v);
  const uint32_t* base = reinterpret_cast<const uint32_t*>(s.texels) + t.offset;
  const uint32_t c00 = base[k.i00], c10 = base[k.i10], c01 = base[k.i01], c11 = base[k.i11];
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c] = tex_channel(c00, c10, c01, c11, 8 * c, k.wx, k.wy);
}

// The alpha test: bilinear alpha (8-bit weights, as tex_sample) > thr.
// The alpha-quad image holds at texel (x, y) the alphas of (x,y), (x+1,y),
// (x,y+1), (x+1,y+1) (wrapped), so the bilinear footprint is one 4-byte load.
// First the 2-bit class of that quad (acls, 16 per word, 1/16 of the quad
// image, so it stays in L2): all four alphas <= thr -> the filtered value is
// too (weights sum to 65536 and the rounding cannot cross an integer), fail;
// all four > thr -> pass; only mixed quads (~5% of a foliage card's texels)
// load the quad and filter.  `wh` = width | height << 16.
__device__ __forceinline__ bool alpha_pass(const uint32_t* aquad, const uint32_t* acls, uint32_t offset, uint32_t wh,
                                           int thr, float u, float v) {
  const int tw = (int)(wh & 0xFFFFu), th = (int)(wh >> 16);
  const f32x2 t2 = texel_coords(u, v, tw, th);
  float tu = t2.x, tv = t2.y;
  if (!(fabsf(tu) < 8388608.0f)) tu = 0.0f;
  if (!(fabsf(tv) < 8388608.0f)) tv = 0.0f;
  const float fu = floorf(tu), fv = floorf(tv);
  const uint32_t idx = offset + __umul24((uint32_t)wrap_index(fv, th) & 0x3FFFu, (uint32_t)tw & 0x7FFFu) +
                       ((uint32_t)wrap_index(fu, tw) & 0x3FFFu);   // (masks: see tex_taps)
  const uint32_t cl = (acls[idx >> 4] >> (2u * (idx & 15u))) & 3u;
  if (cl != 3u) return cl != 0u;
  const int wx = (int)((tu - fu) * 256.0f) & 255, wy = (int)((tv - fv) * 256.0f) & 255;
  const uint32_t q = aquad[idx];
  return bilerp8(q & 255u, (q >> 8) & 255u, (q >> 16) & 255u, q >> 24, wx, wy) > thr;
}

// Build one raster record from screen-space vertices; false if it covers no pixel.
// Groups 0-1 of a raster record (x0 x1 x2 y0 | y1 y2 p0 p1): the part that
// differs between the sub-triangles of one clipped triangle.
struct SubRec { uint4 g0, g1; };

__device__ __forceinline__ bool make_rec(const SceneDev& s, const float* su, const float* sv, SubRec& r) {
  int32_t x[3], y[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!(fabsf(su[k]) < kGuardPx) || !(fabsf(sv[k]) < kGuardPx)) return false;
    x[k] = (int32_t)rintf(su[k] * 256.0f);
    y[k] = (int32_t)rintf(sv[k] * 256.0f);
  }
  const int64_t area = (int64_t)(x[1] - x[0]) * (y[2] - y[0]) - (int64_t)(x[2] - x[0]) * (y[1] - y[0]);
  if (area == 0) return false;
  if (area < 0) {
    int32_t t = x[1]; x[1] = x[2]; x[2] = t;
    t = y[1]; y[1] = y[2]; y[2] = t;
  }
  const int32_t xmin = min(x[0], min(x[1], x[2])), xmax = max(x[0], max(x[1], x[2]));
  const int32_t ymin = min(y[0], min(y[1], y[2])), ymax = max(y[0], max(y[1], y[2]));
  int px0 = (xmin - 128 + 255) >> 8, px1 = (xmax - 128) >> 8;
  int py0 = (ymin - 128 + 255) >> 8, py1 = (ymax - 128) >> 8;
  px0 = max(px0, 0);
  py0 = max(py0, 0);
  px1 = min(px1, (int)s.W - 1);
  py1 = min(py1, (int)s.H - 1);
  if (px0 > px1 || py0 > py1) return false;
  // Small records (at most NxN pixel centres in the box, vertex extent below
  // 32 px): evaluate the spec's edge test at every centre of the box, drop the
  // record if it covers none and shrink the box to the covered pixels.  The
  // covered set is unchanged (so are the outputs); fewer, tighter records mean
  // fewer record stores, bin entries and raster row items.  Exact in int32:
  // |dx|, |dy| < 2^13 and every centre lies within the vertex extent.
  constexpr int N = kSmallCover;
  if (px1 - px0 < N && py1 - py0 < N && xmax - xmin < 8192 && ymax - ymin < 8192) {
    const int32_t cx0 = px0 * 256 + 128, cy0 = py0 * 256 + 128;
    const int ea[3] = {1, 2, 0}, eb[3] = {2, 0, 1};
    int32_t e0[3], sx[3], sy[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int32_t dx = x[eb[e]] - x[ea[e]], dy = y[eb[e]] - y[ea[e]];
      const int32_t bias = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
      e0[e] = __mul24(dx, cy0 - y[ea[e]]) - __mul24(dy, cx0 - x[ea[e]]) + bias;
      sx[e] = -dy * 256;
      sy[e] = dx * 256;
    }
    const int nw = px1 - px0, nh = py1 - py0;
    uint32_t cols = 0, rows = 0;
    // the active lanes' largest box, wave-uniform: a wave of 1x1 and 2x2 boxes
    // evaluates 1 or 4 centres, not N*N
    int nwm = 0, nhm = 0;
#pragma unroll
    for (int k = 1; k < N; ++k) {
      nwm += __any(nw >= k) ? 1 : 0;
      nhm += __any(nh >= k) ? 1 : 0;
    }
    // E(i, j) = e0 + sx*i + sy*j stepped by additions (the same integers; a
    // constant multiple such as sx*3 otherwise became a quarter-rate v_mul_lo_u32)
    int32_t er[3] = {e0[0], e0[1], e0[2]};
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if (j > nhm) break;
      int32_t ec[3] = {er[0], er[1], er[2]};
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if (i > nwm) break;
        const bool in = i <= nw && j <= nh && (ec[0] | ec[1] | ec[2]) >= 0;
        cols |= in ? 1u << i : 0u;
        rows |= in ? 1u << j : 0u;
#pragma unroll
        for (int e = 0; e < 3; ++e) ec[e] += sx[e];
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) er[e] += sy[e];
    }
    if (!cols) return false;
    px1 = px0 + 31 - __clz(cols);
    px0 += __ffs(cols) - 1;
    py1 = py0 + 31 - __clz(rows);
    py0 += __ffs(rows) - 1;
  }
  r.g0 = make_uint4((uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], (uint32_t)y[0]);
  r.g1 = make_uint4((uint32_t)y[1], (uint32_t)y[2], (uint32_t)px0 | ((uint32_t)py0 << 16),
                    (uint32_t)px1 | ((uint32_t)py1 << 16));
  return true;
}

// ---------------------------------------------------------------------------
// Alpha trim: k_setup shrinks the pixel box of an
// alpha-tested record to the pixels whose (u, v) can fall inside the
// triangle's opaque uv box (csg_alpha_box.h): the guards below, then the cut
// (csg_alpha_cut.h: the snapped triangle clipped by the box's four half-planes).
// Every dropped pixel centre
// provably fails alpha_pass as k_raster's fragment() evaluates it, so no output
// changes.  Only unclipped triangles are trimmed (one record, whose covered
// pixel centres lie inside the snapped triangle).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float rcp_w(float w);
constexpr float kTrimEps = 0x1p-20f;   // 4x the rounding of any expression bounded below (at most 2^-22 of its magnitude sum)

// The guards.  `v` are the clip-space vertices (W >= near), uv their texture
// coordinates, U V D the record's planes, T = max(tw, th).  With
//   X, Y   >= |x|, |y| of every vertex, snapped vertex and covered pixel centre,
//   S, Sd  = magnitude sums |P0| X + |P1| Y + |P2| of the uv planes (the larger) and of D,
//   umax   >= |u|, |v| of every covered pixel,
// it returns true only if
//   dmin > 0 bounds the real-valued D below at the three snapped vertices, hence
//     (D is affine, a covered centre is a convex combination of them) at every
//     covered pixel, where u = U / D is then a convex combination of the vertices'
//     U / D as well;
//   (b) the real-valued U / D, V / D at each snapped vertex are within 1 / T
//     of the vertex's uv, so every covered pixel's real (u, v) lies within one
//     texel of the true uv triangle;
//   (a) the (u, v) that fragment() computes and the texel coordinates alpha_pass
//     derives from them differ from the real values by at most 1/4 texel.
// `m` bounds twice over the rounding of a half-plane (U - bound * D)(x, y)
// evaluated in float at any centre of the box, for |bound| <= B.
__device__ __forceinline__ bool alpha_trim_guard(const Cv3* v, const float* uv, const float* U, const float* V,
                                                 const float* D, float T, float B, float& m) {
  float su[3], sv[3], X = 0.0f, Y = 0.0f, umax = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float r = rcp_w(v[k].w);
    su[k] = v[k].x * r;
    sv[k] = v[k].y * r;
    X = fmaxf(X, fabsf(su[k]));
    Y = fmaxf(Y, fabsf(sv[k]));
    umax = fmaxf(umax, fmaxf(fabsf(uv[2 * k]), fabsf(uv[2 * k + 1])));
  }
  X += 1.0f;
  Y += 1.0f;
  umax += 2.0f;
  const float Sd = (fabsf(D[0]) * X + fabsf(D[1]) * Y) + fabsf(D[2]);
  const float S = fmaxf((fabsf(U[0]) * X + fabsf(U[1]) * Y) + fabsf(U[2]), (fabsf(V[0]) * X + fabsf(V[1]) * Y) + fabsf(V[2]));
  // a plane at the snapped vertex (within 1/512 px of su, sv) against its float value at (su, sv)
  const float dD = kTrimEps * Sd + (fabsf(D[0]) + fabsf(D[1])) * (1.0f / 256.0f);
  const float dU = kTrimEps * S + fmaxf(fabsf(U[0]) + fabsf(U[1]), fabsf(V[0]) + fabsf(V[1])) * (1.0f / 256.0f);
  float dmin = INFINITY, res = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float Dk = plane_at(D[0], D[1], D[2], su[k], sv[k]);
    const float Uk = plane_at(U[0], U[1], U[2], su[k], sv[k]), Vk = plane_at(V[0], V[1], V[2], su[k], sv[k]);
    dmin = fminf(dmin, Dk);
    res = fmaxf(res, fmaxf(fabsf(Uk - uv[2 * k] * Dk), fabsf(Vk - uv[2 * k + 1] * Dk)));
  }
  dmin -= dD;
  if (!(dmin >= 0x1p-100f)) return false;
  if (!(((res + dU) + umax * dD) * T <= dmin)) return false;                                           // (b)
  if (!(kTrimEps * T * ((S + umax * Sd) + (umax + 1.0f) * dmin) <= 0.25f * dmin)) return false;      // (a)
  m = kTrimEps * (S + B * Sd);
  return m < INFINITY;
}

// q / w for q < 2^24, 1 <= w <= 256: float reciprocal estimate (off by at
// most one), then one exact correction (no integer division sequence)
__device__ __forceinline__ uint32_t small_div(uint32_t q, uint32_t w) {
  uint32_t d = (uint32_t)((float)q * __builtin_amdgcn_rcpf((float)w));
  const uint32_t p = __umul24(d, w);
  d = p > q ? d - 1u : (p + w <= q ? d + 1u : d);
  return d;
}

// Chunk cull of one (frame, chunk): true if all 8 corners of the chunk's
// object-space AABB fail one frustum plane by a margin -- then every triangle
// inside would fail that plane in the per-triangle test too, so the output is
// unchanged.  Corner c of the box (x from bit 2, y bit 1, z bit 0).  (Measured:
// per-64-triangle slice AABBs cull more but cost more than they save.)
struct CullOut { bool n, f, l, r, t, b; };
__device__ __forceinline__ CullOut corner_out(const SceneDev& s, const Chunk& ch, const float* Cm, int c) {
  const float px = (c & 4) ? ch.hi[0] : ch.lo[0];
  const float py = (c & 2) ? ch.hi[1] : ch.lo[1];
  const float pz = (c & 1) ? ch.hi[2] : ch.lo[2];
  const float X = dot4(Cm + 0, px, py, pz), Y = dot4(Cm + 4, px, py, pz), Wc = dot4(Cm + 8, px, py, pz);
  const float tol = 1e-3f * (fabsf(X) + fabsf(Y) + fabsf(Wc)) + 1e-3f;
  return CullOut{Wc < s.near_clip - tol, Wc > s.far_clip + tol, X < -tol, X > (float)s.W * Wc + tol * (float)s.W,
                 Y < -tol, Y > (float)s.H * Wc + tol * (float)s.H};
}

// The spec's per-vertex 1/W (spec 3): W >= near_clip > 2^-126 after near-plane
// clipping, so below 2^126 the Newton reciprocal is the IEEE one (rcp_ieee);
// the division only past that (never taken by real scenes: a uniform branch)
__device__ __forceinline__ float rcp_w(float w) { return w <= 0x1p126f ? rcp_ieee(w) : 1.0f / w; }

constexpr uint32_t kAmSerial = 16;   // samples a lane tests itself
constexpr uint32_t kAmQueue = 64;    // larger sub-triangles queued per round
constexpr int32_t kAmPast = 0x7FFFFFFF;   // colpx / rowpy of a sample past the frame's far edge

struct AmTri {   // what the sample test needs of one raster sub-triangle
  int32_t x[3], y[3];          // 24.8 fixed point, positive orientation (make_rec)
  float D[3], U[3], V[3];      // planes of the original triangle
  uint32_t atex, wh, thr;      // alpha test (kNoAlpha: none)
  uint32_t i0, ni, j0, nj;     // sample rectangle
};

// Spec §3.3 / §3.5 / §3.6 at the centre of pixel (px, py): covered, in the depth range, alpha passed.
// With kKey a hit also leaves the bits of the fragment's 1/W in `key` (>= 1/far > 0, so never 0).
template <bool kKey>
__device__ __forceinline__ bool amodal_hit(const SceneDev& s, const AmTri& t, int32_t px, int32_t py, uint32_t& key) {
  const int32_t cx = px * 256 + 128, cy = py * 256 + 128;
  const int ea[3] = {1, 2, 0}, eb[3] = {2, 0, 1};
  bool in = true;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int32_t dx = t.x[eb[e]] - t.x[ea[e]], dy = t.y[eb[e]] - t.y[ea[e]];
    const int32_t bias = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
    in &= (int64_t)dx * (cy - t.y[ea[e]]) - (int64_t)dy * (cx - t.x[ea[e]]) + bias >= 0;
  }
  if (!in) return false;
  const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
  const float invw = plane_at(t.D[0], t.D[1], t.D[2], fx, fy);
  if (!(invw >= s.inv_far && invw <= s.inv_near)) return false;
  if constexpr (kKey) key = __float_as_uint(invw);
  if (t.atex == kNoAlpha) return true;
  const float r = rcp_ieee(invw);   // invw in [1/far, 1/near]
  const float u = plane_at(t.U[0], t.U[1], t.U[2], fx, fy) * r, v = plane_at(t.V[0], t.V[1], t.V[2], fx, fy) * r;
  return alpha_pass(s.aquad, s.acls, t.atex, t.wh, (int)t.thr, u, v);
}

}  // namespace csg
