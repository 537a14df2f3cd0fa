// csg_alpha_cut.h -- the cut of the alpha trim ("The cut"):
// the pixel box of an alpha-tested record against the four half-planes of its
// triangle's opaque uv box, by clipping the snapped triangle, not its box.
// Compiles for the device (k_setup, through csg_raster_math.h) and for the host
// (tests/alpha_cut_host.cpp); both sides are built with -ffp-contract=off.
//
// One half-plane is g(x, y) = (h0 * x + h1 * y) + h2 with h = +-(P - bound * D)
// (P = U or V): the float expression alpha_cut_plane() below, the one the
// box cut before this evaluated at the ends of a column.  `m` (alpha_trim_guard)
// is at least four times the rounding of that expression at any point within the
// guard's X, Y, so with g^ the same coefficients evaluated in real arithmetic
// |g - g^| <= m / 4 at a pixel centre, and <= 0.32 m at a snapped vertex (whose
// float coordinates carry one more rounding).
//
// What is kept: every centre inside the snapped triangle T whose four float
// values are all >= -m.  Such a centre has g^ >= -1.25 m, so it lies in the
// convex polygon T n {g^ >= -1.25 m} of every half-plane, whose corners are the
// vertices of T on that side and the crossings of the edges that change side.
// Per half-plane the code boxes a superset of those corners:
//   - a vertex is IN when its float value is >= -2 m (kCutIn): a vertex with
//     g^ >= -1.25 m has a float value >= -1.57 m, so it is IN; an OUT vertex has
//     g^ < -1.68 m and is truly outside;
//   - on an edge with one end IN and one OUT the crossing is placed where the
//     float values, interpolated, reach -4 m (kCutLevel): s = (ga + 4m) / (ga -
//     gb) from a, clamped to [0, 1].  With |ga - gb| >= 8 m (kCutSmall) the real
//     crossing of g^ = -1.25 m lies on the IN side of that point even when
//     numerator and denominator are off by 0.32 m and 0.8 m and s by its own
//     rounding of 2^-22 (a slack of at least 1.26 m / |ga - gb| >= 2.5 * 2^-22);
//   - if |ga - gb| < 8 m the division decides nothing: the crossing is the OUT
//     end itself, i.e. both ends count as in;
//   - the crossing's coordinates a + s * (b - a) and the vertices' own float
//     coordinates are off by less than 2^-21 * X (Y): the extents are widened by
//     2^-20 * (max |x| + 1) (kCutWiden) before they are rounded to centres;
//   - an edge with both ends IN contributes a point of itself (harmless), one
//     with both ends OUT nothing; no vertex IN: no centre is kept, no record.
// The four boxes and the record's box are intersected.  Everything the code
// boxes lies in T n {g^ >= -12 m} (kCutOuter: an OUT end that counts as in has
// g^ >= -11.2 m), so the cut is also never looser than the exact clip at that
// level plus the widening.  If any of the twelve vertex values is NaN or
// infinite the box is returned unchanged.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CSG_CUT_FN __device__ __forceinline__
#else
#define CSG_CUT_FN inline
#endif

namespace csg {

constexpr float kCutIn = 2.0f, kCutLevel = 4.0f, kCutSmall = 8.0f, kCutOuter = 12.0f;   // times m, see above
constexpr float kCutWiden = 0x1p-20f;

// ~1 / x: the hardware reciprocal (1 ulp) on the device, the division on the host
CSG_CUT_FN float cut_rcp(float x) {
#if defined(__HIPCC__)
  return __builtin_amdgcn_rcpf(x);
#else
  return 1.0f / x;
#endif
}

CSG_CUT_FN int cut_imax(int a, int b) { return a > b ? a : b; }
CSG_CUT_FN int cut_imin(int a, int b) { return a < b ? a : b; }

// Half-plane k (0: u >= u_lo, 1: u <= u_hi, 2: v >= v_lo, 3: v <= v_hi, each times D > 0) at (x, y);
// P = U for k < 2, else V, and bd the bound.  (The negation is exact.)
CSG_CUT_FN float alpha_cut_plane(int k, const float* P, const float* D, float bd, float x, float y) {
  const float sg = (k & 1) ? -1.0f : 1.0f;
  const float h0 = sg * (P[0] - bd * D[0]), h1 = sg * (P[1] - bd * D[1]), h2 = sg * (P[2] - bd * D[2]);
  return (h0 * x + h1 * y) + h2;
}

// The record's pixel box (lo = px0 | py0 << 16, hi = px1 | py1 << 16, as the record stores it) against
// the opaque uv box bx = u_lo u_hi v_lo v_hi (finite).  xi, yi: the snapped 24.8 vertices.
// False: no pixel is left.
CSG_CUT_FN bool alpha_cut_box(int32_t xi0, int32_t xi1, int32_t xi2, int32_t yi0, int32_t yi1, int32_t yi2,
                              const float* U, const float* V, const float* D, float bx0, float bx1, float bx2,
                              float bx3, float m, uint32_t& lo, uint32_t& hi) {
  const float x0 = (float)xi0 * (1.0f / 256.0f), x1 = (float)xi1 * (1.0f / 256.0f), x2 = (float)xi2 * (1.0f / 256.0f);
  const float y0 = (float)yi0 * (1.0f / 256.0f), y1 = (float)yi1 * (1.0f / 256.0f), y2 = (float)yi2 * (1.0f / 256.0f);
  float xlo = -INFINITY, xhi = INFINITY, ylo = -INFINITY, yhi = INFINITY, mag = 0.0f;
  bool any = true;
  // (a loop, and the coefficients formed where they are used: unrolled, the four half-planes cost k_setup scratch)
#if defined(__HIPCC__)
#pragma nounroll
#endif
  for (int k = 0; k < 4; ++k) {
    const float sg = (k & 1) ? -1.0f : 1.0f, bd = k == 0 ? bx0 : k == 1 ? bx1 : k == 2 ? bx2 : bx3;
    const float h0 = sg * ((k < 2 ? U[0] : V[0]) - bd * D[0]), h1 = sg * ((k < 2 ? U[1] : V[1]) - bd * D[1]);
    const float h2 = sg * ((k < 2 ? U[2] : V[2]) - bd * D[2]);
    const float g0 = (h0 * x0 + h1 * y0) + h2, g1 = (h0 * x1 + h1 * y1) + h2, g2 = (h0 * x2 + h1 * y2) + h2;   // alpha_cut_plane
    mag += (fabsf(g0) + fabsf(g1)) + fabsf(g2);
    const bool in0 = g0 >= -kCutIn * m, in1 = g1 >= -kCutIn * m, in2 = g2 >= -kCutIn * m;
    any = any && (in0 || in1 || in2);
    // a vertex that is IN (any, if none is) stands in for every point that does not count
    const float rx = in0 ? x0 : in1 ? x1 : x2, ry = in0 ? y0 : in1 ? y1 : y2;
    float nx = rx, mx = rx, ny = ry, my = ry;   // this half-plane's extents
    auto point = [&](bool on, float x, float y) {
      x = on ? x : rx;
      y = on ? y : ry;
      nx = fminf(nx, x); mx = fmaxf(mx, x);
      ny = fminf(ny, y); my = fmaxf(my, y);
    };
    auto crossing = [&](float ga, float gb, bool ina, bool inb, float xa, float ya, float xb, float yb) {
      const float dc = ga - gb;
      float s = fminf(fmaxf((ga + kCutLevel * m) * cut_rcp(dc), 0.0f), 1.0f);
      s = fabsf(dc) >= kCutSmall * m ? s : (ina ? 1.0f : 0.0f);
      point(ina || inb, xa + s * (xb - xa), ya + s * (yb - ya));
    };
    point(in1, x1, y1);
    point(in2, x2, y2);
    crossing(g0, g1, in0, in1, x0, y0, x1, y1);
    crossing(g1, g2, in1, in2, x1, y1, x2, y2);
    crossing(g2, g0, in2, in0, x2, y2, x0, y0);
    xlo = fmaxf(xlo, nx); xhi = fminf(xhi, mx);
    ylo = fmaxf(ylo, ny); yhi = fminf(yhi, my);
  }
  if (!(mag < INFINITY)) return true;   // a NaN or an infinity somewhere: no cut
  if (!any) return false;
  const float wx = (fmaxf(fmaxf(fabsf(x0), fabsf(x1)), fabsf(x2)) + 1.0f) * kCutWiden;
  const float wy = (fmaxf(fmaxf(fabsf(y0), fabsf(y1)), fabsf(y2)) + 1.0f) * kCutWiden;
  // centres px + 0.5 in [lo - w, hi + w], clamped into the box (+-1) before the conversion
  int px0 = (int)(lo & 0xFFFFu), py0 = (int)(lo >> 16), px1 = (int)(hi & 0xFFFFu), py1 = (int)(hi >> 16);
  const float fx0 = (float)px0, fx1 = (float)px1, fy0 = (float)py0, fy1 = (float)py1;
  px0 = cut_imax(px0, (int)ceilf(fminf(fmaxf((xlo - wx) - 0.5f, fx0 - 1.0f), fx1 + 1.0f)));
  px1 = cut_imin(px1, (int)floorf(fminf(fmaxf((xhi + wx) - 0.5f, fx0 - 1.0f), fx1 + 1.0f)));
  py0 = cut_imax(py0, (int)ceilf(fminf(fmaxf((ylo - wy) - 0.5f, fy0 - 1.0f), fy1 + 1.0f)));
  py1 = cut_imin(py1, (int)floorf(fminf(fmaxf((yhi + wy) - 0.5f, fy0 - 1.0f), fy1 + 1.0f)));
  if (px0 > px1 || py0 > py1) return false;
  lo = (uint32_t)px0 | ((uint32_t)py0 << 16);
  hi = (uint32_t)px1 | ((uint32_t)py1 << 16);
  return true;
}

}  // namespace csg
