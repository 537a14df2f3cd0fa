// csg_alpha_box.h -- the camera-invariant "opaque box" of an alpha-tested
// triangle ("alpha trim"): the axis-aligned uv box outside
// which every alpha quad the triangle can reach fails the alpha test whatever
// the bilinear weights, so k_setup may shrink the record's pixel box to it.
// Host only, plain C++ (no HIP): csg_api.cpp builds the boxes at upload,
// tests/alpha_box_host.cpp checks them against a brute-force scan.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace csg {

// The constants of the proof (texels).  A fragment's computed texel coordinates
// lie within kAlphaScanGuard of the triangle's true uv triangle: k_setup trims
// only when the stored planes reproduce the vertices' uvs within 1 texel and the
// evaluation error stays below 1/4 texel (alpha_trim_guard), and the scan's own
// double arithmetic is exact to ~1e-9.  The box is widened by kAlphaBoxMargin
// beyond the quads' exact bounds, which pays for the evaluation error of the
// fragment (<= 1/4) with 1/4 to spare.
constexpr double kAlphaScanGuard = 2.0;
constexpr double kAlphaBoxMargin = 0.5;
constexpr double kAlphaMaxTexel = 4194304.0;   // 2^22: alpha_pass zeroes coordinates from 2^23 on

// Per texture and threshold: for every texel x of row y the nearest alpha quad
// at or after / at or before x (in the row, no wrap) that can pass the test,
// i.e. whose four alphas (x,y), (x+1,y), (x,y+1), (x+1,y+1), wrapped, are not
// all <= thr (class 0 of build_alpha_classes).  next = w, prev = -1: none.
struct AlphaScan {
  uint32_t w = 0, h = 0;
  std::vector<int32_t> next, prev;
};

inline void alpha_scan_build(const uint8_t* rgba, uint32_t w, uint32_t h, uint32_t thr, AlphaScan& s) {
  s.w = w;
  s.h = h;
  s.next.assign((size_t)w * h, (int32_t)w);
  s.prev.assign((size_t)w * h, -1);
  auto a = [&](uint32_t x, uint32_t y) { return (uint32_t)rgba[((size_t)y * w + x) * 4 + 3]; };
  for (uint32_t y = 0; y < h; ++y) {
    const uint32_t y1 = y + 1 == h ? 0 : y + 1;
    int32_t* nx = &s.next[(size_t)y * w];
    int32_t* pv = &s.prev[(size_t)y * w];
    int32_t last = -1;
    for (uint32_t x = 0; x < w; ++x) {
      const uint32_t x1 = x + 1 == w ? 0 : x + 1;
      const uint32_t mx = std::max(std::max(a(x, y), a(x1, y)), std::max(a(x, y1), a(x1, y1)));
      if (mx > thr) last = (int32_t)x;
      pv[x] = last;
    }
    int32_t nxt = (int32_t)w;
    for (uint32_t x = w; x-- > 0;) {
      if (pv[x] == (int32_t)x) nxt = (int32_t)x;
      nx[x] = nxt;
    }
  }
}

// Box values: {u_lo, u_hi, v_lo, v_hi}.  A fragment whose u or v (as the raster
// evaluates them, error included) lies outside can be dropped.
inline void alpha_box_full(float* box) {
  box[0] = box[2] = -INFINITY;
  box[1] = box[3] = INFINITY;
}
inline void alpha_box_empty(float* box) {   // no quad can pass: the triangle emits no record
  box[0] = box[2] = INFINITY;
  box[1] = box[3] = -INFINITY;
}

inline float alpha_round_down(double x) {
  float f = (float)x;
  return (double)f > x ? std::nextafterf(f, -INFINITY) : f;
}
inline float alpha_round_up(double x) {
  float f = (float)x;
  return (double)f < x ? std::nextafterf(f, INFINITY) : f;
}

// The box of one triangle with uvs uv = u0 v0 u1 v1 u2 v2.  Texel space as
// alpha_pass: t = (u * w - 0.5, (1 - v) * h - 0.5), quad index = floor(t),
// wrapped.  Every quad row j that the uv triangle dilated by the guard band
// touches is scanned over the columns the dilated triangle reaches in it.
inline void alpha_tri_box(const AlphaScan& s, const float* uv, float* box) {
  alpha_box_full(box);
  const double G = kAlphaScanGuard;
  const int64_t tw = s.w, th = s.h;
  if (tw == 0 || th == 0) return;
  double tx[3], ty[3];
  for (int k = 0; k < 3; ++k) {
    tx[k] = (double)uv[2 * k] * (double)tw - 0.5;
    ty[k] = (1.0 - (double)uv[2 * k + 1]) * (double)th - 0.5;
    if (!(std::fabs(tx[k]) < kAlphaMaxTexel) || !(std::fabs(ty[k]) < kAlphaMaxTexel)) return;   // also NaN
  }
  const double xmin = std::min(tx[0], std::min(tx[1], tx[2])), xmax = std::max(tx[0], std::max(tx[1], tx[2]));
  const double ymin = std::min(ty[0], std::min(ty[1], ty[2])), ymax = std::max(ty[0], std::max(ty[1], ty[2]));
  const int64_t bx0 = (int64_t)std::floor(xmin - G), bx1 = (int64_t)std::floor(xmax + G);
  const int64_t j0 = (int64_t)std::floor(ymin - G), j1 = (int64_t)std::floor(ymax + G);
  // a whole repeat in either axis: the unwrapped box means nothing
  if (bx1 - bx0 + 1 > tw || j1 - j0 + 1 > th) return;
  bool any = false;
  int64_t qx0 = 0, qx1 = 0, qy0 = 0, qy1 = 0;
  for (int64_t j = j0; j <= j1; ++j) {
    // x extent of the triangle inside the slab ty in [j - G, j + 1 + G]
    const double lo = (double)j - G, hi = (double)j + 1.0 + G;
    double ex0 = INFINITY, ex1 = -INFINITY;
    for (int k = 0; k < 3; ++k) {
      const int n = k == 2 ? 0 : k + 1;
      if (ty[k] >= lo && ty[k] <= hi) { ex0 = std::min(ex0, tx[k]); ex1 = std::max(ex1, tx[k]); }
      for (const double yb : {lo, hi}) {
        if ((ty[k] < yb && ty[n] > yb) || (ty[k] > yb && ty[n] < yb)) {
          const double x = tx[k] + (tx[n] - tx[k]) * ((yb - ty[k]) / (ty[n] - ty[k]));
          ex0 = std::min(ex0, x);
          ex1 = std::max(ex1, x);
        }
      }
    }
    if (!(ex0 <= ex1)) continue;
    const int64_t a = std::max(bx0, (int64_t)std::floor(ex0 - G)), b = std::min(bx1, (int64_t)std::floor(ex1 + G));
    if (a > b) continue;
    const int64_t jr = ((j % th) + th) % th, ar = ((a % tw) + tw) % tw;
    const int32_t* nx = &s.next[(size_t)jr * tw];
    const int32_t* pv = &s.prev[(size_t)jr * tw];
    // [a, b] is at most one repeat long: one or two pieces of the wrapped row
    const int64_t len = b - a, e1 = std::min<int64_t>(ar + len, tw - 1);
    int64_t first = INT64_MAX, last = INT64_MIN;
    if (nx[ar] <= e1) { first = a + (nx[ar] - ar); last = a + (pv[e1] - ar); }
    if (ar + len >= tw) {
      const int64_t e2 = ar + len - tw, off = a + (tw - ar);   // wrapped columns 0..e2 are unwrapped off..off + e2
      if (nx[0] <= e2) { first = std::min(first, off + nx[0]); last = std::max(last, off + pv[e2]); }
    }
    if (first > last) continue;
    if (!any) { qx0 = first; qx1 = last; qy0 = qy1 = j; any = true; }
    qx0 = std::min(qx0, first);
    qx1 = std::max(qx1, last);
    qy1 = j;
  }
  if (!any) { alpha_box_empty(box); return; }
  // survivors have floor(t) in [q0, q1], i.e. t in [q0, q1 + 1); widened by the margin and mapped back to uv
  const double M = kAlphaBoxMargin;
  box[0] = alpha_round_down(((double)qx0 + 0.5 - M) / (double)tw);
  box[1] = alpha_round_up(((double)qx1 + 1.5 + M) / (double)tw);
  box[2] = alpha_round_down(1.0 - ((double)qy1 + 1.5 + M) / (double)th);
  box[3] = alpha_round_up(1.0 - ((double)qy0 + 0.5 - M) / (double)th);
}

}  // namespace csg
