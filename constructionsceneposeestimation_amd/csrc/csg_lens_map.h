// csg_lens_map.h — the map of csg_lens_map (include/csg_api.h): for every pixel of a camera
// with Brown-Conrady lens distortion the position in a pinhole source frame that it shows, in 1/256 source
// pixel.  Plain C++ on the host: no HIP, no allocation, nothing but the caller's buffer is written.  libcsg.so
// exports it (csg_passes.cpp) and tests/lens_host.cpp drives it alone under the sanitizers; tests/lens_ref.py
// restates it in NumPy, bit for bit.
//
// Every operation below is IEEE float64 and rounds once (-ffp-contract=off); an expression is evaluated in
// the order its parentheses give, and a sum or product without parentheses from left to right.
//
// forward(x, y) -> (xd, yd) and the Jacobian (a, b; b, d), which is symmetric:
//   xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2
//   N  = 1 + ((k1 * r2 + k2 * r4) + k3 * r6)          D  = 1 + ((k4 * r2 + k5 * r4) + k6 * r6)
//   Np = (k1 + (2 * k2) * r2) + (3 * k3) * r4          Dp = (k4 + (2 * k5) * r2) + (3 * k6) * r4
//   R  = N / D                                          Rp = (Np * D - N * Dp) / (D * D)        (dR / dr2)
//   xd = (x * R + (2 * p1) * xy) + p2 * (r2 + 2 * xx)
//   yd = (y * R + p1 * (r2 + 2 * yy)) + (2 * p2) * xy
//   a  = ((R + (2 * xx) * Rp) + (2 * p1) * y) + (6 * p2) * x
//   b  = ((2 * xy) * Rp + (2 * p1) * x) + (2 * p2) * y
//   d  = ((R + (2 * yy) * Rp) + (6 * p1) * y) + (2 * p2) * x
//
// Pixel (i, j) of the output camera: xd0 = ((i + 0.5) - cx) / fx, yd0 = ((j + 0.5) - cy) / fy.
// Newton, kLensNewton = 16 steps whatever the data, from (x, y) = (xd0, yd0):
//   (xd, yd, a, b, d) = forward(x, y);  ex = xd - xd0, ey = yd - yd0;  det = a * d - b * b
//   x = x - (d * ex - b * ey) / det;    y = y - (a * ey - b * ex) / det
// Then once more (xd, yd, a, b, d) = forward(x, y), and mx = (xd - xd0) * fx, my = (yd - yd0) * fy.
//
// Cause, the first rule that applies:
//   1 no preimage   one of x, y, xd, yd, a, b, d is not finite; or mx * mx + my * my > 2^-20 (the forward
//                   model of the result misses the pixel's centre by more than 2^-10 output pixels); or not
//                   both a * d - b * b > 0 and a + d > 0 (the result is not in the unfolded region around the
//                   axis, where the Jacobian is positive definite).
//   2 outside       sx = sfx * x + scx, sy = sfy * y + scy; tx = floor(sx * 256 + 0.5), ty likewise; outside if
//                   tx or ty is not in [-2^31 + 1, 2^31 - 1] (a value that is not finite included: nothing else is
//                   converted to an integer); else qx = (int32) tx, qy = (int32) ty, and outside if the source
//                   pixel (qx >> 8, qy >> 8) is not in [0, src_width) x [0, src_height).
//   0 valid
// map[j][i] = (qx, qy) for a valid pixel and (INT32_MIN, cause) for any other; counts = {valid, no preimage,
// outside}.
#pragma once
#include <cmath>
#include <stdint.h>

#include "../../include/csg_api.h"

namespace csg {

constexpr int kLensNewton = 16;
constexpr uint32_t kLensMaxDim = 8192;

struct LensFwd {
  double xd, yd, a, b, d;
};

inline LensFwd lens_forward(const csg_lens_model& m, double x, double y) {
  const double xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2;
  const double N = 1.0 + ((m.k1 * r2 + m.k2 * r4) + m.k3 * r6), D = 1.0 + ((m.k4 * r2 + m.k5 * r4) + m.k6 * r6);
  const double Np = (m.k1 + (2.0 * m.k2) * r2) + (3.0 * m.k3) * r4, Dp = (m.k4 + (2.0 * m.k5) * r2) + (3.0 * m.k6) * r4;
  const double R = N / D, Rp = (Np * D - N * Dp) / (D * D);
  LensFwd f;
  f.xd = (x * R + (2.0 * m.p1) * xy) + m.p2 * (r2 + 2.0 * xx);
  f.yd = (y * R + m.p1 * (r2 + 2.0 * yy)) + (2.0 * m.p2) * xy;
  f.a = ((R + (2.0 * xx) * Rp) + (2.0 * m.p1) * y) + (6.0 * m.p2) * x;
  f.b = ((2.0 * xy) * Rp + (2.0 * m.p1) * x) + (2.0 * m.p2) * y;
  f.d = ((R + (2.0 * yy) * Rp) + (6.0 * m.p1) * y) + (2.0 * m.p2) * x;
  return f;
}

// 1 if the model is one csg_lens_map takes: sizes in 1..8192, every number finite, focal lengths > 0.
inline int lens_model_ok(const csg_lens_model* m) {
  if (!m) return 0;
  if (m->width < 1 || m->width > kLensMaxDim || m->height < 1 || m->height > kLensMaxDim) return 0;
  if (m->src_width < 1 || m->src_width > kLensMaxDim || m->src_height < 1 || m->src_height > kLensMaxDim) return 0;
  const double v[] = {m->fx, m->fy, m->cx, m->cy, m->k1, m->k2, m->p1, m->p2, m->k3, m->k4, m->k5, m->k6,
                      m->sfx, m->sfy, m->scx, m->scy};
  for (double e : v)
    if (!std::isfinite(e)) return 0;
  return m->fx > 0.0 && m->fy > 0.0 && m->sfx > 0.0 && m->sfy > 0.0;
}

// One pixel's entry; returns its cause.
inline uint32_t lens_map_pixel(const csg_lens_model& m, uint32_t i, uint32_t j, int32_t* q) {
  const double xd0 = (((double)i + 0.5) - m.cx) / m.fx, yd0 = (((double)j + 0.5) - m.cy) / m.fy;
  double x = xd0, y = yd0;
  for (int it = 0; it < kLensNewton; ++it) {
    const LensFwd f = lens_forward(m, x, y);
    const double ex = f.xd - xd0, ey = f.yd - yd0, det = f.a * f.d - f.b * f.b;
    x = x - (f.d * ex - f.b * ey) / det;
    y = y - (f.a * ey - f.b * ex) / det;
  }
  const LensFwd f = lens_forward(m, x, y);
  const double mx = (f.xd - xd0) * m.fx, my = (f.yd - yd0) * m.fy;
  q[0] = INT32_MIN;
  q[1] = 1;
  if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(f.xd) && std::isfinite(f.yd) && std::isfinite(f.a) && std::isfinite(f.b) && std::isfinite(f.d)))
    return 1u;
  if (mx * mx + my * my > 0x1p-20) return 1u;
  if (!(f.a * f.d - f.b * f.b > 0.0 && f.a + f.d > 0.0)) return 1u;
  q[1] = 2;
  const double sx = m.sfx * x + m.scx, sy = m.sfy * y + m.scy;
  const double tx = std::floor(sx * 256.0 + 0.5), ty = std::floor(sy * 256.0 + 0.5);
  if (!(tx >= -2147483647.0 && tx <= 2147483647.0 && ty >= -2147483647.0 && ty <= 2147483647.0)) return 2u;
  const int32_t qx = (int32_t)tx, qy = (int32_t)ty;
  const int32_t px = qx >> 8, py = qy >> 8;
  if (px < 0 || px >= (int32_t)m.src_width || py < 0 || py >= (int32_t)m.src_height) return 2u;
  q[0] = qx;
  q[1] = qy;
  return 0u;
}

// csg_lens_map without its export: CSG_ERR_INVALID (nothing written) for a model lens_model_ok refuses or a
// NULL map.
inline int lens_map(const csg_lens_model* m, int32_t* map, uint32_t* counts) {
  if (!lens_model_ok(m) || !map) return CSG_ERR_INVALID;
  uint32_t n[3] = {0u, 0u, 0u};
  for (uint32_t j = 0; j < m->height; ++j)
    for (uint32_t i = 0; i < m->width; ++i) n[lens_map_pixel(*m, i, j, map + ((size_t)j * m->width + i) * 2u)]++;
  if (counts) {
    counts[0] = n[0];
    counts[1] = n[1];
    counts[2] = n[2];
  }
  return CSG_OK;
}

}  // namespace csg
