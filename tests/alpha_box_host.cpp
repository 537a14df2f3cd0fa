// Stand-alone driver of csg_alpha_box.h for tests/test_alpha_box_host.py: reads
//   w h thr n, then w*h alpha bytes (as integers), then n x 6 uv floats (hex float bit patterns)
// from stdin and prints one line "u_lo u_hi v_lo v_hi" (float bit patterns, hex) per triangle.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../constructionsceneposeestimation_amd/csrc/csg_alpha_box.h"

int main() {
  unsigned w, h, thr, n;
  if (scanf("%u %u %u %u", &w, &h, &thr, &n) != 4) return 2;
  std::vector<uint8_t> rgba((size_t)w * h * 4, 7);
  for (size_t k = 0; k < (size_t)w * h; ++k) {
    unsigned a;
    if (scanf("%u", &a) != 1) return 2;
    rgba[k * 4 + 3] = (uint8_t)a;
  }
  csg::AlphaScan s;
  csg::alpha_scan_build(rgba.data(), w, h, thr, s);
  for (unsigned t = 0; t < n; ++t) {
    float uv[6], box[4];
    for (int k = 0; k < 6; ++k) {
      uint32_t bits;
      if (scanf("%" SCNx32, &bits) != 1) return 2;
      memcpy(&uv[k], &bits, 4);
    }
    csg::alpha_tri_box(s, uv, box);
    uint32_t o[4];
    memcpy(o, box, 16);
    printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", o[0], o[1], o[2], o[3]);
  }
  return 0;
}
