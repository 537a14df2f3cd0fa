// Stand-alone driver of csgio_spans_to_rle (csrc/csg_io.cpp) for a sanitizer
// build (tests/test_mask_rle.py): pseudo-random and corner-case id images are
// turned into spans, the spans into counts and strings in heap buffers of
// exactly the size asked for (an overrun is a sanitizer report), and the
// strings are decoded again and compared with the image.
#include "../include/csg_io.h"

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static int fail(const char* what, int a = 0, int b = 0) {
  std::printf("rle_host: %s (%d, %d)\n", what, a, b);
  return 1;
}

static std::vector<uint32_t> from_string(const std::string& s) {
  std::vector<uint32_t> c;
  size_t p = 0;
  while (p < s.size()) {
    int64_t x = 0;
    int k = 0;
    bool more = true;
    while (more && p < s.size()) {
      const int64_t b = s[p] - 48;
      x |= (b & 0x1f) << (5 * k);
      more = (b & 0x20) != 0;
      ++p;
      ++k;
      if (!more && (b & 0x10)) x |= -(int64_t(1) << (5 * k));
    }
    if (c.size() > 2) x += c[c.size() - 2];
    c.push_back((uint32_t)x);
  }
  return c;
}

static int check_image(const std::vector<int32_t>& ids, uint32_t H, uint32_t W, uint32_t L) {
  std::vector<std::vector<uint32_t>> per(L);
  for (uint32_t x = 0; x < W; ++x)
    for (uint32_t y = 0; y < H;) {
      const int32_t l = ids[(size_t)y * W + x];
      if (l < 0 || (uint32_t)l >= L) {
        ++y;
        continue;
      }
      const uint32_t y0 = y;
      while (y < H && ids[(size_t)y * W + x] == l) ++y;
      per[l].push_back(x * H + y0);
      per[l].push_back(y - y0);
    }
  std::vector<uint32_t> off(L + 1, 0), spans;
  for (uint32_t l = 0; l < L; ++l) {
    spans.insert(spans.end(), per[l].begin(), per[l].end());
    off[l + 1] = (uint32_t)(spans.size() / 2);
  }
  std::vector<uint64_t> c_off(L + 1), s_off(L + 1);
  // sizes first (no buffers), then buffers of exactly those sizes
  int rc = csgio_spans_to_rle(spans.data(), off.data(), L, H, W, nullptr, 0, c_off.data(), nullptr, 0, s_off.data());
  if (rc) return fail("sizing call", rc);
  const uint64_t nc = c_off[L], ns = s_off[L];
  uint32_t* counts = (uint32_t*)std::malloc(nc ? nc * 4 : 1);
  char* str = (char*)std::malloc(ns ? ns : 1);
  rc = csgio_spans_to_rle(spans.data(), off.data(), L, H, W, counts, nc, c_off.data(), str, ns, s_off.data());
  int bad = rc ? fail("exact capacities", rc) : 0;
  if (!bad && nc > 0 &&
      csgio_spans_to_rle(spans.data(), off.data(), L, H, W, counts, nc - 1, c_off.data(), str, ns, s_off.data()) != -ENOSPC)
    bad = fail("one count short");
  if (!bad && ns > 0 &&
      csgio_spans_to_rle(spans.data(), off.data(), L, H, W, counts, nc, c_off.data(), str, ns - 1, s_off.data()) != -ENOSPC)
    bad = fail("one character short");
  for (uint32_t l = 0; l < L && !bad; ++l) {
    const std::vector<uint32_t> c(counts + c_off[l], counts + c_off[l + 1]);
    if (per[l].empty()) {
      if (!c.empty() || s_off[l] != s_off[l + 1]) bad = fail("a label without spans has output", (int)l);
      continue;
    }
    if (from_string(std::string(str + s_off[l], str + s_off[l + 1])) != c) bad = fail("string != counts", (int)l);
    uint64_t pos = 0;
    for (size_t i = 0; i < c.size() && !bad; ++i)
      for (uint32_t k = 0; k < c[i] && !bad; ++k, ++pos) {
        if (pos >= (uint64_t)H * W) bad = fail("counts run past the image", (int)l);
        else if ((ids[(size_t)(pos % H) * W + pos / H] == (int32_t)l) != (i % 2 == 1)) bad = fail("mask differs", (int)l, (int)pos);
      }
    if (!bad && pos != (uint64_t)H * W) bad = fail("counts do not cover the image", (int)l);
  }
  std::free(counts);
  std::free(str);
  return bad;
}

int main() {
  uint32_t rng = 12345u;
  auto next = [&]() { return rng = rng * 1664525u + 1013904223u; };
  const uint32_t shapes[][2] = {{1, 1}, {5, 3}, {16, 64}, {37, 70}, {17, 129}};
  for (auto& s : shapes) {
    const uint32_t H = s[0], W = s[1];
    for (uint32_t L : {1u, 3u, 256u})
      for (int pat = 0; pat < 6; ++pat) {
        std::vector<int32_t> ids((size_t)H * W);
        for (uint32_t y = 0; y < H; ++y)
          for (uint32_t x = 0; x < W; ++x) {
            int32_t v = -1;
            if (pat == 1) v = (int32_t)L - 1;                       // a full frame of one label
            if (pat == 2) v = (y & 1) ? -1 : 0;                     // the most spans
            if (pat == 3) v = (int32_t)((next() >> 16) % (L + 2)) - 1;
            if (pat == 4) v = ((x + y) & 1) ? (int32_t)L + 5 : INT32_MIN;
            if (pat == 5) v = (y == H - 1 || y == 0) ? 0 : -1;      // runs that merge across columns
            ids[(size_t)y * W + x] = v;
          }
        if (check_image(ids, H, W, L)) return 1;
      }
  }
  // spans an overflowed frame may hold: every kind is refused, none is followed out of bounds
  const uint32_t bad[][4] = {{4, 4, 2, 2}, {0, 0, 1, 1}, {2, 4, 5, 1}, {14, 3, 0, 0}};
  for (auto& b : bad) {
    const uint32_t off[2] = {0, b[3] || b[2] ? 2u : 1u};
    uint64_t c_off[2], s_off[2];
    if (csgio_spans_to_rle(b, off, 1, 4, 4, nullptr, 0, c_off, nullptr, 0, s_off) != -EINVAL) return fail("bad spans");
  }
  std::printf("rle_host ok\n");
  return 0;
}
