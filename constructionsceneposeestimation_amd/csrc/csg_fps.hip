// csg_fps.hip — farthest-point sampling of point sets for csg_farthest_points: K samples of each set, every
// one the candidate farthest from those chosen before it, without leaving the GPU.  The definition is the
// spec of include/csg_api.h, restated in NumPy by tests/farthest_points_ref.py.
//
//   k_fp_select<T, PPT>  a workgroup of T threads per set.  Thread tid owns the candidates j = i * T + tid,
//                        i < PPT, and keeps their coordinates and their distance to the chosen set (mind)
//                        in registers for the whole run; PPT is a template argument and every register
//                        array is indexed by unrolled constants only (nothing goes to scratch memory).
//
// A step.  Every thread lowers the mind of its candidates by the distance to the point chosen last and
// keeps the largest (with its index and coordinates; a strict > keeps the lowest index, its candidates
// ascend).  The arg-max over the set is a maximum over one 64-bit key per thread: mind's bits above ~j.
// mind is never negative and never NaN, so its bits order as unsigned; the lowest j wins ties by
// construction.  The wave reduces the key by six xor shuffles; the lane that holds the wave's key writes it
// with its point into one of two sets of T / 64 LDS entries, and after the step's one barrier every thread
// reads them all and takes the largest: the next chosen point, known to every thread, no load from memory.
// The two sets alternate, so a wave that runs ahead into the next step writes the other set.  A workgroup
// of one wave needs neither LDS nor barrier: the winner's point comes by a lane read.
//
// Invalid candidates (a coordinate not finite) and the lanes past c_s hold the point 0 and mind 0: their
// distance to anything is >= +0 or +inf, never NaN, so min() keeps their 0 and they are never chosen (a
// step whose maximum is 0 ends the run).
//
// Thread 0 stores fp_xyz and fp_dist2 of a step as it is chosen and stages the chosen candidate as a uint16
// in LDS (K * 2 bytes).  The tail of the kernel writes fp_index and the wrap region t >= t0 from that
// stage, coalesced, and gathers the payload rows (fp_gather): the indices never have to exist in memory,
// so the pass needs no scratch and no second launch.
#include "csg_fps.h"

#pragma clang fp contract(off)

namespace csg {

namespace {

constexpr uint32_t kFpNan = 0x7FC00000u;

__device__ __forceinline__ uint32_t fp_fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// How a set's candidates map to its rows: r_j = (j * m) / c = j * q + (j * rem) / c with q = m / c and
// rem = m % c; j and rem are below 2^14, so 32 bits hold every term.
struct FpRows {
  uint32_t q, rem, c;
  __device__ __forceinline__ uint32_t row(uint32_t j) const { return j * q + (j * rem) / c; }
};

__device__ __forceinline__ uint64_t fp_wave_max(uint64_t key) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(key >> 32), o), lo = __shfl_xor((uint32_t)key, o);
    const uint64_t other = ((uint64_t)hi << 32) | lo;
    key = other > key ? other : key;
  }
  return key;
}

struct FpEntry {   // a wave's largest key and its point
  uint64_t key;
  float x, y, z;
  uint32_t pad;
};

// The rows dst[t] = src[row of sample t] of one payload, t < K: words when the addresses allow, else bytes;
// consecutive threads write consecutive words or bytes.
__device__ __forceinline__ void fp_gather(const FpPayload& pl, size_t s, uint32_t C, uint32_t K, uint32_t t0,
                                          const uint16_t* sel, const FpRows& rows, uint32_t tid, uint32_t T) {
  const uint32_t rb = pl.row_bytes;
  const uint8_t* src = pl.src + s * C * rb;
  uint8_t* dst = pl.dst + s * K * rb;
  if (((rb | (uint32_t)(uintptr_t)pl.src | (uint32_t)(uintptr_t)pl.dst) & 3u) == 0u) {
    const uint32_t rw = rb >> 2, total = K * rw;
    for (uint32_t b = tid; b < total; b += T) {
      const uint32_t t = b / rw, o = b - t * rw;
      const uint32_t r = rows.row(sel[t < t0 ? t : t % t0]);
      reinterpret_cast<uint32_t*>(dst)[b] = reinterpret_cast<const uint32_t*>(src + (size_t)r * rb)[o];
    }
  } else {
    const uint32_t total = K * rb;
    for (uint32_t b = tid; b < total; b += T) {
      const uint32_t t = b / rb, o = b - t * rb;
      const uint32_t r = rows.row(sel[t < t0 ? t : t % t0]);
      dst[b] = src[(size_t)r * rb + o];
    }
  }
}

__device__ __forceinline__ void fp_fill(const FpPayload& pl, size_t s, uint32_t K, uint32_t tid, uint32_t T) {
  uint8_t* dst = pl.dst + s * K * pl.row_bytes;
  const uint32_t total = K * pl.row_bytes;
  for (uint32_t b = tid; b < total; b += T) dst[b] = (uint8_t)pl.fill;
}

// grid (n): workgroup b is set a.first + b.  Dynamic LDS: K uint16.
template <uint32_t T, uint32_t PPT>
__global__ __launch_bounds__(T) void k_fp_select(FpsArgs a) {
  constexpr uint32_t NW = T / 64u;
  extern __shared__ uint16_t fp_sel[];          // [K] the chosen candidates
  __shared__ FpEntry red[2][NW];
  __shared__ uint32_t n_ok[NW];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const size_t s = (size_t)a.first + blockIdx.x;
  const uint32_t K = a.K;

  uint32_t m = a.C;
  if (a.counts) {
    const uint32_t n = a.counts[s];
    m = n == 0xFFFFFFFFu ? 0u : (n < a.C ? n : a.C);
  }
  const uint32_t c = m < a.P ? m : a.P;
  FpRows rows;
  rows.c = c ? c : 1u;
  rows.q = m / rows.c;
  rows.rem = m % rows.c;
  const float* __restrict__ xs = a.xyz + s * a.C * 3u;

  const uint32_t key_s = a.set_keys ? a.set_keys[s] : (uint32_t)s;
  const uint32_t h = fp_fmix32(fp_fmix32(a.seed ^ key_s) ^ 0x9E3779B9u);
  const uint32_t j0 = (uint32_t)(((uint64_t)h * c) >> 32);

  // the candidates, into registers; the start is the maximum of ~cyc above ~j over the valid ones
  float px[PPT], py[PPT], pz[PPT], md[PPT];
  uint32_t ok_n = 0;
  uint64_t skey = 0;
#pragma unroll
  for (uint32_t i = 0; i < PPT; ++i) {
    const uint32_t j = i * T + tid;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    bool ok = false;
    if (j < c) {
      const float* p = xs + (size_t)rows.row(j) * 3u;
      x = p[0];
      y = p[1];
      z = p[2];
      ok = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
    }
    px[i] = ok ? x : 0.0f;
    py[i] = ok ? y : 0.0f;
    pz[i] = ok ? z : 0.0f;
    md[i] = ok ? __builtin_inff() : 0.0f;
    if (ok) {
      ++ok_n;
      const uint32_t cyc = j >= j0 ? j - j0 : j + c - j0;
      const uint64_t k = ((uint64_t)~cyc << 32) | (uint32_t)~j;
      skey = k > skey ? k : skey;
    }
  }
  skey = fp_wave_max(skey);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ok_n += __shfl_xor(ok_n, o);
  if (NW > 1) {
    if (lane == 0) {
      red[0][wave].key = skey;
      n_ok[wave] = ok_n;
    }
    __syncthreads();
    skey = 0;
    ok_n = 0;
#pragma unroll
    for (uint32_t w = 0; w < NW; ++w) {
      const uint64_t k = red[0][w].key;
      skey = k > skey ? k : skey;
      ok_n += n_ok[w];
    }   // red[0] is written again in step 2: behind step 1's barrier, which no wave passes before this
  }
  const size_t o_s = s * K;

  if (ok_n == 0) {   // the empty set (the whole workgroup)
    if (tid == 0 && a.fp_count) {
      a.fp_count[2u * s] = 0u;
      a.fp_count[2u * s + 1u] = 0u;
    }
    for (uint32_t t = tid; t < K; t += T) {
      if (a.fp_index) a.fp_index[o_s + t] = 0xFFFFFFFFu;
      if (a.fp_dist2) a.fp_dist2[o_s + t] = 0.0f;
    }
    if (a.fp_xyz)
      for (uint32_t t = tid; t < 3u * K; t += T) reinterpret_cast<uint32_t*>(a.fp_xyz)[o_s * 3u + t] = kFpNan;
#pragma unroll
    for (uint32_t p = 0; p < kFpMaxPayloads; ++p)
      if (p < a.n_payloads) fp_fill(a.payload[p], s, K, tid, T);
    return;
  }

  uint32_t aj = ~(uint32_t)skey;   // the start
  float ax, ay, az, ag = __builtin_inff();
  {
    const float* p = xs + (size_t)rows.row(aj) * 3u;
    ax = p[0];
    ay = p[1];
    az = p[2];
  }
  uint32_t t = 0, buf = 1;
  for (; t < K; ++t) {
    if (t > 0) {
      float bm = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
      uint32_t bi = 0;
#pragma unroll
      for (uint32_t i = 0; i < PPT; ++i) {
        if (i > 0 && i * T >= c) break;   // (the whole workgroup) no thread has a candidate i of a small set
        const float dx = px[i] - ax, dy = py[i] - ay, dz = pz[i] - az;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const float v = d2 < md[i] ? d2 : md[i];
        md[i] = v;
        if (i == 0 || v > bm) {
          bm = v;
          bi = i;
          bx = px[i];
          by = py[i];
          bz = pz[i];
        }
      }
      const uint64_t own = ((uint64_t)__float_as_uint(bm) << 32) | (uint32_t)~(bi * T + tid);
      uint64_t best = fp_wave_max(own);
      if (NW == 1) {
        const int wl = (int)(~(uint32_t)best & 63u);   // j = i * 64 + lane
        ax = __shfl(bx, wl);
        ay = __shfl(by, wl);
        az = __shfl(bz, wl);
      } else {
        if (own == best) {
          FpEntry e;
          e.key = own;
          e.x = bx;
          e.y = by;
          e.z = bz;
          e.pad = 0;
          red[buf][wave] = e;
        }
        __syncthreads();
        best = red[buf][lane & (NW - 1u)].key;   // NW entries, repeating along the wave
#pragma unroll
        for (int o = NW / 2; o > 0; o >>= 1) {
          const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), o), lo = __shfl_xor((uint32_t)best, o);
          const uint64_t other = ((uint64_t)hi << 32) | lo;
          best = other > best ? other : best;
        }
        const uint32_t bw = (~(uint32_t)best & (T - 1u)) >> 6;   // the wave of thread j mod T
        ax = red[buf][bw].x;
        ay = red[buf][bw].y;
        az = red[buf][bw].z;
        buf ^= 1u;
      }
      ag = __uint_as_float((uint32_t)(best >> 32));
      aj = ~(uint32_t)best;
      if (ag == 0.0f) break;   // every valid candidate coincides with a chosen one (the whole workgroup)
    }
    if (tid == 0) {
      fp_sel[t] = (uint16_t)aj;
      if (a.fp_xyz) {
        float* o = a.fp_xyz + (o_s + t) * 3u;
        o[0] = ax;
        o[1] = ay;
        o[2] = az;
      }
      if (a.fp_dist2) a.fp_dist2[o_s + t] = ag;
    }
  }
  const uint32_t t0 = t;
  __syncthreads();   // fp_sel

  if (tid == 0 && a.fp_count) {
    a.fp_count[2u * s] = t0;
    a.fp_count[2u * s + 1u] = ok_n;
  }
  for (uint32_t u = tid; u < K; u += T) {
    const uint32_t r = rows.row(fp_sel[u < t0 ? u : u % t0]);
    if (a.fp_index) a.fp_index[o_s + u] = r;
    if (u >= t0) {   // the wrap: entry u mod t0 again
      if (a.fp_xyz) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(xs) + (size_t)r * 3u;
        uint32_t* o = reinterpret_cast<uint32_t*>(a.fp_xyz) + (o_s + u) * 3u;
        o[0] = p[0];
        o[1] = p[1];
        o[2] = p[2];
      }
      if (a.fp_dist2) a.fp_dist2[o_s + u] = 0.0f;
    }
  }
#pragma unroll
  for (uint32_t p = 0; p < kFpMaxPayloads; ++p)
    if (p < a.n_payloads) fp_gather(a.payload[p], s, a.C, K, t0, fp_sel, rows, tid, T);
}

template <uint32_t T, uint32_t PPT>
void launch_instance(const FpsArgs& a, uint32_t n, hipStream_t st) {
  const uint32_t lds = ((a.K * 2u) + 15u) & ~15u;
  hipLaunchKernelGGL((k_fp_select<T, PPT>), dim3(n), dim3(T), lds, st, a);
}

}  // namespace

FpsShape fps_shape(uint32_t rows, uint32_t pool) {
  const uint32_t c = rows < pool ? rows : pool;
  if (c <= 64u) return {64u, 1u};
  if (c <= 128u) return {64u, 2u};
  if (c <= 256u) return {256u, 1u};
  if (c <= 512u) return {256u, 2u};
  if (c <= 1024u) return {256u, 4u};
  if (c <= 2048u) return {1024u, 2u};
  if (c <= 4096u) return {1024u, 4u};
  if (c <= 8192u) return {1024u, 8u};
  return {1024u, 16u};
}

void launch_fps(const FpsArgs& a, uint32_t n, hipStream_t st) {
  const FpsShape sh = fps_shape(a.C, a.P);
  switch (sh.threads * 32u + sh.ppt) {
    case 64u * 32u + 1u: launch_instance<64, 1>(a, n, st); break;
    case 64u * 32u + 2u: launch_instance<64, 2>(a, n, st); break;
    case 256u * 32u + 1u: launch_instance<256, 1>(a, n, st); break;
    case 256u * 32u + 2u: launch_instance<256, 2>(a, n, st); break;
    case 256u * 32u + 4u: launch_instance<256, 4>(a, n, st); break;
    case 1024u * 32u + 2u: launch_instance<1024, 2>(a, n, st); break;
    case 1024u * 32u + 4u: launch_instance<1024, 4>(a, n, st); break;
    case 1024u * 32u + 8u: launch_instance<1024, 8>(a, n, st); break;
    default: launch_instance<1024, 16>(a, n, st); break;
  }
}

}  // namespace csg
