// csg_fps.h — host launcher of the farthest-point kernels (csg_fps.hip),
// called by csg_passes.cpp for csg_farthest_points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csg {

constexpr uint32_t kFpMaxPool = 16384;     // candidates of a set: one workgroup holds them in registers
constexpr uint32_t kFpMaxSamples = 16384;  // samples of a set: their candidates are staged as uint16 in LDS
constexpr uint32_t kFpMaxPayloads = 4;
constexpr uint32_t kFpMaxRowBytes = 64;

struct FpPayload {
  const uint8_t* src;   // [S][C][row_bytes]
  uint8_t* dst;         // [S][K][row_bytes]
  uint32_t row_bytes;   // 1..64
  uint32_t fill;        // the byte of an empty set's rows
};

// A csg_fps_job for one range of sets; all pointers are device memory.
struct FpsArgs {
  uint32_t first;             // the range's first set: workgroup b works on set first + b
  uint32_t C, P, K;           // rows, pool, samples
  uint32_t seed;
  uint32_t n_payloads;
  const float* xyz;           // [S][C][3]
  const uint32_t* counts;     // [S], or null
  const uint32_t* set_keys;   // [S], or null
  uint32_t* fp_index;         // outputs of the whole job, any may be null
  float* fp_xyz;
  float* fp_dist2;
  uint32_t* fp_count;
  FpPayload payload[kFpMaxPayloads];
};

// The kernel instance a call runs: T threads a workgroup, each owning `ppt` candidates, the smallest of
// the instances with T * ppt >= min(C, P).
struct FpsShape {
  uint32_t threads, ppt;
};
FpsShape fps_shape(uint32_t rows, uint32_t pool);

// Enqueues k_fp_select for `n` sets (n <= 2^30): one workgroup a set.
void launch_fps(const FpsArgs& a, uint32_t n, hipStream_t st);

}  // namespace csg
