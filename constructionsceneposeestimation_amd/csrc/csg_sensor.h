// csg_sensor.h — host launcher of the stereo-depth kernels (csg_sensor.hip),
// called by csg_passes.cpp for csg_sensor_depth.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csg {

constexpr uint32_t kSnCauses = 7;       // sensor_count[f][0..6]
constexpr uint32_t kSnCountStride = 8;  // words of scratch per frame's counters

// A csg_sensor_job with the pass's scratch, for one range of frames; all pointers are device memory.
struct SensorArgs {
  uint32_t W, H;
  uint32_t first, n;          // the range: frames first .. first + n - 1 of the job
  uint32_t r;                 // window radius 0..4
  uint32_t min_support, tol;
  uint32_t sh;                // 8 - subpixel_bits
  uint32_t noise_k, seed;
  uint32_t clip_band;         // CSG_SENSOR_CLIP_BAND
  float abs_b;                // |baseline|
  uint32_t right;             // baseline > 0: the second camera is to the right, the scan comes from the right end
  float z_min, z_max;
  const float* depth;         // [..][H][W]
  const float* intrinsics;    // [..][4]
  const uint32_t* frame_keys; // or null
  float* sensor_depth;        // outputs of the whole job, any may be null
  uint8_t* sensor_cause;
  uint32_t* sensor_count;
  int32_t* state;             // [n][H][W] scratch: dq of a lit pixel, -cause (1..4) of any other
  uint32_t* counts;           // [n][kSnCountStride] scratch
};

// Enqueues the range's kernels: k_sn_rows, k_sn_match and, with sensor_count, k_sn_counts.
void launch_sensor(const SensorArgs& a, hipStream_t st);

}  // namespace csg
