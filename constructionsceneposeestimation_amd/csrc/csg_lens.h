// csg_lens.h — host launchers of the lens-distortion kernels (csg_lens.hip), called by csg_passes.cpp for
// csg_lens_remap and csg_lens_points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csg {

constexpr uint32_t kLnCauses = 3;   // lens_count[f][0..2]

// A csg_lens_job for csg_lens_remap; all pointers are device memory.
struct LensArgs {
  uint32_t W, H, SW, SH;
  uint32_t n;                 // frames
  uint32_t n_labels;
  uint32_t nearest;           // rgb_filter == CSG_LENS_FILTER_NEAREST
  const int32_t* map;         // [H][W][2]
  const uint8_t* rgb;         // sources [n][SH][SW]..., any may be null
  const int32_t* instance;
  const float* depth;
  const uint16_t* obj_coords;
  uint8_t* lens_rgb;          // outputs [n][H][W]..., any may be null
  int32_t* lens_instance;
  float* lens_depth;
  uint16_t* lens_coords;
  uint8_t* lens_valid;
  uint32_t* lens_stats;       // [n][n_labels][5]
  uint32_t* lens_count;       // [n][3]
};

// Enqueues k_ln_init (with lens_stats or lens_count) and k_ln_remap.
void launch_lens(const LensArgs& a, hipStream_t st);

// The model of csg_lens_points in float32, and its arrays (device memory).
struct LensPointArgs {
  float W, H;
  float fx, fy, cx, cy, sfx, sfy, scx, scy;
  float k1, k2, p1, p2, k3, k4, k5, k6;
  uint32_t total;             // n * K keypoints
  const float* uv;
  const int32_t* vis;
  float* lens_uv;
  int32_t* lens_vis;
};

void launch_lens_points(const LensPointArgs& a, hipStream_t st);

}  // namespace csg
