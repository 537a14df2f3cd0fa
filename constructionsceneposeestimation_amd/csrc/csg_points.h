// csg_points.h — host launchers of the object-point kernels (csg_points.hip),
// called by csg_passes.cpp for csg_sample_object_points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csg_crops.h"

namespace csg {

// A csg_point_job with the pass's scratch; all pointers are device memory.
struct PointArgs {
  uint32_t W, H;              // the job's frames
  uint32_t P;                 // pixels of a frame: W * H <= 2^26
  uint32_t L;                 // labels: ids 0 .. L-1 belong to a label
  uint32_t K, N;              // slots per frame, samples per slot
  uint32_t CH;                // chunks of kPointChunk row-major pixels per frame: ceil(P / kPointChunk)
  uint32_t seed;
  const int32_t* instance;    // [n][H][W]
  const CropSlot* info;       // [n][K], only `label` is read
  const float* depth;         // [n][H][W], iff pt_xyz
  const float* intrinsics;    // [n][4] fx fy cx cy, iff pt_xyz
  const uint8_t* rgb;         // [n][H][W][3], iff pt_rgb
  const uint16_t* obj_coords; // [n][H][W][3], iff pt_coords
  const uint32_t* frame_keys; // [n] or null (the key of frame f is f)
  uint32_t* pt_count;         // [n][K] or null
  uint32_t* pt_choose;        // [n][K][N] or null
  float* pt_xyz;              // [n][K][N][3] or null
  uint8_t* pt_rgb;            // [n][K][N][3] or null
  uint16_t* pt_coords;        // [n][K][N][3] or null
  uint32_t* cnt;              // [n][L][CH] scratch: pixels of a wanted label per chunk (k_pts_count), then
                              // their exclusive scan over the chunks (k_pts_scan); other labels' entries are
                              // neither written nor read
  uint32_t* total;            // [n][L] scratch: M of every wanted label (k_pts_scan)
};

constexpr uint32_t kPointChunk = 4096;       // pixels a wave walks: 16 steps of 64 lanes x 4 ids
constexpr uint32_t kPointMaxLabels = 256;    // the per-wave label tables in LDS are sized for it

// k_pts_count: pixels of every (frame, wanted label, chunk) into cnt.
void launch_pts_count(const PointArgs& a, uint32_t n, hipStream_t st);
// k_pts_scan: cnt -> its exclusive scan over chunks per (frame, wanted label); total, pt_count, and the
// fill of every slot without pixels.
void launch_pts_scan(const PointArgs& a, uint32_t n, hipStream_t st);
// k_pts_emit: every sample of every slot with pixels.
void launch_pts_emit(const PointArgs& a, uint32_t n, hipStream_t st);

}  // namespace csg
