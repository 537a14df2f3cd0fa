// csg_crops.h — host launchers of the object-crop kernels (csg_crops.hip),
// called by csg_passes.cpp for csg_crop_objects and csg_crop_objects_filtered.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csg {

// One crop slot: the layout of csg_crop_info (include/csg_api.h), 32 bytes.
struct CropSlot {
  int32_t label;
  uint32_t pixels;
  float x0, y0, side;
  uint32_t frame;
  uint32_t reserved[2];
};

// A csg_crop_job with the frame size; all pointers are device memory.
struct CropArgs {
  uint32_t W, H;                 // source frames
  uint32_t S, K;                 // crop side (multiple of 4), slots per frame
  uint32_t min_pixels;
  float pad;
  uint32_t n_labels;
  int32_t explicit_boxes;
  uint32_t rgb_filter;           // CSG_CROP_FILTER_*: 1 = area filter for the RGB of minified windows
  const uint8_t* rgb;            // [n][H][W][3]
  const int32_t* instance;       // [n][H][W]
  const uint16_t* obj_coords;    // [n][H][W][3]
  const float* depth;            // [n][H][W]
  const uint32_t* stats;         // [n][n_labels][5]
  const uint8_t* eligible;       // [n_labels] or null
  uint8_t* crop_rgb;             // [n][K][S][S][3]
  uint8_t* crop_mask;            // [n][K][S][S]
  uint16_t* crop_coords;         // [n][K][S][S][3]
  float* crop_depth;             // [n][K][S][S]
  CropSlot* info;                // [n][K]
};

#ifdef __HIPCC__
// The sampling arithmetic of the crop spec (include/csg_api.h), shared by every
// kernel that must land on the same source pixels: k_crop_sample, k_crop_area
// and the amodal pass of csg_kernels.hip.  float32, each operation rounded once.
//
// The liveness rule of a slot whose window is an input (NaN fails every comparison).
__device__ __forceinline__ bool crop_label_live(const CropSlot& sl, uint32_t n_labels) {
  return sl.label >= 0 && (uint32_t)sl.label < n_labels;
}
__device__ __forceinline__ bool crop_window_live(const CropSlot& sl) {
  return sl.side > 0.0f && sl.side <= 32768.0f && fabsf(sl.x0) <= 1048576.0f && fabsf(sl.y0) <= 1048576.0f;
}
__device__ __forceinline__ float crop_step(const CropSlot& sl, uint32_t S) { return sl.side / (float)S; }
// sx of output column i (sy of row j with y0): the sample's position in source pixels
__device__ __forceinline__ float crop_sample_pos(float origin, uint32_t i, float step) {
  return origin + ((float)i + 0.5f) * step;
}
// `inside` along one axis: floorf(s) lies in [0, extent)
__device__ __forceinline__ bool crop_sample_in(float s, float extent) { return s >= 0.0f && s < extent; }
#endif

// k_crop_plan: fills info [n][K] from the frames' label statistics.
void launch_crop_plan(const CropArgs& a, uint32_t n, hipStream_t st);
// k_crop_sample: resamples every slot of info into the requested images
// (under the area filter, all but the RGB of the slots k_crop_area makes).
void launch_crop_sample(const CropArgs& a, uint32_t n, hipStream_t st);
// k_crop_area: the box-filtered RGB of every minified slot (rgb_filter = 1, crop_rgb set).
void launch_crop_area(const CropArgs& a, uint32_t n, hipStream_t st);

}  // namespace csg
