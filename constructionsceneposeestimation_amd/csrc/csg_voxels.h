// csg_voxels.h — host launcher of the voxel-cloud kernels (csg_voxels.hip),
// called by csg_passes.cpp for csg_voxel_cloud.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csg {

// One slot of a frame's open-addressing table: a voxel's key and its integer sums, one 64-byte line.
struct VxSlot {
  uint64_t key;      // kVxEmpty, or the voxel's 63-bit key (csg_voxels.hip)
  uint64_t S[3];     // sum of q_a over the voxel's points
  uint64_t R[3];     // sum of colour_k
  uint32_t minpix;   // lowest row-major pixel index among the points (0xFFFFFFFF: none yet)
  uint32_t n;        // points
};
static_assert(sizeof(VxSlot) == 64, "one slot per 64-byte line");

// The counters of one frame of a range.
struct VxFrame {
  uint32_t claimed;    // slots claimed so far
  uint32_t overflow;   // nonzero: more than C voxels; the frame's points stop on seeing it
  uint32_t dropped;    // points outside the key range
  uint32_t V;          // voxels (k_vx_scan)
};

constexpr uint64_t kVxEmpty = ~0ull;

// A csg_voxel_job with the pass's scratch, for one range of frames; all pointers are device memory.
struct VoxelArgs {
  uint32_t W, H;
  uint32_t P;            // pixels of a frame: W * H <= 2^26
  uint32_t L;            // ids -1 .. L-1 are points (0 when there is no id image)
  uint32_t C;            // records per frame of the outputs
  uint32_t Ceff;         // min(C, P): a frame has at most P voxels
  uint32_t T;            // slots per frame: the smallest power of two >= 2 * Ceff
  uint32_t BW;           // words of a frame's representative bitmap: ceil(P / 32)
  uint32_t first, n;     // the range: frames first .. first + n - 1 of the job
  uint32_t combine;      // combine runs of equal keys inside a wave before the atomics
  float s, r;            // voxel_size and fl32(1.0f / s)
  const float* points;   // [..][H][W][3]
  const uint8_t* rgb;    // or null
  const int32_t* instance;   // or null
  float* vx_xyz;         // outputs of the whole job, any but vx_total may be null
  uint8_t* vx_rgb;
  int32_t* vx_label;
  uint32_t* vx_count;
  uint32_t* vx_total;
  uint32_t* vx_dropped;
  VxSlot* slots;         // [n][T] scratch
  uint32_t* bitmap;      // [n][BW] scratch: bit p set iff pixel p is the lowest of a voxel
  uint32_t* wprefix;     // [n][BW] scratch: set bits in the words before a word
  VxFrame* frames;       // [n] scratch
};

// Enqueues the range's kernels: k_vx_init, k_vx_insert, k_vx_mark, k_vx_scan, k_vx_emit.
void launch_voxels(const VoxelArgs& a, hipStream_t st);

}  // namespace csg
