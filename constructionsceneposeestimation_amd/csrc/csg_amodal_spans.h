// csg_amodal_spans.h — host launcher of the full-frame amodal span kernels
// (csg_amodal_spans.hip), called by csg_passes.cpp for csg_amodal_spans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csg_kernels.h"
#include "csg_spans.h"

namespace csg {

constexpr uint32_t kNoPlane = 0xFFFFFFFFu;   // plane_of[] of a label that is not eligible

// One frame range of a csg_amodal_span_job with the pass's scratch; all pointers are device memory
// and start at the range's first frame.
struct AmodalSpanDev {
  uint32_t W, H;                 // the context's frames
  uint32_t L;                    // label-table length
  uint32_t P;                    // planes per frame: the eligible labels
  uint32_t G;                    // groups of 64 columns: ceil(W / 64)
  uint32_t HW;                   // word rows of a plane: ceil(H / 32)
  uint32_t C;                    // span records a frame may hold
  uint32_t n_sets;               // transform sets in models / iset
  uint32_t n_items;              // (chunk, plane) items: the chunks of every eligible label
  const FrameDev* frames;        // [n]
  const uint32_t* item_chunk;    // [n_items] chunk index
  const uint32_t* item_plane;    // [n_items] the plane of the chunk's label
  const uint32_t* plane_of;      // [L] label -> plane (kNoPlane: not eligible)
  const Chunk* chunks;
  const float* models;           // [n_sets][I][16]
  const InstSetDev* iset;        // [n_sets][I]
  uint32_t* planes;              // [n][P][HW][W] bit y & 31 of word (y >> 5, x); zeroed by the caller
  uint32_t* touched;             // [n][P] non-zero: some block set a bit of the plane; zeroed by the caller
  SpanRec* spans;                // [n][C]
  uint32_t* offsets;             // [n][L + 1]
  uint32_t* cnt;                 // [n][L][G] span counts, then (k_span_scan) their exclusive scan
  uint32_t* stats;               // [n][L][5] pixels, minx, miny, maxx, maxy, or null
};

// k_amodal_plane, k_aplane_init, k_aplane_count, k_span_scan (csg_spans.hip) and k_aplane_emit for n frames
// (n <= 65535: one range of the job).
void launch_amodal_spans(const SceneDev& s, const AmodalSpanDev& a, uint32_t n, hipStream_t st);

}  // namespace csg
