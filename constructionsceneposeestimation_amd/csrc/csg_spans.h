// csg_spans.h — host launchers of the mask-span kernels (csg_spans.hip),
// called by csg_passes.cpp for csg_mask_spans.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csg {

// One span: the layout of csg_span (include/csg_api.h), 8 bytes.
struct SpanRec {
  uint32_t start, len;
};

// A csg_span_job with the pass's scratch; all pointers are device memory.
struct SpanArgs {
  uint32_t W, H;              // the job's frames
  uint32_t L;                 // labels: ids 0 .. L-1 belong to a label
  uint32_t G;                 // groups of 64 columns: ceil(W / 64)
  uint32_t C;                 // span records a frame may hold
  const int32_t* instance;    // [n][H][W]
  SpanRec* spans;             // [n][C]
  uint32_t* offsets;          // [n][L + 1]
  uint32_t* cnt;              // [n][L][G] scratch: span counts (k_span_count), then their exclusive scan
};

constexpr uint32_t kSpanMaxLabels = 256;   // [L][64] uint32 of LDS per wave: 64 KiB at the limit

// k_span_count: spans of every (frame, label, column group) into cnt.
void launch_span_count(const SpanArgs& a, uint32_t n, hipStream_t st);
// k_span_scan: cnt -> its exclusive scan per frame (label-major), and offsets.
void launch_span_scan(const SpanArgs& a, uint32_t n, hipStream_t st);
// k_span_emit: every span record at its final position.
void launch_span_emit(const SpanArgs& a, uint32_t n, hipStream_t st);

}  // namespace csg
