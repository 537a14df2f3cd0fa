// The stand-alone passes of libcsg.so (see include/csg_api.h): object crops, mask spans, mask PNGs, object
// points, voxel clouds, stereo-camera depth, farthest points, lens distortion and the three amodal passes.  Each validates
// its job on the host, orders itself behind the last pass that used its scratch (PassOrder, csg_ctx.h), grows
// that scratch and enqueues its kernels on the caller's stream.  None of them touches a render's work buffers.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "csg_amodal_spans.h"
#include "csg_crops.h"
#include "csg_ctx.h"
#include "csg_fps.h"
#include "csg_lens.h"
#include "csg_lens_map.h"
#include "csg_points.h"
#include "csg_spans.h"

using namespace csg;

// The checks several passes share; `who` is the entry point's name in the message.
static int check_size(csg_ctx* c, const char* who, uint32_t size) {
  if (size < 16 || size > 512 || (size & 3u))
    return c->fail(CSG_ERR_INVALID, "%s: size %u is not a multiple of 4 in 16..512", who, size);
  return CSG_OK;
}

static int check_per_frame(csg_ctx* c, const char* who, uint32_t per_frame) {
  if (per_frame < 1 || per_frame > 64)
    return c->fail(CSG_ERR_INVALID, "%s: per_frame %u outside 1..64", who, per_frame);
  return CSG_OK;
}

static int check_frame_dims(csg_ctx* c, const char* who, uint32_t width, uint32_t height) {
  if (width < 1 || width > 8192 || height < 1 || height > 8192)
    return c->fail(CSG_ERR_INVALID, "%s: frame %u x %u outside 1..8192", who, width, height);
  return CSG_OK;
}

static int check_labels(csg_ctx* c, const char* who, uint32_t n_labels) {
  if (n_labels == 0) return c->fail(CSG_ERR_INVALID, "%s: n_labels must be at least 1", who);
  if (n_labels > CSG_SPAN_MAX_LABELS)
    return c->fail(CSG_ERR_LIMIT, "%s: n_labels %u above CSG_SPAN_MAX_LABELS %u", who, n_labels, CSG_SPAN_MAX_LABELS);
  return CSG_OK;
}

static int check_resident(csg_ctx* c, const char* who, const csg_frame* frames, uint32_t n_frames) {
  for (uint32_t f = 0; f < n_frames; ++f)
    if (frames[f].xform_set >= c->set_valid.size())
      return c->fail(CSG_ERR_INVALID, "%s: frame %u: transform set %u is not resident (%u sets)", who, f,
                     frames[f].xform_set, (unsigned)c->set_valid.size());
  return CSG_OK;
}

// The stream a pass runs on: the caller's, or the context's.
static int pass_stream(csg_ctx* c, void* stream, hipStream_t* st) {
  HIP_TRY(c, hipSetDevice(c->cfg.device));
  *st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  return CSG_OK;
}

// The caller's frame records, through the pinned ring, to am_frames on `st`.
static int am_stage_frames(csg_ctx* c, const csg_frame* frames, uint32_t n_frames, hipStream_t st) {
  static_assert(sizeof(FrameDev) == sizeof(csg_frame), "frame layout");
  StageSlot<FrameDev>& slot = c->am_stage[c->am_stage_next];
  c->am_stage_next = (c->am_stage_next + 1) % kStaging;
  HIP_TRY(c, slot.upload(c->am_frames.p, n_frames, st,
                         [&](FrameDev* h) { memcpy(h, frames, sizeof(FrameDev) * n_frames); }));
  return CSG_OK;
}

// The shared front of the amodal crop passes: orders this pass behind the last amodal pass, grows the
// scratch (device frame records, n_bits words of bit image, n_keys keys) and uploads the frame records.
static int am_begin(csg_ctx* c, const csg_frame* frames, uint32_t n_frames, size_t n_bits, size_t n_keys,
                    hipStream_t st) {
  CSG_TRY(c->am.begin(c, st, c->am_frames.n < n_frames || c->am_bits.n < n_bits || c->am_keys.n < n_keys));
  HIP_TRY(c, c->am_frames.alloc(n_frames));
  HIP_TRY(c, c->am_bits.alloc(n_bits));
  HIP_TRY(c, c->am_keys.alloc(n_keys));
  return am_stage_frames(c, frames, n_frames, st);
}

extern "C" {

// Object crops: a stand-alone pass over device arrays (no scene state, no
// work buffers), so it only validates the job and enqueues the kernels.
int csg_crop_objects(csg_ctx* c, const csg_crop_job* job, uint32_t n_frames, void* stream) {
  return csg_crop_objects_filtered(c, job, CSG_CROP_FILTER_BILINEAR, n_frames, stream);
}

int csg_crop_objects_filtered(csg_ctx* c, const csg_crop_job* job, uint32_t rgb_filter, uint32_t n_frames,
                              void* stream) {
  static_assert(sizeof(CropSlot) == sizeof(csg_crop_info) && sizeof(csg_crop_info) == 32, "csg_crop_info layout");
  static_assert(offsetof(CropSlot, side) == offsetof(csg_crop_info, side) &&
                offsetof(CropSlot, frame) == offsetof(csg_crop_info, frame), "csg_crop_info layout");
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "crop_objects: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "crop_objects: no frames");
  if (rgb_filter != CSG_CROP_FILTER_BILINEAR && rgb_filter != CSG_CROP_FILTER_AREA)
    return c->fail(CSG_ERR_INVALID, "crop_objects: rgb_filter %u is neither CSG_CROP_FILTER_BILINEAR nor _AREA",
                   rgb_filter);
  CSG_TRY(check_size(c, "crop_objects", job->size));
  CSG_TRY(check_per_frame(c, "crop_objects", job->per_frame));
  if (job->min_pixels < 1) return c->fail(CSG_ERR_INVALID, "crop_objects: min_pixels must be at least 1");
  if (!std::isfinite(job->pad) || !(job->pad >= 1.0f))
    return c->fail(CSG_ERR_INVALID, "crop_objects: pad %g is not a finite value >= 1", (double)job->pad);
  if (!job->info) return c->fail(CSG_ERR_INVALID, "crop_objects: info is NULL");
  if (!job->instance) return c->fail(CSG_ERR_INVALID, "crop_objects: the instance image is always needed");
  if (job->crop_rgb && !job->rgb) return c->fail(CSG_ERR_INVALID, "crop_objects: crop_rgb needs rgb");
  if (job->crop_coords && !job->obj_coords)
    return c->fail(CSG_ERR_INVALID, "crop_objects: crop_coords needs obj_coords");
  if (job->crop_depth && !job->depth) return c->fail(CSG_ERR_INVALID, "crop_objects: crop_depth needs depth");
  if (!job->explicit_boxes && !job->inst_stats)
    return c->fail(CSG_ERR_INVALID, "crop_objects: planning needs inst_stats (or explicit_boxes = 1)");
  if (((uintptr_t)job->crop_rgb & 3u) || ((uintptr_t)job->crop_mask & 3u) || ((uintptr_t)job->crop_coords & 7u) ||
      ((uintptr_t)job->crop_depth & 15u) || ((uintptr_t)job->info & 3u))
    return c->fail(CSG_ERR_INVALID, "crop_objects: crop_rgb, crop_mask and info must be 4-byte aligned, crop_coords "
                                    "8-byte, crop_depth 16-byte");
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  CropArgs a{};
  a.W = c->cfg.width;
  a.H = c->cfg.height;
  a.S = job->size;
  a.K = job->per_frame;
  a.min_pixels = job->min_pixels;
  a.pad = job->pad;
  a.n_labels = job->n_labels;
  a.explicit_boxes = job->explicit_boxes ? 1 : 0;
  a.rgb_filter = rgb_filter;
  a.rgb = job->rgb;
  a.instance = job->instance;
  a.obj_coords = job->obj_coords;
  a.depth = job->depth;
  a.stats = job->inst_stats;
  a.eligible = job->eligible;
  a.crop_rgb = job->crop_rgb;
  a.crop_mask = job->crop_mask;
  a.crop_coords = job->crop_coords;
  a.crop_depth = job->crop_depth;
  a.info = reinterpret_cast<CropSlot*>(job->info);
  if (!a.explicit_boxes) launch_crop_plan(a, n_frames, st);
  if (a.crop_rgb || a.crop_mask || a.crop_coords || a.crop_depth) launch_crop_sample(a, n_frames, st);
  if (a.rgb_filter == CSG_CROP_FILTER_AREA && a.crop_rgb) launch_crop_area(a, n_frames, st);   // behind the plan
  HIP_TRY(c, hipGetLastError());
  return CSG_OK;
}

// Mask spans: a stand-alone pass over a device id image (no scene state, no work buffers); validates
// the job, grows the pass's own count scratch and enqueues count, scan and emit.
int csg_mask_spans(csg_ctx* c, const csg_span_job* job, uint32_t n_frames, void* stream) {
  static_assert(sizeof(SpanRec) == sizeof(csg_span) && sizeof(csg_span) == 8, "csg_span layout");
  static_assert(kSpanMaxLabels == CSG_SPAN_MAX_LABELS, "label limit");
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "mask_spans: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "mask_spans: no frames");
  if (!job->instance || !job->spans || !job->span_offsets)
    return c->fail(CSG_ERR_INVALID, "mask_spans: instance, spans and span_offsets must not be NULL");
  CSG_TRY(check_frame_dims(c, "mask_spans", job->width, job->height));
  if (job->capacity == 0) return c->fail(CSG_ERR_INVALID, "mask_spans: capacity must be at least 1");
  CSG_TRY(check_labels(c, "mask_spans", job->n_labels));
  if (((uintptr_t)job->spans & 7u) || ((uintptr_t)job->span_offsets & 3u))
    return c->fail(CSG_ERR_INVALID, "mask_spans: spans must be 8-byte aligned, span_offsets 4-byte");
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  SpanArgs a{};
  a.W = job->width;
  a.H = job->height;
  a.L = job->n_labels;
  a.G = (job->width + 63u) / 64u;
  a.C = job->capacity;
  a.instance = job->instance;
  a.spans = reinterpret_cast<SpanRec*>(job->spans);
  a.offsets = job->span_offsets;
  const size_t n_cnt = (size_t)n_frames * a.L * a.G;
  CSG_TRY(c->ms.begin(c, st, c->ms_cnt.n < n_cnt));
  HIP_TRY(c, c->ms_cnt.alloc(n_cnt));
  a.cnt = c->ms_cnt.p;
  launch_span_count(a, n_frames, st);
  launch_span_scan(a, n_frames, st);
  launch_span_emit(a, n_frames, st);
  HIP_TRY(c, hipGetLastError());
  return c->ms.end(c, st);
}

// Mask PNGs: a stand-alone pass over the span arrays (no scene state, no work buffers); validates the
// job, uploads the items, grows the pass's own scratch and enqueues the kernels.  The bit planes are
// bounded at kMaskPlaneCap bytes: a job that needs more runs as ranges of items on the stream, each
// filling and reading the same scratch and continuing file_offsets where the last one ended.
int csg_encode_span_masks(csg_ctx* c, const csg_mask_png_job* job, void* stream) {
  constexpr size_t kMaskPlaneCap = 64u << 20;
  static_assert(sizeof(MaskItem) == sizeof(csg_mask_item) && sizeof(csg_mask_item) == 8, "csg_mask_item layout");
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "encode_span_masks: null job");
  if (!job->spans || !job->span_offsets || !job->items || !job->out || !job->file_offsets)
    return c->fail(CSG_ERR_INVALID, "encode_span_masks: spans, span_offsets, items, out and file_offsets must not "
                                    "be NULL");
  if (job->n_frames == 0) return c->fail(CSG_ERR_INVALID, "encode_span_masks: no frames");
  if (job->n_items == 0) return c->fail(CSG_ERR_INVALID, "encode_span_masks: no items");
  CSG_TRY(check_frame_dims(c, "encode_span_masks", job->width, job->height));
  if (job->capacity == 0) return c->fail(CSG_ERR_INVALID, "encode_span_masks: capacity must be at least 1");
  CSG_TRY(check_labels(c, "encode_span_masks", job->n_labels));
  if (((uintptr_t)job->spans & 7u) || ((uintptr_t)job->span_offsets & 3u) || ((uintptr_t)job->file_offsets & 7u))
    return c->fail(CSG_ERR_INVALID, "encode_span_masks: spans and file_offsets must be 8-byte aligned, span_offsets "
                                    "4-byte");
  for (uint32_t i = 0; i < job->n_items; ++i)
    if (job->items[i].frame >= job->n_frames || job->items[i].label >= job->n_labels)
      return c->fail(CSG_ERR_INVALID, "encode_span_masks: item %u names frame %u of %u, label %u of %u", i,
                     job->items[i].frame, job->n_frames, job->items[i].label, job->n_labels);
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  MaskPngArgs a{};
  a.W = job->width;
  a.H = job->height;
  a.L = job->n_labels;
  a.C = job->capacity;
  a.KW = 2u * ((a.W + 63u) / 64u);
  const size_t per_item = (size_t)a.KW * a.H;   // words of one item's plane
  size_t cap = kMaskPlaneCap;
  if (const char* e = getenv("CSG_MASK_PNG_PLANE_CAP")) cap = (size_t)strtoull(e, nullptr, 10);   // (tests: bytes)
  const uint32_t range = (uint32_t)std::min<size_t>(std::min<uint32_t>(job->n_items, 65535u),   // grid y limit
                                                    std::max<size_t>(1, cap / (per_item * sizeof(uint32_t))));
  // the streams of a range that fits out_capacity fit the staging: each is shorter than its file, and
  // starts at a multiple of 4
  const uint64_t worst = ((uint64_t)mpng::max_zlib_bytes(a.W, a.H) + 3u) & ~3ull;
  const uint64_t zcap = (std::min<uint64_t>(job->out_capacity + 4ull * range, worst * range) + 15u) & ~15ull;
  const size_t n_planes = (size_t)range * per_item, n_rows = (size_t)3 * range * a.H;
  CSG_TRY(c->mp.begin(c, st, c->mp_items.n < job->n_items || c->mp_planes.n < n_planes || c->mp_rows.n < n_rows ||
                              c->mp_files.n < range + 1u || c->mp_z.n < zcap));
  HIP_TRY(c, c->mp_items.alloc(job->n_items));
  HIP_TRY(c, c->mp_planes.alloc(n_planes));
  HIP_TRY(c, c->mp_rows.alloc(n_rows));
  HIP_TRY(c, c->mp_files.alloc(range + 1u));
  HIP_TRY(c, c->mp_z.alloc(zcap));
  HIP_TRY(c, c->mp_stage.upload(c->mp_items.p, job->n_items, st,
                                [&](MaskItem* h) { memcpy(h, job->items, sizeof(MaskItem) * job->n_items); }));
  a.spans = reinterpret_cast<const SpanRec*>(job->spans);
  a.offsets = job->span_offsets;
  a.items = c->mp_items.p;
  a.planes = c->mp_planes.p;
  a.rows = c->mp_rows.p;
  a.files = c->mp_files.p;
  a.zbuf = c->mp_z.p;
  a.zcap = zcap;
  a.out = job->out;
  a.out_capacity = job->out_capacity;
  a.file_offsets = job->file_offsets;
  for (uint32_t i0 = 0; i0 < job->n_items; i0 += range) {
    a.first = i0;
    a.n = std::min(range, job->n_items - i0);
    launch_mask_png(a, st);
  }
  HIP_TRY(c, hipGetLastError());
  return c->mp.end(c, st);
}

// JPEG files: a stand-alone pass over an RGB image in device memory (no scene state, no work buffers);
// validates the job, uploads the format's tables, grows the pass's own scratch and enqueues the kernels.
// The scratch (coefficients, bit counts, staging slots) is bounded at kJpegScratchCap bytes: a job that
// needs more runs as ranges of frames on the stream, each filling and reading the same scratch and
// continuing file_offsets where the last one ended.
int csg_encode_jpeg(csg_ctx* c, const csg_jpeg_job* job, void* stream) {
  constexpr size_t kJpegScratchCap = 256u << 20;
  static_assert(jpg::k444 == CSG_JPEG_444 && jpg::k420 == CSG_JPEG_420, "subsampling values");
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "encode_jpeg: null job");
  if (!job->rgb || !job->out || !job->file_offsets)
    return c->fail(CSG_ERR_INVALID, "encode_jpeg: rgb, out and file_offsets must not be NULL");
  if (job->n_frames == 0) return c->fail(CSG_ERR_INVALID, "encode_jpeg: no frames");
  CSG_TRY(check_frame_dims(c, "encode_jpeg", job->width, job->height));
  if (job->quality < 1 || job->quality > 100)
    return c->fail(CSG_ERR_INVALID, "encode_jpeg: quality %u outside 1..100", job->quality);
  if (job->subsampling != CSG_JPEG_444 && job->subsampling != CSG_JPEG_420)
    return c->fail(CSG_ERR_INVALID, "encode_jpeg: subsampling %u is neither CSG_JPEG_444 nor CSG_JPEG_420",
                   job->subsampling);
  if ((uintptr_t)job->file_offsets & 7u) return c->fail(CSG_ERR_INVALID, "encode_jpeg: file_offsets must be 8-byte aligned");
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  JpegArgs a{};
  a.W = job->width;
  a.H = job->height;
  a.sub = job->subsampling;
  a.g = jpg::geometry(a.W, a.H, a.sub);
  a.slot = jpg::slot_bytes(a.g);
  const size_t blocks = (size_t)a.g.my * a.g.mx * a.g.bpm;   // of one frame
  const size_t per_frame = blocks * (64u * sizeof(int16_t) + sizeof(uint32_t)) + (size_t)a.g.my * (a.slot + 8u) + 8u;
  size_t cap = kJpegScratchCap;
  if (const char* e = getenv("CSG_JPEG_SCRATCH_CAP")) cap = (size_t)strtoull(e, nullptr, 10);   // (tests: bytes)
  const uint32_t range = (uint32_t)std::min<size_t>(std::min<uint32_t>(job->n_frames, 65535u),   // grid limit
                                                    std::max<size_t>(1, cap / per_frame));
  const size_t n_int = (size_t)range * a.g.my;
  CSG_TRY(c->jp.begin(c, st, c->jp_tables.n < 1 || c->jp_coef.n < range * blocks * 64u || c->jp_abits.n < range * blocks ||
                              c->jp_z.n < n_int * a.slot || c->jp_isize.n < n_int || c->jp_ipos.n < n_int ||
                              c->jp_fsize.n < range));
  HIP_TRY(c, c->jp_tables.alloc(1));
  HIP_TRY(c, c->jp_coef.alloc(range * blocks * 64u));
  HIP_TRY(c, c->jp_abits.alloc(range * blocks));
  HIP_TRY(c, c->jp_z.alloc(n_int * a.slot));
  HIP_TRY(c, c->jp_isize.alloc(n_int));
  HIP_TRY(c, c->jp_ipos.alloc(n_int));
  HIP_TRY(c, c->jp_fsize.alloc(range));
  HIP_TRY(c, c->jp_stage.upload(c->jp_tables.p, 1, st, [&](jpg::Tables* h) {
    jpg::build_tables(*h, job->width, job->height, job->quality, job->subsampling);
  }));
  a.tables = c->jp_tables.p;
  a.rgb = job->rgb;
  a.coef = c->jp_coef.p;
  a.abits = c->jp_abits.p;
  a.zbuf = c->jp_z.p;
  a.isize = c->jp_isize.p;
  a.ipos = c->jp_ipos.p;
  a.fsize = c->jp_fsize.p;
  a.out = job->out;
  a.out_capacity = job->out_capacity;
  a.file_offsets = job->file_offsets;
  for (uint32_t f0 = 0; f0 < job->n_frames; f0 += range) {
    a.first = f0;
    a.n = std::min(range, job->n_frames - f0);
    launch_jpeg(a, st);
  }
  HIP_TRY(c, hipGetLastError());
  return c->jp.end(c, st);
}

// Object points: a stand-alone pass over device arrays (no scene state, no work buffers); validates the
// job, grows the pass's own count scratch and enqueues count, scan and emit.
int csg_sample_object_points(csg_ctx* c, const csg_point_job* job, uint32_t n_frames, void* stream) {
  static_assert(kPointMaxLabels == CSG_SPAN_MAX_LABELS, "label limit");
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "sample_object_points: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "sample_object_points: no frames");
  CSG_TRY(check_frame_dims(c, "sample_object_points", job->width, job->height));
  CSG_TRY(check_labels(c, "sample_object_points", job->n_labels));
  CSG_TRY(check_per_frame(c, "sample_object_points", job->per_frame));
  if (job->samples < 16 || job->samples > 16384 || (job->samples & 3u))
    return c->fail(CSG_ERR_INVALID, "sample_object_points: samples %u is not a multiple of 4 in 16..16384",
                   job->samples);
  if (!job->instance || !job->info)
    return c->fail(CSG_ERR_INVALID, "sample_object_points: instance and info are always needed");
  if (!job->pt_count && !job->pt_choose && !job->pt_xyz && !job->pt_rgb && !job->pt_coords)
    return c->fail(CSG_ERR_INVALID, "sample_object_points: no output");
  if (job->pt_xyz && (!job->depth || !job->intrinsics))
    return c->fail(CSG_ERR_INVALID, "sample_object_points: pt_xyz needs depth and intrinsics");
  if (job->pt_rgb && !job->rgb) return c->fail(CSG_ERR_INVALID, "sample_object_points: pt_rgb needs rgb");
  if (job->pt_coords && !job->obj_coords)
    return c->fail(CSG_ERR_INVALID, "sample_object_points: pt_coords needs obj_coords");
  if ((((uintptr_t)job->instance | (uintptr_t)job->info | (uintptr_t)job->depth | (uintptr_t)job->intrinsics |
        (uintptr_t)job->frame_keys | (uintptr_t)job->pt_count | (uintptr_t)job->pt_choose | (uintptr_t)job->pt_xyz |
        (uintptr_t)job->pt_rgb) & 3u) || (((uintptr_t)job->obj_coords | (uintptr_t)job->pt_coords) & 1u))
    return c->fail(CSG_ERR_INVALID, "sample_object_points: obj_coords and pt_coords must be 2-byte aligned, every "
                                    "other pointer but rgb 4-byte");
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  PointArgs a{};
  a.W = job->width;
  a.H = job->height;
  a.P = job->width * job->height;
  a.L = job->n_labels;
  a.K = job->per_frame;
  a.N = job->samples;
  a.CH = (a.P + kPointChunk - 1u) / kPointChunk;
  a.seed = job->seed;
  a.instance = job->instance;
  a.info = reinterpret_cast<const CropSlot*>(job->info);
  a.depth = job->pt_xyz ? job->depth : nullptr;   // a source nobody asked for is never read
  a.intrinsics = job->pt_xyz ? job->intrinsics : nullptr;
  a.rgb = job->pt_rgb ? job->rgb : nullptr;
  a.obj_coords = job->pt_coords ? job->obj_coords : nullptr;
  a.frame_keys = job->frame_keys;
  a.pt_count = job->pt_count;
  a.pt_choose = job->pt_choose;
  a.pt_xyz = job->pt_xyz;
  a.pt_rgb = job->pt_rgb;
  a.pt_coords = job->pt_coords;
  const size_t n_tot = (size_t)n_frames * a.L, n_cnt = n_tot * a.CH;
  CSG_TRY(c->op.begin(c, st, c->op_cnt.n < n_cnt + n_tot));
  HIP_TRY(c, c->op_cnt.alloc(n_cnt + n_tot));
  a.cnt = c->op_cnt.p;
  a.total = c->op_cnt.p + n_cnt;
  launch_pts_count(a, n_frames, st);
  launch_pts_scan(a, n_frames, st);
  launch_pts_emit(a, n_frames, st);
  HIP_TRY(c, hipGetLastError());
  return c->op.end(c, st);
}

// Voxel clouds: a stand-alone pass over device arrays (no scene state, no work buffers); validates the
// job, grows the pass's own scratch and enqueues the kernels.  The scratch (a table of T slots of 64 bytes
// and two bitmap-sized arrays per frame) is bounded at kVoxelScratchCap bytes: a job that needs more runs
// as ranges of frames on the stream, each initialising, filling and reading the same scratch.
int csg_voxel_cloud(csg_ctx* c, const csg_voxel_job* job, uint32_t n_frames, void* stream) {
  constexpr size_t kVoxelScratchCap = 256u << 20;
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "voxel_cloud: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "voxel_cloud: no frames");
  CSG_TRY(check_frame_dims(c, "voxel_cloud", job->width, job->height));
  if (!std::isfinite(job->voxel_size) || !(job->voxel_size > 0.0f))
    return c->fail(CSG_ERR_INVALID, "voxel_cloud: voxel_size %g is not a finite value > 0", (double)job->voxel_size);
  if (job->capacity == 0) return c->fail(CSG_ERR_INVALID, "voxel_cloud: capacity must be at least 1");
  if (job->instance && (job->n_labels == 0 || job->n_labels > CSG_SPAN_MAX_LABELS))
    return c->fail(CSG_ERR_INVALID, "voxel_cloud: n_labels %u outside 1..%u", job->n_labels, CSG_SPAN_MAX_LABELS);
  if (!job->points || !job->vx_total) return c->fail(CSG_ERR_INVALID, "voxel_cloud: points and vx_total must not be NULL");
  if (((uintptr_t)job->points | (uintptr_t)job->instance | (uintptr_t)job->vx_xyz | (uintptr_t)job->vx_label |
       (uintptr_t)job->vx_count | (uintptr_t)job->vx_total | (uintptr_t)job->vx_dropped) & 3u)
    return c->fail(CSG_ERR_INVALID, "voxel_cloud: every pointer but rgb and vx_rgb must be 4-byte aligned");
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  VoxelArgs a{};
  a.W = job->width;
  a.H = job->height;
  a.P = job->width * job->height;
  a.L = job->instance ? job->n_labels : 0u;
  a.C = job->capacity;
  a.Ceff = std::min(a.C, a.P);
  a.T = 2;
  while (a.T < 2u * a.Ceff) a.T <<= 1;   // Ceff <= 2^26
  a.BW = (a.P + 31u) / 32u;
  a.s = job->voxel_size;
  a.r = 1.0f / job->voxel_size;
  a.combine = 1;
  if (const char* e = getenv("CSG_VOXEL_COMBINE")) a.combine = atoi(e) != 0;   // (A/B: 0 = an atomic per point)
  a.points = job->points;
  a.rgb = job->rgb;
  a.instance = job->instance;
  a.vx_xyz = job->vx_xyz;
  a.vx_rgb = job->vx_rgb;
  a.vx_label = job->vx_label;
  a.vx_count = job->vx_count;
  a.vx_total = job->vx_total;
  a.vx_dropped = job->vx_dropped;
  const size_t per_frame = (size_t)a.T * sizeof(VxSlot) + (size_t)a.BW * 8u + sizeof(VxFrame);
  size_t cap = kVoxelScratchCap;
  if (const char* e = getenv("CSG_VOXEL_SCRATCH_CAP")) cap = (size_t)strtoull(e, nullptr, 10);   // (tests: bytes)
  const uint32_t range = (uint32_t)std::min<size_t>(std::min<uint32_t>(n_frames, 65535u),   // grid y limit
                                                    std::max<size_t>(1, cap / per_frame));
  const size_t n_slots = (size_t)range * a.T, n_words = (size_t)range * a.BW * 2u;
  CSG_TRY(c->vx.begin(c, st, c->vx_slots.n < n_slots || c->vx_words.n < n_words || c->vx_frames.n < range));
  HIP_TRY(c, c->vx_slots.alloc(n_slots));
  HIP_TRY(c, c->vx_words.alloc(n_words));
  HIP_TRY(c, c->vx_frames.alloc(range));
  a.slots = c->vx_slots.p;
  a.bitmap = c->vx_words.p;
  a.wprefix = c->vx_words.p + (size_t)range * a.BW;
  a.frames = c->vx_frames.p;
  for (uint32_t f0 = 0; f0 < n_frames; f0 += range) {
    a.first = f0;
    a.n = std::min(range, n_frames - f0);
    launch_voxels(a, st);
  }
  HIP_TRY(c, hipGetLastError());
  return c->vx.end(c, st);
}

// Stereo-camera depth: a stand-alone pass over device arrays (no scene state, no work buffers); validates
// the job, grows the pass's own scratch and enqueues the kernels.  The scratch (an int32 of state per pixel
// and eight counters per frame) is bounded at kSensorScratchCap bytes: a job that needs more runs as ranges
// of frames on the stream, each writing and reading the same scratch.
int csg_sensor_depth(csg_ctx* c, const csg_sensor_job* job, uint32_t n_frames, void* stream) {
  constexpr size_t kSensorScratchCap = 256u << 20;
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "sensor_depth: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "sensor_depth: no frames");
  CSG_TRY(check_frame_dims(c, "sensor_depth", job->width, job->height));
  if (job->radius > 4) return c->fail(CSG_ERR_INVALID, "sensor_depth: radius %u outside 0..4", job->radius);
  const uint32_t window = (2u * job->radius + 1u) * (2u * job->radius + 1u);
  if (job->min_support < 1 || job->min_support > window)
    return c->fail(CSG_ERR_INVALID, "sensor_depth: min_support %u outside 1..%u", job->min_support, window);
  if (job->subpixel_bits > 8)
    return c->fail(CSG_ERR_INVALID, "sensor_depth: subpixel_bits %u outside 0..8", job->subpixel_bits);
  if (job->noise_k > (1u << 20)) return c->fail(CSG_ERR_INVALID, "sensor_depth: noise_k %u above 2^20", job->noise_k);
  if (job->flags & ~CSG_SENSOR_CLIP_BAND) return c->fail(CSG_ERR_INVALID, "sensor_depth: unknown flags 0x%x", job->flags);
  if (!std::isfinite(job->baseline) || job->baseline == 0.0f)
    return c->fail(CSG_ERR_INVALID, "sensor_depth: baseline %g is not a finite value other than 0", (double)job->baseline);
  if (!std::isfinite(job->z_min) || !std::isfinite(job->z_max) || !(job->z_min > 0.0f) || !(job->z_min <= job->z_max))
    return c->fail(CSG_ERR_INVALID, "sensor_depth: z_min %g, z_max %g: not finite with 0 < z_min <= z_max",
                   (double)job->z_min, (double)job->z_max);
  if (!job->depth || !job->intrinsics) return c->fail(CSG_ERR_INVALID, "sensor_depth: depth and intrinsics must not be NULL");
  if (!job->sensor_depth && !job->sensor_cause && !job->sensor_count)
    return c->fail(CSG_ERR_INVALID, "sensor_depth: no output");
  if (((uintptr_t)job->depth | (uintptr_t)job->intrinsics | (uintptr_t)job->frame_keys | (uintptr_t)job->sensor_depth |
       (uintptr_t)job->sensor_count) & 3u)
    return c->fail(CSG_ERR_INVALID, "sensor_depth: every pointer but sensor_cause must be 4-byte aligned");
  const size_t P = (size_t)job->width * job->height;
  {   // no output may overlap a source: k_sn_match writes a tile while other tiles' rows are still read
    const struct { const void* p; size_t bytes; } src[] = {{job->depth, (size_t)n_frames * P * 4u},
                                                           {job->intrinsics, (size_t)n_frames * 16u},
                                                           {job->frame_keys, (size_t)n_frames * 4u}},
        dst[] = {{job->sensor_depth, (size_t)n_frames * P * 4u}, {job->sensor_cause, (size_t)n_frames * P},
                 {job->sensor_count, (size_t)n_frames * kSnCauses * 4u}};
    for (const auto& s : src)
      for (const auto& d : dst) {
        const uintptr_t s0 = (uintptr_t)s.p, d0 = (uintptr_t)d.p;
        if (s.p && d.p && s0 < d0 + d.bytes && d0 < s0 + s.bytes)
          return c->fail(CSG_ERR_INVALID, "sensor_depth: an output overlaps a source");
      }
  }
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  SensorArgs a{};
  a.W = job->width;
  a.H = job->height;
  a.r = job->radius;
  a.min_support = job->min_support;
  a.tol = job->tol;
  a.sh = 8u - job->subpixel_bits;
  a.noise_k = job->noise_k;
  a.seed = job->seed;
  a.clip_band = job->flags & CSG_SENSOR_CLIP_BAND;
  a.abs_b = std::fabs(job->baseline);
  a.right = job->baseline > 0.0f;
  a.z_min = job->z_min;
  a.z_max = job->z_max;
  a.depth = job->depth;
  a.intrinsics = job->intrinsics;
  a.frame_keys = job->frame_keys;
  a.sensor_depth = job->sensor_depth;
  a.sensor_cause = job->sensor_cause;
  a.sensor_count = job->sensor_count;
  const size_t per_frame = P * sizeof(int32_t) + kSnCountStride * sizeof(uint32_t);
  size_t cap = kSensorScratchCap;
  if (const char* e = getenv("CSG_SENSOR_SCRATCH_CAP")) cap = (size_t)strtoull(e, nullptr, 10);   // (tests: bytes)
  const uint32_t range = (uint32_t)std::min<size_t>(std::min<uint32_t>(n_frames, 65535u),   // grid y / z limit
                                                    std::max<size_t>(1, cap / per_frame));
  const size_t n_state = (size_t)range * P, n_counts = (size_t)range * kSnCountStride;
  CSG_TRY(c->sn.begin(c, st, c->sn_state.n < n_state || c->sn_counts.n < n_counts));
  HIP_TRY(c, c->sn_state.alloc(n_state));
  HIP_TRY(c, c->sn_counts.alloc(n_counts));
  a.state = c->sn_state.p;
  a.counts = c->sn_counts.p;
  for (uint32_t f0 = 0; f0 < n_frames; f0 += range) {
    a.first = f0;
    a.n = std::min(range, n_frames - f0);
    launch_sensor(a, st);
  }
  HIP_TRY(c, hipGetLastError());
  return c->sn.end(c, st);
}

// Farthest-point sampling: a stand-alone pass over device arrays (no scene state, no work buffers, no
// scratch: a set's candidates live in its workgroup's registers, the chosen ones in its LDS); validates the
// job and enqueues one kernel, in ranges of 2^30 sets.
int csg_farthest_points(csg_ctx* c, const csg_fps_job* job, uint32_t n_sets, void* stream) {
  static_assert(CSG_FPS_MAX_PAYLOADS == kFpMaxPayloads, "payload slots");
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "farthest_points: null job");
  if (n_sets == 0) return c->fail(CSG_ERR_INVALID, "farthest_points: no sets");
  if (job->rows < 1 || job->rows > (1u << 24)) return c->fail(CSG_ERR_INVALID, "farthest_points: rows %u outside 1..2^24", job->rows);
  if (job->pool < 1 || job->pool > kFpMaxPool)
    return c->fail(CSG_ERR_INVALID, "farthest_points: pool %u outside 1..%u", job->pool, kFpMaxPool);
  if (job->samples < 1 || job->samples > kFpMaxSamples)
    return c->fail(CSG_ERR_INVALID, "farthest_points: samples %u outside 1..%u", job->samples, kFpMaxSamples);
  if (!job->xyz) return c->fail(CSG_ERR_INVALID, "farthest_points: xyz must not be NULL");
  if (job->n_payloads > kFpMaxPayloads)
    return c->fail(CSG_ERR_INVALID, "farthest_points: %u payloads, at most %u", job->n_payloads, kFpMaxPayloads);
  if (!job->fp_index && !job->fp_xyz && !job->fp_dist2 && !job->fp_count && job->n_payloads == 0)
    return c->fail(CSG_ERR_INVALID, "farthest_points: no output");
  for (uint32_t p = 0; p < job->n_payloads; ++p) {
    const csg_fps_payload& pl = job->payloads[p];
    if (!pl.src || !pl.dst) return c->fail(CSG_ERR_INVALID, "farthest_points: payload %u: src and dst must not be NULL", p);
    if (pl.row_bytes < 1 || pl.row_bytes > kFpMaxRowBytes)
      return c->fail(CSG_ERR_INVALID, "farthest_points: payload %u: row_bytes %u outside 1..%u", p, pl.row_bytes, kFpMaxRowBytes);
  }
  if (((uintptr_t)job->xyz | (uintptr_t)job->counts | (uintptr_t)job->set_keys | (uintptr_t)job->fp_index |
       (uintptr_t)job->fp_xyz | (uintptr_t)job->fp_dist2 | (uintptr_t)job->fp_count) & 3u)
    return c->fail(CSG_ERR_INVALID, "farthest_points: every pointer but the payloads' must be 4-byte aligned");
  {   // no output may overlap a source or another output: sets run concurrently and read what others write
    struct Range { const void* p; size_t bytes; };
    const size_t S = n_sets, C = job->rows, K = job->samples;
    Range src[3 + kFpMaxPayloads] = {{job->xyz, S * C * 12u}, {job->counts, S * 4u}, {job->set_keys, S * 4u}};
    Range dst[4 + kFpMaxPayloads] = {{job->fp_index, S * K * 4u}, {job->fp_xyz, S * K * 12u}, {job->fp_dist2, S * K * 4u},
                                     {job->fp_count, S * 8u}};
    for (uint32_t p = 0; p < job->n_payloads; ++p) {
      src[3 + p] = {job->payloads[p].src, S * C * job->payloads[p].row_bytes};
      dst[4 + p] = {job->payloads[p].dst, S * K * job->payloads[p].row_bytes};
    }
    auto overlap = [](const Range& x, const Range& y) {
      const uintptr_t x0 = (uintptr_t)x.p, y0 = (uintptr_t)y.p;
      return x.p && y.p && x0 < y0 + y.bytes && y0 < x0 + x.bytes;
    };
    const uint32_t n_src = 3 + job->n_payloads, n_dst = 4 + job->n_payloads;
    for (uint32_t d = 0; d < n_dst; ++d) {
      for (uint32_t s = 0; s < n_src; ++s)
        if (overlap(dst[d], src[s])) return c->fail(CSG_ERR_INVALID, "farthest_points: an output overlaps a source");
      for (uint32_t e = d + 1; e < n_dst; ++e)
        if (overlap(dst[d], dst[e])) return c->fail(CSG_ERR_INVALID, "farthest_points: two outputs overlap");
    }
  }
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  FpsArgs a{};
  a.C = job->rows;
  a.P = job->pool;
  a.K = job->samples;
  a.seed = job->seed;
  a.n_payloads = job->n_payloads;
  a.xyz = job->xyz;
  a.counts = job->counts;
  a.set_keys = job->set_keys;
  a.fp_index = job->fp_index;
  a.fp_xyz = job->fp_xyz;
  a.fp_dist2 = job->fp_dist2;
  a.fp_count = job->fp_count;
  for (uint32_t p = 0; p < job->n_payloads; ++p)
    a.payload[p] = {static_cast<const uint8_t*>(job->payloads[p].src), static_cast<uint8_t*>(job->payloads[p].dst),
                    job->payloads[p].row_bytes, job->payloads[p].fill & 0xFFu};
  constexpr uint32_t kRange = 1u << 30;   // workgroups of a launch
  for (uint32_t s0 = 0; s0 < n_sets;) {
    const uint32_t n = std::min(kRange, n_sets - s0);
    a.first = s0;
    launch_fps(a, n, st);
    s0 += n;
  }
  HIP_TRY(c, hipGetLastError());
  return CSG_OK;
}

// Lens distortion.  The map is host arithmetic alone (csg_lens_map.h): no context, no GPU.
int csg_lens_map(const csg_lens_model* m, int32_t* map, uint32_t* counts) { return lens_map(m, map, counts); }

// The resampling: a stand-alone pass over device arrays (no scene state, no work buffers, no scratch: the
// statistics are reduced into the outputs themselves); validates the job and enqueues the kernels.
int csg_lens_remap(csg_ctx* c, const csg_lens_job* job, uint32_t n_frames, void* stream) {
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "lens_remap: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "lens_remap: no frames");
  CSG_TRY(check_frame_dims(c, "lens_remap", job->width, job->height));
  CSG_TRY(check_frame_dims(c, "lens_remap", job->src_width, job->src_height));
  if (job->rgb_filter != CSG_LENS_FILTER_BILINEAR && job->rgb_filter != CSG_LENS_FILTER_NEAREST)
    return c->fail(CSG_ERR_INVALID, "lens_remap: rgb_filter %u is neither CSG_LENS_FILTER_BILINEAR nor _NEAREST",
                   job->rgb_filter);
  if (!job->map) return c->fail(CSG_ERR_INVALID, "lens_remap: map is NULL");
  if (!job->lens_rgb && !job->lens_instance && !job->lens_depth && !job->lens_coords && !job->lens_valid &&
      !job->lens_stats && !job->lens_count)
    return c->fail(CSG_ERR_INVALID, "lens_remap: no output");
  if (job->lens_rgb && !job->rgb) return c->fail(CSG_ERR_INVALID, "lens_remap: lens_rgb needs rgb");
  if ((job->lens_instance || job->lens_stats) && !job->instance)
    return c->fail(CSG_ERR_INVALID, "lens_remap: lens_instance and lens_stats need instance");
  if (job->lens_depth && !job->depth) return c->fail(CSG_ERR_INVALID, "lens_remap: lens_depth needs depth");
  if (job->lens_coords && !job->obj_coords) return c->fail(CSG_ERR_INVALID, "lens_remap: lens_coords needs obj_coords");
  if (job->lens_stats) CSG_TRY(check_labels(c, "lens_remap", job->n_labels));
  if (((uintptr_t)job->map & 7u) || ((uintptr_t)job->obj_coords & 1u) ||
      (((uintptr_t)job->instance | (uintptr_t)job->depth | (uintptr_t)job->lens_rgb | (uintptr_t)job->lens_instance |
        (uintptr_t)job->lens_depth | (uintptr_t)job->lens_coords | (uintptr_t)job->lens_stats | (uintptr_t)job->lens_count) & 3u))
    return c->fail(CSG_ERR_INVALID, "lens_remap: map must be 8-byte aligned, obj_coords 2-byte, every other pointer but "
                                    "rgb and lens_valid 4-byte");
  const size_t P = (size_t)job->width * job->height, SP = (size_t)job->src_width * job->src_height, n = n_frames;
  {   // no output may overlap a source, the map or another output
    struct Range { const void* p; size_t bytes; };
    const Range src[] = {{job->map, P * 8u}, {job->rgb, n * SP * 3u}, {job->instance, n * SP * 4u},
                         {job->depth, n * SP * 4u}, {job->obj_coords, n * SP * 6u}};
    const Range dst[] = {{job->lens_rgb, n * P * 3u}, {job->lens_instance, n * P * 4u}, {job->lens_depth, n * P * 4u},
                         {job->lens_coords, n * P * 6u}, {job->lens_valid, n * P},
                         {job->lens_stats, n * job->n_labels * 20u}, {job->lens_count, n * kLnCauses * 4u}};
    auto overlap = [](const Range& x, const Range& y) {
      const uintptr_t x0 = (uintptr_t)x.p, y0 = (uintptr_t)y.p;
      return x.p && y.p && x0 < y0 + y.bytes && y0 < x0 + x.bytes;
    };
    constexpr size_t n_dst = sizeof dst / sizeof dst[0];
    for (size_t d = 0; d < n_dst; ++d) {
      for (const Range& s : src)
        if (overlap(dst[d], s)) return c->fail(CSG_ERR_INVALID, "lens_remap: an output overlaps a source");
      for (size_t e = d + 1; e < n_dst; ++e)
        if (overlap(dst[d], dst[e])) return c->fail(CSG_ERR_INVALID, "lens_remap: two outputs overlap");
    }
  }
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  LensArgs a{};
  a.W = job->width;
  a.H = job->height;
  a.SW = job->src_width;
  a.SH = job->src_height;
  a.n = n_frames;
  a.n_labels = job->lens_stats ? job->n_labels : 0u;
  a.nearest = job->rgb_filter == CSG_LENS_FILTER_NEAREST;
  a.map = job->map;
  a.rgb = job->rgb;
  a.instance = job->instance;
  a.depth = job->depth;
  a.obj_coords = job->obj_coords;
  a.lens_rgb = job->lens_rgb;
  a.lens_instance = job->lens_instance;
  a.lens_depth = job->lens_depth;
  a.lens_coords = job->lens_coords;
  a.lens_valid = job->lens_valid;
  a.lens_stats = job->lens_stats;
  a.lens_count = job->lens_count;
  launch_lens(a, st);
  HIP_TRY(c, hipGetLastError());
  return CSG_OK;
}

// The keypoints through the forward model: validates, rounds the model to float32 and enqueues one kernel.
int csg_lens_points(csg_ctx* c, const csg_lens_job* job, uint32_t n_frames, void* stream) {
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "lens_points: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "lens_points: no frames");
  if (!lens_model_ok(job->model)) return c->fail(CSG_ERR_INVALID, "lens_points: model is NULL or not one csg_lens_map takes");
  if (job->n_keypoints < 1 || job->n_keypoints > 65536u)
    return c->fail(CSG_ERR_INVALID, "lens_points: n_keypoints %u outside 1..65536", job->n_keypoints);
  const size_t total = (size_t)n_frames * job->n_keypoints;
  if (total > (1u << 30)) return c->fail(CSG_ERR_INVALID, "lens_points: more than 2^30 keypoints");
  if (!job->keypoints_uv || !job->keypoints_vis || !job->lens_uv || !job->lens_vis)
    return c->fail(CSG_ERR_INVALID, "lens_points: keypoints_uv, keypoints_vis, lens_uv and lens_vis must not be NULL");
  if (((uintptr_t)job->keypoints_uv | (uintptr_t)job->keypoints_vis | (uintptr_t)job->lens_uv | (uintptr_t)job->lens_vis) & 3u)
    return c->fail(CSG_ERR_INVALID, "lens_points: every pointer must be 4-byte aligned");
  {
    struct Range { const void* p; size_t bytes; };
    const Range r[] = {{job->lens_uv, total * 8u}, {job->lens_vis, total * 4u}, {job->keypoints_uv, total * 8u},
                       {job->keypoints_vis, total * 4u}};
    for (size_t d = 0; d < 2; ++d)
      for (size_t s = d + 1; s < 4; ++s) {
        const uintptr_t x0 = (uintptr_t)r[d].p, y0 = (uintptr_t)r[s].p;
        if (x0 < y0 + r[s].bytes && y0 < x0 + r[d].bytes)
          return c->fail(CSG_ERR_INVALID, "lens_points: an output overlaps a source or the other output");
      }
  }
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  const csg_lens_model& m = *job->model;
  LensPointArgs a{};
  a.W = (float)m.width;
  a.H = (float)m.height;
  a.fx = (float)m.fx;
  a.fy = (float)m.fy;
  a.cx = (float)m.cx;
  a.cy = (float)m.cy;
  a.sfx = (float)m.sfx;
  a.sfy = (float)m.sfy;
  a.scx = (float)m.scx;
  a.scy = (float)m.scy;
  a.k1 = (float)m.k1;
  a.k2 = (float)m.k2;
  a.p1 = (float)m.p1;
  a.p2 = (float)m.p2;
  a.k3 = (float)m.k3;
  a.k4 = (float)m.k4;
  a.k5 = (float)m.k5;
  a.k6 = (float)m.k6;
  a.total = (uint32_t)total;
  a.uv = job->keypoints_uv;
  a.vis = job->keypoints_vis;
  a.lens_uv = job->lens_uv;
  a.lens_vis = job->lens_vis;
  launch_lens_points(a, st);
  HIP_TRY(c, hipGetLastError());
  return CSG_OK;
}

// Amodal crop masks: reads the scene tables (synced here as a render syncs them) and the caller's
// `info`; everything it writes besides the output is scratch of its own.
int csg_crop_amodal(csg_ctx* c, const csg_amodal_job* job, uint32_t n_frames, void* stream) {
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "crop_amodal: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "crop_amodal: no frames");
  CSG_TRY(check_size(c, "crop_amodal", job->size));
  CSG_TRY(check_per_frame(c, "crop_amodal", job->per_frame));
  if (!job->frames) return c->fail(CSG_ERR_INVALID, "crop_amodal: frames is NULL");
  if (!job->info) return c->fail(CSG_ERR_INVALID, "crop_amodal: info is NULL");
  if (!job->crop_amodal) return c->fail(CSG_ERR_INVALID, "crop_amodal: crop_amodal is NULL");
  if (((uintptr_t)job->crop_amodal & 3u) || ((uintptr_t)job->info & 3u))
    return c->fail(CSG_ERR_INVALID, "crop_amodal: crop_amodal and info must be 4-byte aligned");
  if (!c->have_scene) return c->fail(CSG_ERR_INVALID, "crop_amodal: no scene uploaded");
  CSG_TRY(check_resident(c, "crop_amodal", job->frames, n_frames));
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  CSG_TRY(sync_scene_state(c));
  const uint32_t S = job->size, K = job->per_frame, words = (S * S + 31u) / 32u;
  const size_t n_bits = (size_t)n_frames * K * words;
  CSG_TRY(am_begin(c, job->frames, n_frames, n_bits, 0, st));
  HIP_TRY(c, hipMemsetAsync(c->am_bits.p, 0, n_bits * sizeof(uint32_t), st));
  AmodalDev a{};
  a.S = S;
  a.K = K;
  a.n_labels = c->n_lab;
  a.n_sets = (uint32_t)c->set_valid.size();
  a.words = words;
  a.frames = c->am_frames.p;
  a.info = reinterpret_cast<const CropSlot*>(job->info);
  a.lab_off = c->lab_off.p;
  a.lab_chunks = c->lab_chunks.p;
  a.chunks = c->chunks.p;
  a.models = c->models.p;
  a.iset = c->iset.p;
  a.bits = c->am_bits.p;
  a.out = job->crop_amodal;
  launch_crop_amodal(scene_dev(c), a, n_frames, c->lab_max_chunks, st);
  HIP_TRY(c, hipGetLastError());
  return c->am.end(c, st);
}

// Amodal depth and object coordinates: the same pass keeping, per sample, the largest 1/W instead of a
// bit.  The keys (4 B per sample) live in crop_amodal_depth when it is given -- the finish pass converts
// them in place --, else in scratch of the pass's own, bounded at kAmKeyCap bytes: the job then runs as
// frame ranges on the stream, each zeroing, filling and finishing the same scratch.
int csg_crop_amodal_geometry(csg_ctx* c, const csg_amodal_geometry_job* job, uint32_t n_frames, void* stream) {
  constexpr size_t kAmKeyCap = 64u << 20;
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "crop_amodal_geometry: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "crop_amodal_geometry: no frames");
  CSG_TRY(check_size(c, "crop_amodal_geometry", job->size));
  CSG_TRY(check_per_frame(c, "crop_amodal_geometry", job->per_frame));
  if (!job->frames) return c->fail(CSG_ERR_INVALID, "crop_amodal_geometry: frames is NULL");
  if (!job->info) return c->fail(CSG_ERR_INVALID, "crop_amodal_geometry: info is NULL");
  if (!job->crop_amodal && !job->crop_amodal_depth && !job->crop_amodal_coords)
    return c->fail(CSG_ERR_INVALID, "crop_amodal_geometry: crop_amodal, crop_amodal_depth and crop_amodal_coords "
                                    "are all NULL");
  if (((uintptr_t)job->crop_amodal & 3u) || ((uintptr_t)job->info & 3u) || ((uintptr_t)job->crop_amodal_depth & 15u) ||
      ((uintptr_t)job->crop_amodal_coords & 7u))
    return c->fail(CSG_ERR_INVALID, "crop_amodal_geometry: crop_amodal and info must be 4-byte aligned, "
                                    "crop_amodal_coords 8-byte, crop_amodal_depth 16-byte");
  if (!c->have_scene) return c->fail(CSG_ERR_INVALID, "crop_amodal_geometry: no scene uploaded");
  CSG_TRY(check_resident(c, "crop_amodal_geometry", job->frames, n_frames));
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  CSG_TRY(sync_scene_state(c));
  if (job->crop_amodal_coords) CSG_TRY(sync_object_frames(c));
  const uint32_t S = job->size, K = job->per_frame;
  const size_t per_frame = (size_t)K * S * S;   // samples, and keys, of one frame
  uint32_t range = n_frames;                    // frames per range; the depth output holds every key
  if (!job->crop_amodal_depth) {
    size_t cap = kAmKeyCap;
    if (const char* e = getenv("CSG_AMODAL_KEY_CAP")) cap = (size_t)strtoull(e, nullptr, 10);   // (tests: bytes)
    range = (uint32_t)std::min<size_t>(n_frames, std::max<size_t>(1, cap / (per_frame * sizeof(uint32_t))));
  }
  CSG_TRY(am_begin(c, job->frames, n_frames, 0, job->crop_amodal_depth ? 0 : (size_t)range * per_frame, st));
  AmodalDev a{};
  a.S = S;
  a.K = K;
  a.n_labels = c->n_lab;
  a.n_sets = (uint32_t)c->set_valid.size();
  a.words = S * S;
  a.lab_off = c->lab_off.p;
  a.lab_chunks = c->lab_chunks.p;
  a.chunks = c->chunks.p;
  a.models = c->models.p;
  a.iset = c->iset.p;
  AmodalGeomOut g{};
  g.W = c->cfg.width;
  g.H = c->cfg.height;
  g.table = c->of.p;
  for (uint32_t f0 = 0; f0 < n_frames; f0 += range) {   // every array from the range's first frame
    const uint32_t nf = std::min(range, n_frames - f0);
    const size_t at = (size_t)f0 * per_frame;
    a.frames = c->am_frames.p + f0;
    a.info = reinterpret_cast<const CropSlot*>(job->info) + (size_t)f0 * K;
    g.mask = job->crop_amodal ? job->crop_amodal + at : nullptr;
    g.depth = job->crop_amodal_depth ? job->crop_amodal_depth + at : nullptr;
    g.coords = job->crop_amodal_coords ? job->crop_amodal_coords + at * 3 : nullptr;
    a.bits = g.depth ? reinterpret_cast<uint32_t*>(g.depth) : c->am_keys.p;
    HIP_TRY(c, hipMemsetAsync(a.bits, 0, (size_t)nf * per_frame * sizeof(uint32_t), st));
    launch_crop_amodal_geometry(scene_dev(c), a, g, nf, c->lab_max_chunks, st);
  }
  HIP_TRY(c, hipGetLastError());
  return c->am.end(c, st);
}

// Full-frame amodal spans: the scene tables and the caller's frames as the other amodal passes read
// them; bit planes, counts and tables are scratch of the pass's own.  The planes are bounded at
// kAmPlaneCap bytes: a job that needs more runs as frame ranges on the stream, each zeroing, filling and
// reading the same scratch.
int csg_amodal_spans(csg_ctx* c, const csg_amodal_span_job* job, uint32_t n_frames, void* stream) {
  constexpr size_t kAmPlaneCap = 64u << 20;
  if (!c) return CSG_ERR_INVALID;
  if (!job) return c->fail(CSG_ERR_INVALID, "amodal_spans: null job");
  if (n_frames == 0) return c->fail(CSG_ERR_INVALID, "amodal_spans: no frames");
  if (!job->frames) return c->fail(CSG_ERR_INVALID, "amodal_spans: frames is NULL");
  if (!job->spans || !job->span_offsets)
    return c->fail(CSG_ERR_INVALID, "amodal_spans: spans and span_offsets must not be NULL");
  if (job->capacity == 0) return c->fail(CSG_ERR_INVALID, "amodal_spans: capacity must be at least 1");
  if (((uintptr_t)job->spans & 7u) || ((uintptr_t)job->span_offsets & 3u) || ((uintptr_t)job->amodal_stats & 3u))
    return c->fail(CSG_ERR_INVALID, "amodal_spans: spans must be 8-byte aligned, span_offsets and amodal_stats 4-byte");
  if (!c->have_scene) return c->fail(CSG_ERR_INVALID, "amodal_spans: no scene uploaded");
  if (c->n_lab > CSG_SPAN_MAX_LABELS)
    return c->fail(CSG_ERR_LIMIT, "amodal_spans: %u labels above CSG_SPAN_MAX_LABELS %u", c->n_lab, CSG_SPAN_MAX_LABELS);
  CSG_TRY(check_resident(c, "amodal_spans", job->frames, n_frames));
  hipStream_t st;
  CSG_TRY(pass_stream(c, stream, &st));
  CSG_TRY(sync_scene_state(c));
  const uint32_t L = c->n_lab, W = c->cfg.width, H = c->cfg.height;
  const uint32_t G = (W + 63u) / 64u, HW = (H + 31u) / 32u;
  // the job's table: label -> plane, then one (chunk, plane) item per chunk of an eligible label, as all
  // the items' chunks followed by all their planes
  std::vector<uint32_t> tab(L, kNoPlane), items_p;
  uint32_t P = 0;
  for (uint32_t l = 0; l < L; ++l) {
    if (job->eligible && !job->eligible[l]) continue;
    tab[l] = P;
    for (uint32_t k = c->h_lab_off[l]; k < c->h_lab_off[l + 1]; ++k) {
      tab.push_back(c->h_lab_chunks[k]);
      items_p.push_back(P);
    }
    ++P;
  }
  const uint32_t n_items = (uint32_t)items_p.size();
  tab.insert(tab.end(), items_p.begin(), items_p.end());
  const size_t n_tab = tab.size();
  const size_t per_frame = (size_t)P * HW * W;   // words of one frame's planes
  size_t cap = kAmPlaneCap;
  if (const char* e = getenv("CSG_AMODAL_PLANE_CAP")) cap = (size_t)strtoull(e, nullptr, 10);   // (tests: bytes)
  uint32_t range = std::min<uint32_t>(n_frames, 65535u);   // grid z limit
  if (per_frame) range = (uint32_t)std::min<size_t>(range, std::max<size_t>(1, cap / (per_frame * sizeof(uint32_t))));
  const size_t n_planes = (size_t)range * per_frame, n_touched = (size_t)range * std::max(P, 1u);
  const size_t n_cnt = (size_t)range * L * G;
  CSG_TRY(c->am.begin(c, st, c->as_planes.n < n_planes || c->as_touched.n < n_touched || c->as_cnt.n < n_cnt ||
                              c->as_tables.n < n_tab || c->am_frames.n < n_frames));
  HIP_TRY(c, c->as_planes.alloc(n_planes));
  HIP_TRY(c, c->as_touched.alloc(n_touched));
  HIP_TRY(c, c->as_cnt.alloc(n_cnt));
  HIP_TRY(c, c->as_tables.alloc(n_tab));
  HIP_TRY(c, c->am_frames.alloc(n_frames));
  CSG_TRY(am_stage_frames(c, job->frames, n_frames, st));
  HIP_TRY(c, c->as_stage.upload(c->as_tables.p, n_tab, st,
                                [&](uint32_t* h) { memcpy(h, tab.data(), sizeof(uint32_t) * n_tab); }));
  AmodalSpanDev a{};
  a.W = W;
  a.H = H;
  a.L = L;
  a.P = P;
  a.G = G;
  a.HW = HW;
  a.C = job->capacity;
  a.n_sets = (uint32_t)c->set_valid.size();
  a.n_items = n_items;
  a.plane_of = c->as_tables.p;
  a.item_chunk = c->as_tables.p + L;
  a.item_plane = c->as_tables.p + L + n_items;
  a.chunks = c->chunks.p;
  a.models = c->models.p;
  a.iset = c->iset.p;
  a.planes = c->as_planes.p;
  a.touched = c->as_touched.p;
  a.cnt = c->as_cnt.p;
  for (uint32_t f0 = 0; f0 < n_frames; f0 += range) {   // every array from the range's first frame
    const uint32_t nf = std::min(range, n_frames - f0);
    a.frames = c->am_frames.p + f0;
    a.spans = reinterpret_cast<SpanRec*>(job->spans) + (size_t)f0 * a.C;
    a.offsets = job->span_offsets + (size_t)f0 * (L + 1u);
    a.stats = job->amodal_stats ? job->amodal_stats + (size_t)f0 * L * 5u : nullptr;
    if (per_frame) HIP_TRY(c, hipMemsetAsync(a.planes, 0, (size_t)nf * per_frame * sizeof(uint32_t), st));
    HIP_TRY(c, hipMemsetAsync(a.touched, 0, n_touched * sizeof(uint32_t), st));
    launch_amodal_spans(scene_dev(c), a, nf, st);
  }
  HIP_TRY(c, hipGetLastError());
  return c->am.end(c, st);
}

}  // extern "C"
