// Internal to the host code of libcsg.so: the context (struct csg_ctx), the types that own its device
// memory, pinned memory and events, and the few helpers csg_api.cpp and csg_passes.cpp share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/csg_api.h"
#include "csg_encode.h"
#include "csg_jpeg.h"
#include "csg_kernels.h"
#include "csg_mask_png.h"
#include "csg_sensor.h"
#include "csg_voxels.h"

namespace csg {

// A device allocation owned by one object: freed by release() or at the end
// of its scope (a local scratch buffer cannot leak on an early error return).
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t alloc(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (count == 0) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

// Page-locked host memory, grow-only like DevBuf::alloc.  Whoever grows it has waited for its readers.
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  size_t n = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t alloc(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    if (count == 0) return hipSuccess;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) n = count;
    return e;
  }
};

// An ordering event (no timing), created on first use.
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t ensure() { return e ? hipSuccess : hipEventCreateWithFlags(&e, hipEventDisableTiming); }
};

// Pinned staging for one H2D copy at a time: the slot is refilled only after the copy that read it has
// completed (its event), so back-to-back asynchronous jobs never see each other's host data.  A ring is
// StageSlot<T> slots[kStaging] plus a `next` index.
template <class T>
struct StageSlot {
  PinnedBuf<T> buf;
  Event copied;
  bool busy = false;   // `copied` has been recorded
  // fill(T*) writes the n elements that go to `dst` on `st`
  template <class Fill>
  hipError_t upload(T* dst, size_t n, hipStream_t st, Fill fill) {
    hipError_t e = copied.ensure();
    if (e == hipSuccess && busy) e = hipEventSynchronize(copied.e);   // the slot's last H2D copy is done
    if (e == hipSuccess) e = buf.alloc(n);
    if (e != hipSuccess) return e;
    fill(buf.p);
    e = hipMemcpyAsync(dst, buf.p, sizeof(T) * n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(copied.e, st);
    if (e == hipSuccess) busy = true;
    return e;
  }
};

// Orders a stand-alone pass behind the last pass that used the same scratch, on whichever stream that
// ran: a pass that is about to reallocate scratch waits for it on the host (the last pass still reads
// what is freed), any other pass on a different stream waits on the device (it overwrites what the last
// pass reads), and every pass records the event at its end.
struct PassOrder {
  Event done;
  hipStream_t stream = nullptr;   // of the last pass
  bool busy = false;              // `done` has been recorded
  int begin(csg_ctx* c, hipStream_t st, bool will_reallocate);
  int end(csg_ctx* c, hipStream_t st);
  int wait_host(csg_ctx* c);      // for whoever rewrites what a pass on any stream may still read
};

struct HostTexture {
  std::vector<uint8_t> rgba;
  uint32_t w = 0, h = 0;
  bool present = false;
};

constexpr uint32_t kStaging = 4;   // slots of a staging ring

}  // namespace csg

struct csg_ctx {
  template <class T> using DevBuf = csg::DevBuf<T>;
  using FrameDev = csg::FrameDev;
  csg_config cfg{};
  std::string err;
  hipStream_t stream = nullptr;
  uint32_t tiles_x = 0, tiles_y = 0, n_tiles = 0;

  // scene
  bool have_scene = false;
  uint32_t n_inst = 0, n_meshes = 0, n_materials = 0;
  uint64_t n_tris_total = 0;
  DevBuf<float> tri_pos, tri_uv;       // de-indexed triangle soup (see SceneDev)
  // Alpha trim (csg_alpha_box.h): one opaque uv box per soup triangle, built by sync_scene_state from the
  // mesh's authored alpha texture and threshold (h_abox_tex: that texture per mesh, -1: no box built).
  // CSG_ALPHA_TRIM=0 uploads "full" boxes and sets no InstSetDev::trim: nothing is trimmed (A/B, tests).
  DevBuf<float> abox;                   // [T][4] u_lo u_hi v_lo v_hi
  std::vector<float> h_tri_uv;          // host copy of tri_uv (the boxes are rebuilt when textures change)
  std::vector<int32_t> h_abox_tex;      // per mesh
  bool alpha_trim = true;
  DevBuf<csg::InstDesc> inst;
  std::vector<csg::MatDesc> h_mats;
  std::vector<csg::MatDesc> h_set_mats;      // [sets][n_materials] as uploaded
  std::vector<csg::MeshDesc> h_meshes;
  DevBuf<csg::Chunk> chunks;
  uint32_t n_chunks = 0;
  uint32_t uid_shift = csg::kUidShift;       // SceneDev::uid_shift
  std::vector<csg::HostTexture> textures;
  bool tex_dirty = true;
  DevBuf<uint8_t> texels;
  DevBuf<uint32_t> aquad;
  DevBuf<uint32_t> acls;                // alpha-test class of each alpha quad (see build_alpha_classes)
  std::vector<int> acls_thr;            // per texture: the threshold acls was built for
  DevBuf<csg::TexDesc> texd;
  csg::LightDev light{{0.26f, 0.29f, 0.34f}, {0.78f, 0.78f, 0.78f}, {0.7071f, 0.f, 0.7071f},
                      191u | (217u << 8) | (255u << 16)};   // default (csg_set_light)
  // domain randomisation per transform set (csg_set_dr_light / csg_set_dr_textures)
  std::vector<csg::LightDev> dr_light;
  std::vector<uint8_t> dr_light_valid;
  std::vector<int32_t> dr_tex;          // [sets][n_materials]; kKeepTexture = the material's own
  bool dr_dirty = true;
  DevBuf<csg::LightDev> lights;
  DevBuf<csg::MatDesc> set_mats;
  uint32_t n_table_sets = 0;
  std::vector<float> h_models;          // [sets][I][16]
  std::vector<uint8_t> set_valid;
  DevBuf<float> models;
  bool models_dirty = true;
  uint32_t n_kp = 0;
  std::vector<float> h_kp;              // [sets][K][3]
  std::vector<uint8_t> kp_valid;
  DevBuf<float> kp;
  bool kp_dirty = true;
  // object frames (csg_set_object_frames): per set and label a 3x4 world -> unit-box matrix
  uint32_t n_lab = 1;                   // label-table length: largest instance label + 1, at least 1
  std::vector<float> h_of;              // [sets][n_lab][12], zeros where never set
  uint32_t of_sets = 0;                 // sets h_of holds
  DevBuf<float> of;                     // [of_table_sets][n_lab][12] (sync_object_frames)
  uint32_t of_table_sets = 0;
  bool of_dirty = true;

  // per-batch work buffers: record and bin pools shared by the frames of a
  // launch chain, each frame's region (Slab) planned by k_plan from its hints
  // or the per-frame caps rec_cap / bin_cap
  uint32_t rec_cap = 0, bin_cap = 0, work_frames = 0;
  uint64_t rec_pool = 0, bin_pool = 0;            // pool entries allocated
  bool use_hints = false;                         // csg_size_work sized the pools from frame hints
  uint32_t hint_fallbacks = 0;                    // re-renders the hinted pools caused (csg_work_info)
  uint64_t plan_rec_pool = 0, plan_bin_pool = 0;  // ... to these
  DevBuf<csg::Slab> slab;                         // [chain frames] (k_plan)
  DevBuf<uint64_t> plan_need;                     // [2] pool entries the batch's largest chain asked for (k_plan)
  DevBuf<FrameDev> frames;
  // Pinned staging ring for host frame records (sized to cfg.max_frames by ensure_work): a batch's
  // records are copied into the next slot, so back-to-back async batches never render each other's cameras.
  csg::StageSlot<FrameDev> stage[csg::kStaging];
  uint32_t stage_next = 0;
  // The stream of the most recent enqueue.  The work buffers are shared, so a
  // batch on a different stream first waits for the previous stream to drain;
  // csg_synchronize waits on it.
  hipStream_t last_stream = nullptr;
  DevBuf<uint32_t> fset;                // [chain frames] checked transform set of each frame (k_clip)
  DevBuf<float> clip, pv;
  DevBuf<csg::Rec> recs;
  DevBuf<uint32_t> rect, rec_count, tile_count, tile_off, bins, overflow;
  DevBuf<uint32_t> bcount;              // [chain frames][bin_blocks][n_tiles] count grid
  DevBuf<csg::InstSetDev> iset;         // [n_table_sets][n_inst] resolved materials (sync_scene_state)
  std::vector<csg::InstDesc> h_inst;    // host copy of the instance table
  // internal outputs (host-output mode / scratch)
  DevBuf<uint8_t> o_rgb;
  DevBuf<int32_t> o_inst;
  DevBuf<float> o_depth, o_kp_uv, kp_w, o_points, cam;
  DevBuf<uint16_t> o_normals;
  DevBuf<uint16_t> o_objc;              // object coordinates (host-output mode)
  DevBuf<int32_t> o_kp_vis;
  DevBuf<uint32_t> kp_pix, kp_tiles;
  DevBuf<uint32_t> o_stats;
  DevBuf<uint8_t> o_dvis;               // depth visualisation (host-output mode)
  DevBuf<float> o_drange;
  DevBuf<uint32_t> o_cov;               // label coverage (host-output mode)
  DevBuf<uint32_t> drange;              // [2][chain frames] min / max depth bits (k_raster's resolve)
  DevBuf<uint32_t> jet;                 // JET colour map, 256 x (r | g << 8 | b << 16)
  // images of the last batch (for the file encoders) and the encoders' buffers
  const uint8_t* last_rgb = nullptr;
  const float* last_depth = nullptr;
  const float* last_points = nullptr;
  const uint8_t* last_dvis = nullptr;
  DevBuf<csg::EncPng> enc_rgb, enc_dpng, enc_d16;
  DevBuf<uint2> enc_rowsum;
  DevBuf<uint32_t> enc_rows_rgb, enc_rows_dpng, enc_rows_csv, enc_rows_pcd, enc_rows_d16, enc_rows_ply, enc_ply_n;
  DevBuf<uint8_t> enc_d16img;           // [F][H][W] big-endian 16-bit depth samples
  DevBuf<uint64_t> enc_fsize, enc_foff, enc_zoff;
  DevBuf<uint8_t> enc_zbuf, enc_out;
  DevBuf<uint8_t> dstat_part;           // depth-statistics partial sums
  DevBuf<double> o_dstats;              // depth statistics (host-output mode)
  float depth16_scale = 250.0f;         // counts per metre of the batch's 16-bit depth PNGs
  uint64_t enc_total = 0;               // bytes of the last batch's files (0: none)
  uint32_t enc_nfiles = 0;
  std::vector<uint64_t> h_foff;

  // timing: ring of per-batch event quintuples (recorded, never waited on in the loop)
  bool timing = true;
  static constexpr uint32_t kRing = 4096;
  std::vector<hipEvent_t> ring;         // kRing * 5
  std::vector<uint32_t> ring_frames;
  uint64_t ring_count = 0;
  hipEvent_t* ev = nullptr;             // events of the most recent batch
  uint32_t last_F = 0;
  uint32_t dbg = 0;                     // CSG_DEBUG ablation bits (profiling builds of the pipeline only)
  // k_count / k_bin workgroups per frame (CSG_BINBLOCKS: A/B only; set in
  // csg_create from the tile count).  16 at 1080p's 4,080 tiles of 32 x 16
  // keeps the [blocks][tiles] count grid the size 32 blocks gave 32 x 32 tiles
  // (C3: binning 2.27 vs 2.69 ms per 960 frames with 16 vs 32 blocks; at 2,880
  // frames per step 8 / 16 / 24 blocks: binning 5.8 / 6.2 / 6.3 ms, k_raster
  // 97.3 / 97.1 / 96.9 ms); 8 above 8,192 tiles (C5 at 4K, 16,200 tiles, 480
  // frames: binning 4.3 / 4.7 / 4.4 / 5.2 ms with 8 / 16 / 4 / 2 blocks;
  // profiles/r05/ab/tile_shape.md)
  uint32_t bin_blocks = 32;
  uint32_t chain_frames = 0;            // frames per launch chain (cfg.frames_per_launch; CSG_CHAIN overrides)
  // Host outputs: each launch chain's slice is copied to the host on copy_stream
  // while the next chains render (created with the first host-output batch).
  static constexpr uint32_t kCopyEv = 16;
  hipStream_t copy_stream = nullptr;
  csg::Event copy_ev[kCopyEv];
  csg::Event copy_done;
  // The host wire of the instance ids (csg_widen.h): a host-output batch's ids
  // cross PCIe as (id + 1) in ids_bytes (1 with at most 255 labels, 2 with at
  // most 65,535; 4 = int32 as rendered, no narrowing) and are widened to the
  // caller's int32 by WidenPool threads while later chains render.
  // CSG_NARROW_IDS=0 keeps int32 on the wire (A/B, tests).
  uint32_t ids_bytes = 4;               // set by csg_upload_scene from the label range
  bool narrow_ids = true;
  bool split_pageable = true;           // CSG_SPLIT_PAGEABLE=0: pageable host outputs as one chain (A/B, tests)
  DevBuf<uint8_t> o_ids_n;              // [F][H][W] narrowed ids (device)
  csg::PinnedBuf<uint8_t> h_ids_n;      // ... their pinned host landing buffer
  // Amodal passes (csg_crop_amodal, csg_crop_amodal_geometry, csg_amodal_spans).  The label -> chunks
  // table is built with the scene.  The passes have scratch of their own, grown to the job and never
  // shared with a render, under one order (am): device copies of the frame records, behind a pinned
  // staging ring for the host records, the crops' bit image and key image, and the spans' bit planes of
  // one frame range, their "touched" words, the span counts, and the item and label -> plane tables
  // behind their staging slot.
  DevBuf<uint32_t> lab_off, lab_chunks;   // [n_lab + 1], [chunks that carry a label >= 0]
  uint32_t lab_max_chunks = 0;            // the most chunks one label has
  std::vector<uint32_t> h_lab_off, h_lab_chunks;   // host copies (csg_amodal_spans builds a job's item list from them)
  csg::PassOrder am;
  DevBuf<FrameDev> am_frames;
  csg::StageSlot<FrameDev> am_stage[csg::kStaging];
  uint32_t am_stage_next = 0;
  DevBuf<uint32_t> am_bits;
  DevBuf<uint32_t> am_keys;               // csg_crop_amodal_geometry without a depth output: the key image
  DevBuf<uint32_t> as_planes, as_touched, as_cnt, as_tables;
  csg::StageSlot<uint32_t> as_stage;
  // Mask spans (csg_mask_spans): the pass's own scratch, the span counts [n][L][groups of 64 columns],
  // grown to the job, under an order of its own.
  DevBuf<uint32_t> ms_cnt;
  csg::PassOrder ms;
  // Object points (csg_sample_object_points): the pass's own scratch, the pixel counts [n][L][chunks] and
  // the totals [n][L] behind them, grown to the job, under an order of its own.
  DevBuf<uint32_t> op_cnt;
  csg::PassOrder op;
  // Mask PNGs (csg_encode_span_masks): the pass's own scratch -- the items behind their staging slot, and
  // of one range of items the bit planes, the per-row numbers, the per-file layout and the zlib staging --
  // grown to the job, under an order of its own.
  DevBuf<csg::MaskItem> mp_items;
  csg::StageSlot<csg::MaskItem> mp_stage;
  DevBuf<uint32_t> mp_planes, mp_rows;
  DevBuf<csg::MaskFile> mp_files;
  DevBuf<uint8_t> mp_z;
  csg::PassOrder mp;
  // JPEG files (csg_encode_jpeg): the pass's own scratch -- the format's tables behind their staging slot, and
  // of one range of frames the coefficients, the blocks' AC bits, the intervals' staging slots, sizes and
  // positions and the files' sizes -- grown to the job, under an order of its own.
  DevBuf<csg::jpg::Tables> jp_tables;
  csg::StageSlot<csg::jpg::Tables> jp_stage;
  DevBuf<int16_t> jp_coef;
  DevBuf<uint32_t> jp_abits, jp_isize, jp_ipos;
  DevBuf<uint8_t> jp_z;
  DevBuf<uint64_t> jp_fsize;
  csg::PassOrder jp;
  // Voxel clouds (csg_voxel_cloud): the pass's own scratch -- of one range of frames the tables, the
  // bitmaps of the voxels' lowest pixels with their word prefixes, and the frames' counters -- grown to the
  // job, under an order of its own.
  DevBuf<csg::VxSlot> vx_slots;
  DevBuf<uint32_t> vx_words;
  DevBuf<csg::VxFrame> vx_frames;
  csg::PassOrder vx;
  // Stereo-camera depth (csg_sensor_depth): the pass's own scratch -- of one range of frames the state
  // image (an int32 per pixel) and the causes' counters -- grown to the job, under an order of its own.
  DevBuf<int32_t> sn_state;
  DevBuf<uint32_t> sn_counts;
  csg::PassOrder sn;
  // csg_keep_depth / csg_last_depth: host-output batches render their depth into o_depth whether or not anything copies it
  bool keep_depth = false;
  const float* kept_depth = nullptr;
  uint32_t kept_depth_frames = 0;
  // csg_keep_points / csg_last_points: host-output batches render their points into o_points whether or not anything copies them
  bool keep_points = false;
  const float* kept_points = nullptr;
  uint32_t kept_points_frames = 0;
  // csg_keep_rgb / csg_last_rgb: host-output batches render their RGB into o_rgb whether or not anything copies it
  bool keep_rgb = false;
  const uint8_t* kept_rgb = nullptr;
  uint32_t kept_rgb_frames = 0;
  // csg_keep_instance / csg_last_instance: host-output batches keep their ids on the device
  bool keep_ids = false;
  const int32_t* last_inst = nullptr;
  uint32_t last_inst_frames = 0;
  // the last sizing pass (csg_size_work)
  uint32_t sized_frames = 0, sized_max_rec = 0, sized_max_bin = 0;
  double sized_mean_rec = 0.0, sized_mean_bin = 0.0;

  int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
};

#define HIP_TRY(ctx, expr)                                                                           \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                            \
      return (ctx)->fail(_e == hipErrorOutOfMemory ? CSG_ERR_OOM : CSG_ERR_DEVICE, "%s: %s", #expr,  \
                         hipGetErrorString(_e));                                                     \
  } while (0)

// ... and the same for a call that returns a status of ours.
#define CSG_TRY(call)       \
  do {                      \
    const int _rc = (call); \
    if (_rc) return _rc;    \
  } while (0)

namespace csg {

inline int PassOrder::begin(csg_ctx* c, hipStream_t st, bool will_reallocate) {
  HIP_TRY(c, done.ensure());
  if (busy) {
    if (will_reallocate) HIP_TRY(c, hipEventSynchronize(done.e));
    else if (stream != st) HIP_TRY(c, hipStreamWaitEvent(st, done.e, 0));
  }
  return CSG_OK;
}

inline int PassOrder::end(csg_ctx* c, hipStream_t st) {
  HIP_TRY(c, hipEventRecord(done.e, st));
  stream = st;
  busy = true;
  return CSG_OK;
}

inline int PassOrder::wait_host(csg_ctx* c) {
  if (busy) HIP_TRY(c, hipEventSynchronize(done.e));
  return CSG_OK;
}

// csg_api.cpp, for the passes of csg_passes.cpp:
int drain(csg_ctx* c);                // wait for everything the context enqueued on its own and the last batch's stream
int sync_scene_state(csg_ctx* c);     // bring the device tables of the scene up to date
int sync_object_frames(csg_ctx* c);   // ... and the object-frame table
SceneDev scene_dev(const csg_ctx* c);

}  // namespace csg
