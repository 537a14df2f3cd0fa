/*
 * csg_api.h — C ABI of the MI355X construction-scene frame generator
 * (libcsg.so, built for gfx950).  Plain C99: no C++ or torch types cross
 * this boundary.  Every entry point returns 0 on success, a negative
 * csg_status on failure; csg_last_error() gives the message.
 *
 * What each entry point replaces in the reference
 * (xander683/ConstructionScenePoseEstimation, generate_construction_data.py):
 *
 *   csg_create ................ Camera(prim_path, resolution) + clip/focal/aperture
 *                               setup + camera.initialize()           :1421-1453
 *   csg_upload_scene .......... the USD stage the RTX renderer reads  :1370
 *   csg_upload_texture ........ material texture binding (OmniPBR
 *                               diffuse/opacity maps)                 world2 materials
 *   csg_set_light ............. setup_scene_lighting (dome 500,
 *                               distant light clamped to 1500)        :1289-1345
 *   csg_set_instance_transforms randomize_object_positions' xformOp
 *                               edits (every 10 frames)               :914-1231, :1542
 *   csg_set_dr_light / ........ per-epoch domain randomisation (dome tint,
 *   csg_set_dr_textures         sun, texture swap; C4 of BASELINE.json)
 *   csg_set_keypoints ......... (new) 3D points whose 2D projection is
 *                               annotated; the reference produces none
 *   csg_set_object_frames ..... (new) per transform set, each label's world -> unit-box
 *                               matrix for csg_outputs.obj_coords (the dense object-
 *                               coordinate / NOCS label); the reference produces none
 *   csg_render_batch .......... camera.set_world_pose + next_update_async
 *                               + get_rgba / distance_to_image_plane /
 *                               instance_segmentation .get_data()     :1586-1595, :1669,
 *                                                                     :1681, :1475/:1909
 *   csg_project_keypoints ..... 3D->2D projection with the frame's
 *                               intrinsics (pinhole of :646-649)
 *   csg_outputs.file_kinds .... the frame's files encoded on the GPU:
 *                               cv2.imwrite of the RGB and JET depth
 *                               images, np.savetxt of the depth  :1672-1673,
 *                               and of the point cloud           :1687-1709,
 *                                                                :714-775, :1716-1757
 *                               plus two compact kinds without a reference
 *                               counterpart: the point cloud as a binary PLY
 *                               and the depth as a 16-bit greyscale PNG
 *   csg_copy_files / csg_host_alloc / csg_host_free (pinned buffers for them)
 *   csg_encode_files .......... (new) the same encoders on device arrays the
 *                               caller supplies, at the job's own frame size
 *   csg_size_work / csg_get_work_info (per-frame work-buffer caps measured
 *                               on a sample of frames; no reference counterpart:
 *                               Kit sizes its own render buffers)
 *   csg_host_id_bytes ......... width of the instance ids on the host wire
 *                               (int32 mask of :1909-1910 narrowed to
 *                               id + 1 bytes on PCIe, widened on the host)
 *   csg_crop_objects .......... (new) fixed-size zoomed-in patches around the largest
 *                               visible objects of each frame (RGB, visible mask, object
 *                               coordinates, depth and the windows they were cut from),
 *                               the input of two-stage pose networks; the reference
 *                               produces none (its users crop whole frames on the host)
 *   csg_crop_objects_filtered . the same with an exact area filter for the RGB of
 *                               minified windows (CSG_CROP_FILTER_AREA)
 *   csg_crop_amodal ........... (new) the amodal mask of each crop: the object's full
 *                               silhouette as if nothing stood in front of it (BOP's
 *                               `mask` next to `mask_visib`), rasterised from the scene
 *                               at the crop's own sample positions; the reference
 *                               would render the frame once more per object
 *   csg_crop_amodal_geometry .. (new) the amodal depth and object coordinates of each
 *                               crop (and its amodal mask) from one pass of the same kind
 *   csg_mask_spans ............ (new) per-object run-length masks (COCO RLE spans) of
 *                               the visible ids
 *   csg_amodal_spans .......... (new) the same spans of every object's amodal mask over
 *                               the whole frame, with its amodal box and pixel count
 *   csg_encode_span_masks ..... (new) those spans as finished per-object mask PNG files
 *                               (BOP's `mask_visib` / `mask` folders), packed in device memory
 *   csg_encode_jpeg ........... (new) RGB frames in device memory as finished baseline JPEG
 *                               files (BOP's `rgb/%06d.jpg`), packed in device memory
 *   csg_sample_object_points .. (new) N pixels of each object's visible mask with their
 *                               image indices, camera-frame points, colours and object
 *                               coordinates: the input of the point-based pose networks
 *   csg_voxel_cloud ........... (new) the frame's world-space points voxel-downsampled on a
 *                               world-fixed grid, one labelled record per (cell, object)
 *   csg_sensor_depth .......... (new) a depth image as a stereo depth camera would return
 *                               it: half-occlusion holes, window erosion, quantised and noisy
 *                               disparity, with the cause of every missing value
 *   csg_farthest_points ....... (new) farthest-point samples of point sets (the point samples,
 *                               the voxel clouds), with payload rows carried along
 *   csg_lens_map / csg_lens_remap / csg_lens_points  (new) frames and their labels as a
 *                               camera with lens distortion (Brown-Conrady) shows them
 *   csg_last_error / csg_destroy
 *
 * Threading: several contexts may share a device (each has its own stream
 * and work buffers; the generator drives two from two threads); a context is
 * used by one thread at a time.  The only process-wide state is the pool of
 * host threads that widens narrowed instance ids (csg_host_id_bytes).
 */
#ifndef CSG_API_H
#define CSG_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSG_ABI_VERSION 14

typedef enum {
  CSG_OK = 0,
  CSG_ERR_INVALID = -1,      /* bad argument / state */
  CSG_ERR_DEVICE = -2,       /* HIP runtime error */
  CSG_ERR_OOM = -3,          /* device allocation failed */
  CSG_ERR_OVERFLOW = -4,     /* a per-frame work buffer overflowed; raise caps */
  CSG_ERR_LIMIT = -5,        /* scene exceeds a fixed limit (instances, tris/mesh) */
  CSG_ERR_CAPACITY = -6      /* csg_outputs.files too small: file_offsets[n_files] holds the
                                bytes needed; csg_copy_files fetches them without rendering again */
} csg_status;

typedef struct csg_ctx csg_ctx;

typedef struct {
  int32_t device;            /* HIP device ordinal (after HIP_VISIBLE_DEVICES) */
  uint32_t width, height;    /* output resolution, e.g. 1920x1080; at most 8192 x 8192 (256 x 512
                                tiles of 32 x 16: CSG_ERR_INVALID beyond) */
  uint32_t max_frames;       /* frames per csg_render_batch call (work buffers sized for it) */
  float near_clip, far_clip; /* 0.5 / 250 m, generate_construction_data.py:1437; in [2^-126, 2^126] */
  uint32_t records_per_frame;/* raster-triangle capacity per frame (0 = auto) */
  uint32_t bins_per_frame;   /* tile-bin entry capacity per frame (0 = auto) */
  uint32_t frames_per_launch;/* frames per kernel chain inside a batch (0 = the whole batch):
                                work buffers are sized for one chain, so this bounds their
                                memory independently of max_frames */
} csg_config;

typedef struct {
  const float* positions;    /* [n_vertices][3] object space */
  uint32_t n_vertices;
  const uint32_t* indices;   /* [n_tris][3] */
  uint32_t n_tris;           /* < 2^20 */
  const float* uvs;          /* [n_uvs][2] USD st, or NULL */
  uint32_t n_uvs;
  const uint32_t* uv_indices;/* [n_tris][3] into uvs, or NULL */
  uint32_t material;
} csg_mesh;

typedef struct {
  uint8_t base_color[4];     /* sRGB u8 albedo multiplier (alpha unused) */
  int32_t texture;           /* texture id or -1 */
  uint32_t alpha_test;       /* 1: discard fragments with texture alpha <= threshold */
  uint32_t alpha_threshold;  /* 0..255 (alpha is 8-bit) */
} csg_material;

typedef struct {
  float model[16];           /* row-major 4x4, column-vector convention p' = M p */
  uint32_t mesh;
  int32_t inst_idx;          /* value written to the instance mask; -1 = background */
  uint32_t reserved[2];
} csg_instance;

typedef struct {
  float ambient[3];          /* dome light contribution per channel */
  float sun[3];              /* distant light contribution per channel */
  float sun_dir[3];          /* unit vector toward the sun, world space */
  uint8_t sky[4];            /* background RGB */
} csg_light;

/* The rotation of `view` must have a positive determinant (a proper look-at).
 * The normals output is flipped by the sign of the screen-space determinant
 * of the triangle, which faces the camera only then: under an improper view
 * (determinant < 0) every normal faces away from the camera, while ids, depth,
 * RGB, points, obj_coords and keypoints are what the geometry says
 * (DESIGN.md section 3, item 8). */
typedef struct {
  float view[16];            /* row-major world->camera (USD camera: -Z forward), rotation of det > 0 */
  float proj[16];            /* row-major; rows 0,1,3 give (u*w, v*w, w) in pixels */
  uint32_t xform_set;        /* instance-transform set (randomisation epoch) */
  uint32_t frame_id;
  uint32_t records_hint;     /* work to reserve for this frame: raster records and tile-bin */
  uint32_t bins_hint;        /* entries; csg_size_work writes them (0 = the per-frame caps) */
} csg_frame;

typedef struct {
  /* Caller-owned buffers, [n_frames] leading dimension.  Any may be NULL. */
  uint8_t* rgb;              /* [n][H][W][3] */
  int32_t* instance;         /* [n][H][W], -1 background */
  float* depth;              /* [n][H][W] distance to image plane, +inf no hit */
  float* keypoints_uv;       /* [n][K][2] pixels */
  int32_t* keypoints_vis;    /* [n][K] 0 out/behind, 1 occluded, 2 visible */
  uint32_t* inst_stats;      /* [n][n_labels][5] = pixels, minx, miny, maxx, maxy */
  uint32_t n_labels;
  int32_t on_device;         /* 1: device pointers (stay in HBM; instance, depth and points
                                16-B aligned, normals and obj_coords 8 B, rgb 4 B: CSG_ERR_INVALID otherwise,
                                as k_raster stores 4-pixel groups), 0: host pointers */
  uint16_t* normals;         /* [n][H][W][3] f16 bits: unit world-space face normal facing
                                the camera; 0 where nothing is hit (C5 normals) */
  float* points;             /* [n][H][W][3] world-space point of each pixel from its depth
                                (depth_to_pointcloud GDP:616-711, fused); NaN where no hit */
  uint8_t* depth_vis;        /* [n][H][W][3] RGB: the reference's depth PNG (GDP:1690-1709):
                                valid depth (finite, > 0) normalised by the frame's min / max,
                                JET colour map (OpenCV COLORMAP_JET), black if nothing is hit */
  float* depth_range;        /* [n][2] min, max of the valid depth (NaN, NaN: nothing hit) */
  uint32_t* label_covered;   /* [n][n_labels] pixels each label would cover unoccluded: a
                                fragment of it covers the centre, lies in the depth range and
                                passes the alpha test (no depth test).  Bit 31 set = unknown
                                (a 32x32 tile held more than 32 labels).  occlusionRatio =
                                1 - pixels / covered (bounding_box_3d, GDP:1780-1790) */
  /* Files encoded on the GPU (csg_render_batch only, not the async form).
   * file_kinds: bit set of CSG_FILE_*; per frame one file per kind, in bit
   * order: file j = frame * n_kinds + k.  The packed bytes of all files go to
   * `files` (host memory, files_cap bytes; pinned memory from csg_host_alloc
   * copies at full PCIe rate), file j at [file_offsets[j], file_offsets[j + 1])
   * (file_offsets: n_frames * n_kinds + 1 entries).  The images a kind needs
   * are rendered to internal scratch when the caller did not ask for them. */
  uint32_t file_kinds;
  uint32_t pad_files;
  uint8_t* files;
  uint64_t files_cap;
  uint64_t* file_offsets;
  double* depth_stats;       /* [n][6] per frame: valid pixels (finite, > 0), zero pixels, infinite
                                pixels, sum / min / max of the valid depths (the reference's
                                DataQualityLogger.log_depth, GDP:318-341); the sum in float64 in a
                                fixed order (64 partial sums per frame, then in order) */
  uint16_t* obj_coords;      /* [n][H][W][3] object coordinates (NOCS): the pixel's surface point in its
                                object's frame, normalised to the object's box (csg_set_object_frames) and
                                quantised: u = (uint16)(min(max(q, 0), 1) * 65535 + 0.5) per axis, q =
                                A * (the pixel's `points` value) with A the frame's set's matrix of the
                                pixel's instance id.  (0, 0, 0) where the id is -1 -- also the value of the
                                box's low corner: the instance image tells them apart -- and for labels
                                without a box or sets without a table.  Parts of an articulated object
                                (human limbs, crane parts) are expressed in the object root's frame and
                                box; a posed part that leaves that box is clamped.  8-B aligned with
                                on_device = 1.  Depth and ids it needs are rendered to internal scratch
                                when the caller did not ask for them. */
  float depth16_counts_per_metre; /* scale of CSG_FILE_DEPTH16_PNG: sample = depth in metres * this.  0 = the
                                default, 250 (4 mm steps; 65535 / 250 = 262.1 m covers the default 250 m far
                                clip).  Negative or not finite: CSG_ERR_INVALID (csg_render_batch) */
} csg_outputs;

/* csg_outputs.file_kinds */
#define CSG_FILE_RGB_PNG 1u        /* 8-bit RGB PNG of the frame (cv2.imwrite, GDP:1672-1673): filter Sub,
                                      one dynamic-Huffman deflate block of literals and distance-1 matches,
                                      2 KiB IDAT chunks */
#define CSG_FILE_DEPTH_CSV 2u      /* np.savetxt(depth, fmt="%.6f", delimiter=" ") text (GDP:1687-1688),
                                      byte-identical */
#define CSG_FILE_DEPTH_PNG 4u      /* the JET depth visualisation (csg_outputs.depth_vis) as a PNG
                                      (GDP:1690-1709) */
#define CSG_FILE_POINTCLOUD_TXT 8u /* np.savetxt(np.hstack([xyz, rgb]), fmt="%.6f", delimiter=" ",
                                      header="x y z r g b", comments="") of the pixels with a point
                                      (csg_outputs.points not NaN), row-major (GDP:766-770,
                                      :1716-1757), byte-identical */
#define CSG_FILE_POINTCLOUD_PLY 16u /* the same points as a binary PLY: the header
                                        ply\n
                                        format binary_little_endian 1.0\n
                                        element vertex <N>\n            (N plain decimal)
                                        property float x\n  property float y\n  property float z\n
                                        property uchar red\n  property uchar green\n  property uchar blue\n
                                        end_header\n
                                      (one property per line, no indentation), then N records of 15 bytes:
                                      the pixel's three float32 of csg_outputs.points as a bit copy
                                      (little-endian; -0.0 stays -0.0) and its three RGB bytes.  A pixel is
                                      a point under the TXT kind's rule (no NaN in x, y, z); row-major.  A
                                      frame without a point is the header with "element vertex 0" */
#define CSG_FILE_DEPTH16_PNG 32u   /* the depth as a 16-bit greyscale PNG (bit depth 16, colour type 0; filter
                                      Sub at distance 2, otherwise encoded as the RGB PNG) at s =
                                      depth16_counts_per_metre: sample v = 0 where the depth is not finite
                                      or <= 0, else t = fl32(d * s), v = 65535 if t >= 65535, else
                                      (uint32) fl32(t + 0.5f) (multiply and add rounded separately).  So a
                                      valid depth below half a count reads 0 like "no hit", and depths
                                      beyond 65535 / s saturate at 65535 */

typedef struct {
  uint64_t records;          /* raster triangles emitted (all frames of the last launch chain) */
  uint64_t bin_entries;      /* tile-bin entries (same frames) */
  uint32_t frames;           /* frames of the last launch chain */
  uint32_t pad;
  float ms_setup, ms_bin, ms_raster, ms_keypoints, ms_total;   /* HIP-event timings */
} csg_batch_stats;

int csg_create(const csg_config* cfg, csg_ctx** out);
void csg_destroy(csg_ctx* ctx);
const char* csg_last_error(const csg_ctx* ctx);
int csg_abi_version(void);

int csg_upload_scene(csg_ctx* ctx, const csg_mesh* meshes, uint32_t n_meshes,
                     const csg_material* materials, uint32_t n_materials,
                     const csg_instance* instances, uint32_t n_instances);
int csg_upload_texture(csg_ctx* ctx, uint32_t tex_id, const uint8_t* rgba8, uint32_t width,
                       uint32_t height);
int csg_set_light(csg_ctx* ctx, const csg_light* light);
/* n must equal the scene's instance count; set_id < 65536 (also for the per-set calls below). */
int csg_set_instance_transforms(csg_ctx* ctx, uint32_t set_id, const float* model4x4, uint32_t n);
/* World-space keypoints of one transform set: [n][3]; n is fixed per scene. */
int csg_set_keypoints(csg_ctx* ctx, uint32_t set_id, const float* pts_world, uint32_t n);
/* Object frames of one transform set for csg_outputs.obj_coords: per label a
 * row-major 3x4 float32 matrix [n][12] taking a world point to the label's
 * unit box, diag(1 / (hi - lo)) * (T_obj^-1 with lo subtracted from the
 * translation), computed in float64 and rounded once.  n must equal the
 * scene's label-table length (largest inst_idx + 1, at least 1); every value
 * finite (CSG_ERR_INVALID otherwise).  All-zero rows give output 0: the rule
 * for labels without a box and for instances of no object; sets that never
 * got a table hold zeros. */
int csg_set_object_frames(csg_ctx* ctx, uint32_t set_id, const float* world_to_unit, uint32_t n);

/* Domain randomisation per transform set (randomisation epoch; C4).
 * csg_set_dr_light: the set's lighting (dome tint/intensity, sun), replacing
 * the csg_set_light default for frames of that set.
 * csg_set_dr_textures: per material, the texture the set uses: a texture id,
 * -1 for none, or CSG_KEEP_TEXTURE for the material's own; n = n_materials. */
#define CSG_KEEP_TEXTURE (-2)
int csg_set_dr_light(csg_ctx* ctx, uint32_t set_id, const csg_light* light);
int csg_set_dr_textures(csg_ctx* ctx, uint32_t set_id, const int32_t* texture_per_material, uint32_t n);

/* Render n_frames (<= max_frames) frames; synchronous.  A work buffer that
 * overflows (records or bin entries past the configured caps) is grown from
 * the device counters and the batch rendered again, up to 6 attempts; the
 * results do not depend on the caps.  An overflow left by an earlier
 * asynchronous batch is reported first (CSG_ERR_OVERFLOW), as by
 * csg_synchronize.  With host outputs the batch runs as launch chains of an
 * eighth of it (at least 32 frames), each chain's outputs copied to the host
 * on a copy stream while later chains render (CSG_SPLIT_PAGEABLE=0 at
 * csg_create: pageable destinations as one chain).
 *
 * Alpha-tested records are trimmed to their triangle's opaque uv box, computed
 * at upload from the mesh uvs, the authored alpha texture and its threshold
 * (DESIGN.md section 3, item 6): fewer records, bin entries and fragments, the
 * same outputs.  CSG_ALPHA_TRIM=0 at csg_create uploads "full" boxes and
 * renders untrimmed (A/B, tests); csg_get_batch_stats' records and bin_entries
 * show the difference. */
int csg_render_batch(csg_ctx* ctx, const csg_frame* frames, uint32_t n_frames, const csg_outputs* out);
/* Same, enqueued on `stream` (a hipStream_t, NULL = context stream); frames
 * may be a device pointer when frames_on_device = 1.  Returns after enqueue;
 * the work buffers are not grown.  Host frame records are staged through a
 * ring of pinned buffers, so the caller may reuse `frames` at once.  A batch
 * on a different stream than the previous one waits for that stream first
 * (one set of work buffers per context).  Device frame records are checked on
 * the device: a transform set >= the sets uploaded renders with set 0, a
 * keypoint set never uploaded projects nothing, and both are reported by the
 * next csg_synchronize (CSG_ERR_INVALID).  Sets inside the range that were
 * never uploaded hold zero transforms (nothing is drawn). */
int csg_render_batch_async(csg_ctx* ctx, const csg_frame* frames, uint32_t n_frames,
                           int32_t frames_on_device, const csg_outputs* out, void* stream);
/* Wait for every batch enqueued so far (context stream and the caller's
 * stream of the last batch).  Overflow and device-set errors are sticky
 * across asynchronous batches: any batch since the last csg_synchronize /
 * csg_render_batch that truncated its records or bin lists makes this return
 * CSG_ERR_OVERFLOW (then the flag is cleared). */
int csg_synchronize(csg_ctx* ctx);
int csg_get_batch_stats(csg_ctx* ctx, csg_batch_stats* st);

/* Per-stage device time accumulated with HIP events recorded on the launch
 * stream for every launch chain since the last reset (no host sync inside
 * the timed loop); `batches` counts launch chains.  Stages: setup = k_clip+k_setup, bin = k_count+k_scan+k_bin,
 * keypoints = k_keypoints (projection), raster = k_raster (tile raster,
 * keypoint depth test, resolve). */
typedef struct {
  uint32_t batches;          /* launch chains accumulated (capped at the ring size, 4096) */
  uint32_t frames;           /* frames in those batches */
  double ms_setup, ms_bin, ms_raster, ms_keypoints;
} csg_timing;
int csg_timing_reset(csg_ctx* ctx);
int csg_timing_read(csg_ctx* ctx, csg_timing* out);

/* World-space AABB of each instance's vertices under transform set set_id,
 * out [n_instances][6] = xmin, ymin, zmin, xmax, ymax, zmax (host buffer);
 * the GPU side of the bounding_box_3d annotator (GDP:1780-1790). */
int csg_instance_bounds(csg_ctx* ctx, uint32_t set_id, float* out);

/* The files of the last csg_render_batch that asked for files, again
 * (after CSG_ERR_CAPACITY): dst host memory of cap bytes; offsets as
 * csg_outputs.file_offsets (may be NULL). */
int csg_copy_files(csg_ctx* ctx, uint8_t* dst, uint64_t cap, uint64_t* offsets);
/* The file encoders on device arrays the caller supplies instead of a rendered
 * batch's: the same passes csg_render_batch runs for csg_outputs.file_kinds
 * and csg_outputs.depth_stats, so any array of the layouts below -- a render's
 * outputs kept in HBM, or synthetic data -- becomes the same files.  The frame
 * size is the job's, not the context's (1..8192 each way); n_frames is not
 * bound by max_frames (the encoders' scratch grows with the job).  Files and
 * offsets are laid out as csg_outputs says: file j = frame * n_kinds + k.
 *
 * Synchronous: waits for the context's earlier work (as csg_synchronize, whose
 * errors it returns), runs on the context's stream and returns with `files`
 * and `depth_stats` written.  The caller's arrays must be complete before the
 * call (work on other streams is not waited for).  CSG_ERR_INVALID for a NULL
 * source of a requested kind (see the members), a zero or too large
 * dimension, n_frames == 0, an unknown kind, a depth16_counts_per_metre that
 * is negative or not finite, depth or points off 4-byte alignment, or nothing
 * asked for.  CSG_ERR_CAPACITY when files_cap is too small: file_offsets holds
 * the sizes and csg_copy_files fetches the bytes, as after csg_render_batch
 * (depth_stats is written in that case too). */
typedef struct {
  uint32_t width, height, n_frames, file_kinds;  /* file_kinds: CSG_FILE_* (0: depth_stats only) */
  const uint8_t* rgb;        /* [n][H][W][3], any alignment: RGB_PNG, POINTCLOUD_TXT, POINTCLOUD_PLY */
  const uint8_t* depth_vis;  /* [n][H][W][3], any alignment: DEPTH_PNG */
  const float* depth;        /* [n][H][W]: DEPTH_CSV, DEPTH16_PNG, depth_stats */
  const float* points;       /* [n][H][W][3]: POINTCLOUD_TXT, POINTCLOUD_PLY */
  float depth16_counts_per_metre;  /* as csg_outputs' */
  uint8_t* files;            /* host, files_cap bytes */
  uint64_t files_cap;
  uint64_t* file_offsets;    /* host, n_frames * n_kinds + 1 */
  double* depth_stats;       /* host [n][6] as csg_outputs.depth_stats, or NULL */
} csg_encode_job;
int csg_encode_files(csg_ctx* ctx, const csg_encode_job* job);

/* Page-locked host memory for csg_outputs.files and the other host outputs. */
int csg_host_alloc(csg_ctx* ctx, uint64_t bytes, void** out);
int csg_host_free(csg_ctx* ctx, void* p);

/* Work-buffer sizing.  k_setup appends each frame's raster records into the
 * frame's region of a record pool and k_bin its tile lists into a region of a
 * bin pool; the pools hold one launch chain (frames_per_launch frames), whose
 * frames get back-to-back regions (a planning kernel at the head of the
 * chain).  A frame's region is its csg_frame hints, or with hints 0 the
 * per-frame caps.  With the config's caps 0 and no sizing those are sized for
 * every triangle of the scene (1.125 x triangles per frame, 3x that in bin
 * entries), which no frame can overflow but which a typical view uses a
 * fraction of (C3 1080p: ~1/5 of the records, ~1/9 of the bin entries).
 *
 * csg_size_work runs the sizing pass on `n_frames` frames (host records, or
 * device records when frames_on_device = 1; any number, in chains of 64):
 * k_clip, k_setup, k_count, k_colscan and k_scan only, no raster and no
 * outputs.  It then
 *   - writes each frame's hints: its measured record and bin-entry counts
 *     times (1 + margin) (margin >= 0, e.g. 0.25) plus a small pad, into
 *     the frame records passed (device or host memory);
 *   - sets the per-frame caps (frames without hints) to the largest counts
 *     measured, with the same margin;
 *   - sizes the pools for the heaviest run of frames_per_launch consecutive
 *     frames of the order given (fewer frames than that: all of them plus
 *     the rest at the per-frame caps),
 * and frees the work buffers (the next batch allocates them).  The counts are
 * a pure function of the frame and the scene, so batches that render the
 * measured frames, in that order, with their hints, never overflow.  Other
 * batches can: csg_render_batch then renders again -- with the pools grown to
 * the largest launch chain's hinted total when the frames were grouped
 * differently, else without hints (every frame at the per-frame caps), then
 * with grown caps -- and prints a "[csg]" line on stderr for each such retry;
 * an asynchronous batch reports CSG_ERR_OVERFLOW at the next csg_synchronize.  Waits for the context's
 * earlier batches first (and reports their errors). */
typedef struct {
  uint32_t records_per_frame;  /* current per-frame caps (frames without hints) */
  uint32_t bins_per_frame;
  uint32_t frames_per_launch;  /* frames the work buffers hold (one launch chain) */
  uint32_t sized_frames;       /* frames the last csg_size_work measured (0: none) */
  uint32_t max_records;        /* largest per-frame counts it measured */
  uint32_t max_bins;
  double mean_records;         /* and their means */
  double mean_bins;
  uint64_t work_bytes;         /* device bytes of the work buffers at the current pools */
  uint64_t pool_records;       /* pool entries of one launch chain */
  uint64_t pool_bins;
  uint32_t hinted;             /* 1: pools sized from frame hints (csg_size_work) */
  uint32_t hint_retries;       /* re-renders the hinted pools caused (grown pools or hints turned off) */
} csg_work_info;
int csg_size_work(csg_ctx* ctx, csg_frame* frames, uint32_t n_frames, int32_t frames_on_device,
                  float margin, csg_work_info* out);
int csg_get_work_info(csg_ctx* ctx, csg_work_info* out);

/* Bytes per instance id on the host wire of host-output batches: 1 when every
 * instance label is in [-1, 254], 2 up to 65,534, else 4 (int32 as rendered).
 * The ids cross PCIe as (id + 1) in that width and are widened into the
 * caller's int32 array on host threads (the reference's int32 mask,
 * generate_construction_data.py:1909-1910, :2066-2069) before the batch's
 * stream completes; CSG_NARROW_IDS=0 at csg_create keeps int32 on the wire.
 * Returns the width (1, 2 or 4), or a negative status. */
int csg_host_id_bytes(const csg_ctx* ctx);

/* Object crops (zoom-in patches): for each frame, up to per_frame square
 * windows resampled to size x size pixels from arrays a render wrote (or any
 * arrays of the same layout); a stand-alone pass that needs no scene and no
 * earlier render, on device memory only.  The frame size is the context's.
 *
 * All float arithmetic below is float32, each operation rounded once in the
 * written order.
 *
 * Plan (explicit_boxes = 0), per frame: label l is a candidate iff eligible[l]
 * != 0 (or eligible is NULL) and inst_stats[l][0] >= min_pixels.  Candidates
 * are ordered by pixels descending, ties to the lower label; the first
 * per_frame fill slots 0.. in that order, the other slots are empty (label -1,
 * every other field 0).  A filled slot's window comes from the label's inclusive
 * box minx, miny, maxx, maxy (unsigned 32-bit arithmetic): w = maxx - minx + 1,
 * h = maxy - miny + 1, cx = (float)(minx + maxx + 1) * 0.5f, cy likewise, side =
 * pad * (float)max(w, h), x0 = cx - side * 0.5f, y0 = cy - side * 0.5f.
 *
 * Explicit boxes (explicit_boxes = 1): `info` is read and never written; slot
 * [f][k] samples frame f (its `frame` and `pixels` fields are ignored).  A slot
 * is live iff 0 <= label < n_labels, side is finite with 0 < side <= 32768, and
 * |x0|, |y0| are finite and <= 2^20; any other slot behaves as an empty one.
 *
 * Sample, for a live slot with label L, output column i, row j (S = size):
 * step = side / (float)S, sx = x0 + ((float)i + 0.5f) * step, sy likewise.
 * Nearest pixel px = floor(sx), py = floor(sy), `inside` iff it lies in the
 * frame.  mask = 255 iff inside and instance[py][px] == L, else 0; coords =
 * obj_coords[py][px] where the mask is set, else (0, 0, 0); depth =
 * depth[py][px] where the mask is set, else +inf.  RGB is bilinear and not
 * masked: tx = sx - 0.5f, xl = floorf(tx), wx = (int)((tx - xl) * 256.0f), and
 * ty, yl, wy likewise; taps (xl, yl) .. (xl + 1, yl + 1), a tap outside the
 * frame reads (0, 0, 0); per channel top = a * (256 - wx) + b * wx, bot
 * likewise, value = (top * (256 - wy) + bot * wy + 32768) >> 16.  Empty slots
 * write zeros to every requested image, +inf to the depth.  So a window with
 * integer x0, y0 and side == S copies the source window exactly; windows with
 * step > 1 alias (no area filter): csg_crop_objects_filtered with
 * CSG_CROP_FILTER_AREA, below, filters their RGB.
 *
 * No source value can make a kernel read or write outside the arrays described:
 * every tap is checked against the frame and every label against n_labels. */
typedef struct {            /* 32 bytes */
  int32_t  label;           /* inst_idx of the slot's object; -1 = empty slot */
  uint32_t pixels;          /* its visible pixels (inst_stats[.][label][0]); 0 in explicit mode */
  float    x0, y0, side;    /* the square source window, in source pixels */
  uint32_t frame;           /* index of the frame in the batch */
  uint32_t reserved[2];     /* 0 */
} csg_crop_info;

typedef struct {
  uint32_t size;            /* S: crop side, multiple of 4, 16..512 */
  uint32_t per_frame;       /* K: slots per frame, 1..64 */
  uint32_t min_pixels;      /* >= 1: a label needs this many visible pixels */
  float    pad;             /* window side = pad * max(w, h) of the visible 2D box; finite, >= 1 */
  int32_t  explicit_boxes;  /* 0: plan from inst_stats; 1: `info` is an input */
  uint32_t n_labels;
  /* sources, device memory, [n][H][W]...: the arrays a render wrote */
  const uint8_t*  rgb;         /* needed iff crop_rgb */
  const int32_t*  instance;    /* always */
  const uint16_t* obj_coords;  /* iff crop_coords */
  const float*    depth;       /* iff crop_depth */
  const uint32_t* inst_stats;  /* [n][n_labels][5], iff explicit_boxes == 0 */
  const uint8_t*  eligible;    /* [n_labels], non-zero = may be cropped; NULL = all */
  /* outputs, device memory; any of the four images may be NULL */
  uint8_t*  crop_rgb;          /* [n][K][S][S][3], 4-B aligned */
  uint8_t*  crop_mask;         /* [n][K][S][S], 255 / 0, 4-B aligned */
  uint16_t* crop_coords;       /* [n][K][S][S][3], 8-B aligned */
  float*    crop_depth;        /* [n][K][S][S], 16-B aligned */
  csg_crop_info* info;         /* [n][K], 4-B aligned; output, or input when explicit_boxes = 1 */
} csg_crop_job;

/* Enqueues on `stream` (a hipStream_t, NULL = the context's stream) and
 * returns; on the stream of the render that wrote the sources it needs no
 * synchronisation in between.  csg_synchronize waits for it when the stream is
 * the context's or that of the context's last batch; otherwise the caller
 * synchronises its stream.  CSG_ERR_INVALID for size, per_frame, min_pixels or
 * pad out of range, a missing source of a requested output, a misaligned
 * output, info NULL or n_frames == 0. */
int csg_crop_objects(csg_ctx* ctx, const csg_crop_job* job, uint32_t n_frames, void* stream);

/* csg_crop_objects with a choice of RGB filter.  CSG_CROP_FILTER_BILINEAR is
 * csg_crop_objects itself, byte for byte; CSG_CROP_FILTER_AREA replaces the RGB
 * of minified windows by an exact box filter (what a CPU pipeline's area
 * resampling does), so that a crop pixel averages every source pixel it stands
 * for.  Mask, coordinates and depth are the same under either filter (labels
 * are not blended), and so is `info`.
 *
 * The area filter applies to the RGB of a live slot with step = side /
 * (float)S > 1.0f (a float32 comparison) whose window also has side <= 32768
 * and |x0|, |y0| <= 2^20 -- every live slot of explicit boxes does; a planned
 * window beyond those bounds keeps its bilinear RGB.  Any other slot's RGB is
 * the bilinear RGB above, bit for bit.  It is exact integer arithmetic on
 * float32 edges, so the result does not depend on the order of summation:
 *
 * Edges (float32, each operation rounded once): ex_i = x0 + (float)i * step for
 * i = 0..S, EX_i = (int32)floorf(ex_i * 256.0f); ey_j, EY_j likewise from y0.
 * Crop pixel (i, j) stands for the source rectangle [EX_i, EX_{i+1}) x [EY_j,
 * EY_{j+1}) in 1/256 of a source pixel: neighbours share an edge, so the
 * footprints tile the window.  |E| < 2^29; DX = EX_{i+1} - EX_i and DY lie in
 * [1, 2^19 + 64] (step <= 2048, an edge rounded by at most 1/16 pixel).
 *
 * Weights: source column p is [256 p, 256 (p + 1)) and has weight wx_i(p) =
 * max(0, min(EX_{i+1}, 256 (p + 1)) - max(EX_i, 256 p)), an integer in 0..256;
 * the weights of a footprint sum to DX.  wy_j(r) likewise for source row r.
 *
 * Value, per channel: acc = sum_r wy_j(r) * (sum_p wx_i(p) * c[r][p]) over the
 * pixels of the footprint, where a pixel outside the frame contributes 0 and
 * still counts in the denominator (as a bilinear tap outside the frame reads
 * (0, 0, 0)); value = (acc + (D >> 1)) / D with D = DX * DY in unsigned 64-bit
 * integers.  A row sum is below 2^27, acc below 2^47, the quotient at most
 * 255.  A pixel with DX <= 0 or DY <= 0 (which no window within the bounds
 * above produces) is (0, 0, 0).
 *
 * So an image that is constant over a footprint gives that constant; a window
 * with integer x0, y0 and step == 2 gives (a + b + c + d + 2) >> 2 of each 2x2
 * block; and towards step == 1 the box narrows to one source pixel, whose
 * weights are the bilinear ones, so the two filters meet without a seam.
 *
 * Arguments are checked as csg_crop_objects checks them; any other rgb_filter
 * is CSG_ERR_INVALID (nothing is enqueued or written).  CSG_CROP_FILTER_AREA
 * with crop_rgb == NULL is valid and changes nothing.  The guarantee above
 * holds: no window and no source value yields an address outside the arrays. */
#define CSG_CROP_FILTER_BILINEAR 0u   /* csg_crop_objects' RGB, unchanged */
#define CSG_CROP_FILTER_AREA     1u   /* exact box filter where step > 1 */
int csg_crop_objects_filtered(csg_ctx* ctx, const csg_crop_job* job, uint32_t rgb_filter,
                              uint32_t n_frames, void* stream);

/* Amodal crop masks: for each slot of `info`, the samples of its window that the
 * slot's object covers when every other object is taken out of the scene --
 * BOP's `mask`, where crop_mask is `mask_visib`.  Unlike the crops this pass
 * reads the uploaded scene (geometry, the frames' transform sets and their
 * materials) and no rendered array; it is the per-pixel form of label_covered
 * (occlusionRatio), without that counter's limit of 32 labels per tile.
 *
 * Live slot: a slot is live under the rule csg_crop_objects applies to an
 * `info` it reads: 0 <= label < the scene's label-table length (largest inst_idx
 * + 1), side finite with 0 < side <= 32768, |x0|, |y0| finite and <= 2^20.
 * Every other slot -- an empty one, a planned window beyond those bounds --
 * writes zeros.  Slot [f][k] belongs to frames[f].
 *
 * Sample (i, j) of a live slot with label L has the px, py and `inside` of
 * csg_crop_objects (the same float32 expressions).  crop_amodal = 255 iff the
 * sample is inside and some instance with inst_idx == L has a triangle that, at
 * pixel (px, py) of frame f, passes all of:
 *   - one of its raster sub-triangles (after the near clip; fixed point, exact
 *     edge functions, top-left rule) covers the pixel centre under the models
 *     of transform set frames[f].xform_set and the frame's view and proj;
 *   - its 1/W at the centre lies in [1/far_clip, 1/near_clip];
 *   - the alpha test with the material that set gives the instance (texture
 *     swaps of csg_set_dr_textures applied).
 * There is no depth test and no per-tile label cap: the pixel is one that is not
 * -1 in a render of the frame from which every instance of another label is
 * removed.  A set inside the range that was never uploaded has zero models and
 * draws nothing, so its slots are all zero; so are those of a label no
 * instance carries.
 *
 * So: wherever crop_mask of the same slot is 255, crop_amodal is 255; every
 * byte of crop_amodal is written; and no `info` value -- NaN, infinite, far
 * away, any label -- yields an address outside the arrays described.
 *
 * Enqueues on `stream` (NULL = the context's stream) and returns; `frames` are
 * copied before it returns.  Behind csg_crop_objects on the same stream it needs
 * no synchronisation.  csg_synchronize waits for it under the rule for the
 * crops.  The pass has scratch of its own, grown to the job (n_frames is not
 * bound by max_frames), and never touches the render's work buffers: a render on
 * another stream may run beside it.  Pending scene changes (transforms,
 * textures) are uploaded first, as by a render.
 *
 * CSG_ERR_INVALID, nothing enqueued or written: job, frames, info or crop_amodal
 * NULL; n_frames == 0; size or per_frame out of range; crop_amodal or info
 * misaligned; no scene uploaded; a frames[f].xform_set that is not resident
 * (>= the largest set id uploaded + 1). */
typedef struct {
  uint32_t size;               /* S, as csg_crop_job: multiple of 4, 16..512 */
  uint32_t per_frame;          /* K, 1..64 */
  const csg_frame* frames;     /* HOST records [n]: view, proj, xform_set of the frames the crops were cut
                                  from; copied before the call returns (the caller may reuse them at once) */
  const csg_crop_info* info;   /* DEVICE [n][K], read only: what csg_crop_objects wrote or read; slot [f][k]
                                  belongs to frames[f] (its `frame` and `pixels` fields are ignored) */
  uint8_t* crop_amodal;        /* DEVICE [n][K][S][S], 255 / 0, 4-B aligned */
} csg_amodal_job;
int csg_crop_amodal(csg_ctx* ctx, const csg_amodal_job* job, uint32_t n_frames, void* stream);

/* Amodal depth and object coordinates of the crops: the geometry that belongs
 * to the amodal mask, made by the same pass.  For sample (i, j) of a live slot
 * with label L (px, py and `inside` as above) let H be the set of fragments
 * csg_crop_amodal counts at pixel (px, py): triangles of instances with
 * inst_idx == L, covered, 1/W in [1/far_clip, 1/near_clip], alpha passed under the
 * frame's transform set; no depth test against other objects.
 *   crop_amodal         255 iff the sample is inside and H is not empty: byte for
 *                       byte what csg_crop_amodal writes.
 *   crop_amodal_depth   1 / w*, w* = the largest 1/W over H (compared as float32
 *                       bits: all are positive, so the bit order is the value
 *                       order), by the resolve's correctly rounded reciprocal;
 *                       +inf where H is empty.  It is the depth of a render of
 *                       the frame with every instance of another label removed,
 *                       and depends only on the maximum, not on the triangle that
 *                       supplied it.
 *   crop_amodal_coords  the object coordinates (csg_outputs.obj_coords) of pixel
 *                       (px, py) with that depth and label L: the frame's camera
 *                       constants and the object-frame table of its transform
 *                       set (csg_set_object_frames); (0, 0, 0) where H is empty
 *                       and for a set without a table.
 * Dead slots write 0, +inf and (0, 0, 0); every byte of every requested output
 * is written; no `info` value yields an address outside the arrays.  So wherever
 * crop_mask of the same slot is 255, crop_amodal_depth and crop_amodal_coords
 * equal crop_depth and crop_coords bit for bit, and at an inside sample where
 * only crop_amodal is 255 the amodal depth is >= the frame's depth at (px, py).
 *
 * At least one output is non-NULL.  Argument rules, slot liveness, stream and
 * ownership semantics are csg_crop_amodal's (messages start with
 * "crop_amodal_geometry:"); pending scene changes and, when coordinates are
 * asked for, the object-frame table are brought up to date first, as by a render.
 * Scratch: 4 bytes per sample while the pass runs.  crop_amodal_depth, when
 * given, holds them itself; otherwise the pass has a bounded buffer of its own
 * and runs the job as frame ranges on the stream. */
typedef struct {
  uint32_t size, per_frame;          /* as csg_amodal_job */
  const csg_frame* frames;           /* HOST [n], copied before the call returns */
  const csg_crop_info* info;         /* DEVICE [n][K], read only */
  uint8_t* crop_amodal;              /* DEVICE [n][K][S][S] 255 / 0, 4-B aligned, or NULL */
  float* crop_amodal_depth;          /* DEVICE [n][K][S][S], 16-B aligned, or NULL */
  uint16_t* crop_amodal_coords;      /* DEVICE [n][K][S][S][3], 8-B aligned, or NULL */
} csg_amodal_geometry_job;
int csg_crop_amodal_geometry(csg_ctx* ctx, const csg_amodal_geometry_job* job, uint32_t n_frames, void* stream);

/* Per-object run-length masks: the vertical runs of every label of an instance
 * image, in the column-major order of COCO's run-length masks, so that a
 * frame's per-object masks leave the GPU as a few thousand 8-byte records
 * instead of a dense image.  A stand-alone pass on device memory only, like
 * the crops: it needs no scene and no earlier render, and the frame size is the
 * job's own (as in csg_encode_files), not the context's.  Integers only.
 *
 * Definition.  `instance` is [n][H][W] int32, L = n_labels.  A pixel belongs to
 * label l iff its id equals l and 0 <= l < L; every other value (-1, any other
 * negative, >= L) belongs to no label.  A span of label l in frame f is a
 * maximal run of vertically adjacent pixels of l within one column x, rows
 * y0 .. y0 + len - 1; spans never cross a column boundary.  It is stored as a
 * csg_span: start = x * H + y0 (COCO's column-major pixel index) and len.
 *
 *   spans         [n][C] csg_span, C = capacity.  Frame f uses spans[f * C ..],
 *                 ordered by label ascending, then start ascending.
 *   span_offsets  [n][L + 1] uint32.  Label l's spans of frame f are records
 *                 [off[f][l], off[f][l + 1]) of the frame; off[f][0] = 0 and
 *                 off[f][L] is the frame's total WHETHER OR NOT IT FITS.
 *
 * Overflow.  When a frame's total exceeds C, that frame's records are
 * unspecified within its C slots (its offsets are still exact); nothing is
 * written outside them and the other frames are unaffected.  The call is
 * asynchronous and cannot return the overflow: the caller reads off[f][L] > C
 * after its stream completes and repeats the pass with a larger C.  A frame has
 * at most W * ((H + 1) / 2) spans.
 *
 * The result is a pure function of the input (the order is total; nothing in
 * it depends on scheduling), every record below a fitting frame's total and
 * every offset is written, and nothing else: records from a frame's total up to
 * C keep what they held.  No input value makes a kernel read or write outside
 * the arrays described.
 *
 * Enqueues on `stream` (NULL = the context's stream) and returns; behind the
 * render that wrote `instance` on the same stream it needs no synchronisation.
 * csg_synchronize waits for it under the rule for the crops.  The pass has
 * scratch of its own (4 bytes per frame, label and 64 columns), grown to the
 * job, and never touches the render's work buffers.
 *
 * CSG_ERR_INVALID, nothing enqueued or written: job, instance, spans or
 * span_offsets NULL; n_frames == 0; width or height 0 or above 8192;
 * capacity == 0; n_labels == 0; spans not 8-byte or span_offsets not 4-byte
 * aligned.  CSG_ERR_LIMIT: n_labels above CSG_SPAN_MAX_LABELS (a wave keeps a
 * 256-byte row per label in LDS; the one-byte id wire of csg_host_id_bytes
 * marks the same practical range). */
#define CSG_SPAN_MAX_LABELS 256u
typedef struct {            /* 8 bytes */
  uint32_t start;           /* x * height + y0 */
  uint32_t len;             /* rows, >= 1 */
} csg_span;

typedef struct {
  uint32_t width, height;      /* of the frames in `instance`: 1..8192 each */
  uint32_t n_labels;           /* L: 1..CSG_SPAN_MAX_LABELS */
  uint32_t capacity;           /* C: span records per frame, >= 1 */
  const int32_t* instance;     /* DEVICE [n][H][W] */
  csg_span* spans;             /* DEVICE [n][C], 8-B aligned */
  uint32_t* span_offsets;      /* DEVICE [n][L + 1], 4-B aligned */
} csg_span_job;
int csg_mask_spans(csg_ctx* ctx, const csg_span_job* job, uint32_t n_frames, void* stream);

/* The ids of a host-output batch for csg_mask_spans, without their trip to the
 * host.  A host-output batch (csg_outputs.on_device = 0) renders the instance
 * ids only when csg_outputs.instance asks for them, and then copies them.
 * After csg_keep_instance(ctx, 1) every later host-output batch renders them
 * into the context's own device image even when csg_outputs.instance is NULL,
 * and copies nothing more than it did; 0 turns that off again.
 * csg_last_instance returns the device image [n_frames][height][width] int32 of
 * the context's last batch and its frame count (NULL and 0 when that batch
 * rendered no ids, or wrote them to the caller's device memory); it stays
 * valid until the context's next batch.  Neither call touches the GPU. */
int csg_keep_instance(csg_ctx* ctx, int32_t keep);
int csg_last_instance(csg_ctx* ctx, const int32_t** instance, uint32_t* n_frames);

/* Full-frame amodal object masks as run-length spans: for every label its
 * silhouette over the whole frame as if nothing stood in front of it (BOP's
 * `mask` next to `mask_visib`), in the layout of csg_mask_spans, with the amodal
 * box (`bbox_obj`) and pixel count (`px_count_all`), from one pass over the
 * scene.  L is the uploaded scene's label-table length (largest instance label
 * + 1, at least 1); W and H are the context's frame size.
 *
 * Definition.  Pixel (x, y) of frame f belongs to the amodal mask of label l iff
 * eligible[l] holds (NULL = every label) and the pixel satisfies
 * csg_crop_amodal's condition at (px, py) = (x, y): some instance with
 * inst_idx == l has a triangle one of whose raster sub-triangles covers the
 * pixel centre under the frame's transform set (spec 3.1-3.4), with its 1/W in
 * [1/far, 1/near] (3.5) and passing the alpha test with the material that set
 * gives the instance (3.6, texture swaps applied).  There is no depth test and
 * no per-tile label cap: equivalently, the pixel is not -1 in a render of the
 * frame with every instance of another label removed.  So every pixel whose
 * rendered id is l lies in l's mask, and masks of different labels may overlap.
 *
 *   spans, span_offsets  the spans of that per-label mask under exactly
 *                 csg_mask_spans' rules: vertical runs, start = x * H + y0,
 *                 ordered by label and then by start; off[f][0] = 0 and
 *                 off[f][L] is the frame's total WHETHER OR NOT IT FITS C.  An
 *                 overflowing frame has unspecified records inside its own C
 *                 slots and exact offsets; nothing outside its slots is written
 *                 and other frames are unaffected.  Records from a fitting
 *                 frame's total up to C keep what they held.
 *   amodal_stats  [n][L][5] uint32 = pixels, minx, miny, maxx, maxy of the mask
 *                 (inclusive box, inside the frame by construction); a label
 *                 without pixels gets inst_stats' empty value (0, 0xFFFFFFFF,
 *                 0xFFFFFFFF, 0, 0).  Every entry is written.  May be NULL.
 *
 * A transform set inside the resident range that was never uploaded draws
 * nothing.  The result is a pure function of the input.
 *
 * Asynchronous on `stream`; the stream, ownership and csg_synchronize rules are
 * csg_crop_amodal's: `frames` and `eligible` are copied before the call
 * returns, pending scene changes are uploaded first as by a render, and the
 * completion event shared with the other amodal passes orders the pass against
 * scene uploads, reallocation and passes on other streams.  Scratch is the
 * pass's own, never the render's work buffers: one bit per pixel, eligible label
 * and frame of a range (rows packed 32 to a word), bounded at 64 MiB -- a job
 * that needs more runs as frame ranges on the stream, each range zeroing,
 * filling and reading the same scratch (at least one frame per range).
 * CSG_AMODAL_PLANE_CAP (bytes) overrides the bound.
 *
 * CSG_ERR_INVALID, nothing enqueued or written: job, frames, spans or
 * span_offsets NULL; n_frames == 0; capacity == 0; spans not 8-byte or
 * span_offsets / amodal_stats not 4-byte aligned; no scene uploaded; a frame's
 * xform_set not resident.  CSG_ERR_LIMIT: L above CSG_SPAN_MAX_LABELS. */
typedef struct {
  uint32_t capacity;          /* C: span records per frame, >= 1 */
  const csg_frame* frames;    /* HOST [n]: view, proj, xform_set; copied before the call returns */
  const uint8_t* eligible;    /* HOST [L] or NULL (= all): labels with 0 get no spans and empty stats; copied */
  csg_span* spans;            /* DEVICE [n][C], 8-B aligned */
  uint32_t* span_offsets;     /* DEVICE [n][L + 1], 4-B aligned */
  uint32_t* amodal_stats;     /* DEVICE [n][L][5] = pixels, minx, miny, maxx, maxy, 4-B aligned, or NULL */
} csg_amodal_span_job;
int csg_amodal_spans(csg_ctx* ctx, const csg_amodal_span_job* job, uint32_t n_frames, void* stream);

/* Per-object mask PNGs from spans: each (frame, label) item's mask, the union of
 * that label's span records of that frame, as a finished 8-bit grey PNG file
 * (0 / 255), all files packed into `out` -- what BOP's `mask_visib` and `mask`
 * folders hold, one file per object per frame, without the dense ids crossing
 * PCIe and without a zlib call per object on the host.  A stand-alone pass on
 * device memory only, like csg_mask_spans: it needs no scene and no earlier
 * render, and the frame size is the job's own.  Integers only.
 *
 *   spans, span_offsets  exactly what csg_mask_spans or csg_amodal_spans wrote for
 *                 `n_frames` frames of `width` x `height` with L = n_labels and
 *                 C = capacity; read only.
 *   items         HOST [n_items] csg_mask_item {frame, label}, copied before the
 *                 call returns.  The same label may appear in several items; a
 *                 label without spans gives an all-zero mask, a valid file.
 *   out           file i starts at out + file_offsets[i].
 *   file_offsets  [n_items + 1] uint64; file_offsets[0] = 0 and
 *                 file_offsets[n_items] is the exact total WHETHER OR NOT IT FITS.
 *
 * Records.  A record is used whole or not at all: it is ignored if len == 0,
 * start >= W * H, or (start mod H) + len > H.  A frame whose off[f][L] > C
 * (csg_mask_spans' overflow) may hold anything in its records and offsets: no
 * value makes a kernel read or write outside the arrays described, and the files
 * of that frame's items are then unspecified but well inside their ranges.
 *
 * Overflow.  When the total exceeds out_capacity, `out` is unspecified inside
 * out_capacity, nothing is written beyond it and the offsets are still exact:
 * the caller reads file_offsets[n_items] after its stream completes and repeats
 * the pass with an output of that size.
 *
 * The file, byte for byte (one deterministic encoding; csrc/csg_mask_png.h, and
 * writers.mask_png_bytes in Python): PNG signature; IHDR with W, H, bit depth 8,
 * colour type 0, compression, filter and interlace 0; IDAT chunks of 2048 zlib
 * bytes, the last one shorter; IEND.  The zlib stream is 78 01, ONE deflate block
 * with BFINAL = 1 and BTYPE = 01 (fixed Huffman), byte padding, and the Adler-32
 * big-endian.  The raw stream is per row the filter byte 0 and W bytes 0 / 255.
 * Each row is tokenised on its own: its 1 + W bytes split into maximal runs of
 * equal bytes (the filter byte joins a leading run of zeros) and each run is one
 * literal, distance-1 matches of at most 258 bytes and a remainder below 3 bytes
 * as literals; one end-of-block code follows the last row.
 *
 * Asynchronous on `stream` (NULL = the context's stream); behind the span pass
 * on the same stream it needs no synchronisation.  The result is a pure function
 * of the input.  Scratch is the pass's own, under an order of its own: one bit
 * per pixel and item (bounded at 64 MiB: a job that needs more runs as ranges of
 * items on the stream; CSG_MASK_PNG_PLANE_CAP, bytes, overrides the bound), 12
 * bytes per row and item, and a staging area for the zlib streams of at most
 * out_capacity + 4 bytes per item.
 *
 * CSG_ERR_INVALID, nothing enqueued or written: job, spans, span_offsets, items,
 * out or file_offsets NULL; n_frames, n_items or capacity 0; width or height 0
 * or above 8192; n_labels 0; an item with frame >= n_frames or label >=
 * n_labels; spans or file_offsets not 8-byte or span_offsets not 4-byte aligned.
 * CSG_ERR_LIMIT: n_labels above CSG_SPAN_MAX_LABELS. */
typedef struct {            /* 8 bytes */
  uint32_t frame;           /* < n_frames */
  uint32_t label;           /* < n_labels */
} csg_mask_item;

typedef struct {
  uint32_t width, height;      /* of the frames the spans describe: 1..8192 each */
  uint32_t n_frames;
  uint32_t n_labels;           /* L: 1..CSG_SPAN_MAX_LABELS */
  uint32_t capacity;           /* C: span records per frame, >= 1 */
  uint32_t n_items;            /* >= 1 */
  const csg_span* spans;       /* DEVICE [n_frames][C], 8-B aligned */
  const uint32_t* span_offsets;/* DEVICE [n_frames][L + 1], 4-B aligned */
  const csg_mask_item* items;  /* HOST [n_items], copied before the call returns */
  uint8_t* out;                /* DEVICE [out_capacity] */
  uint64_t out_capacity;
  uint64_t* file_offsets;      /* DEVICE [n_items + 1], 8-B aligned */
} csg_mask_png_job;
int csg_encode_span_masks(csg_ctx* ctx, const csg_mask_png_job* job, void* stream);

/* Baseline JPEG files of RGB frames, made on the GPU.  A stand-alone pass on
 * device memory only, like csg_encode_span_masks: it needs no scene and no
 * earlier render, and the frame size is the job's own.  Frame f becomes one
 * .jpg file; the files are packed back to back in `out`: file f occupies
 * out[file_offsets[f] .. file_offsets[f + 1]), file_offsets[0] = 0, and
 * file_offsets[n_frames] is the exact total whether or not it fits.  Nothing is
 * written beyond out_capacity, and a file that does not fit whole is not written
 * at all: the caller reads file_offsets[n_frames] after its stream completes and
 * repeats the pass with an output of that size.
 *
 * The file, byte for byte (one deterministic encoding; csrc/csg_jpeg.h, and
 * writers.jpeg_bytes in Python): SOI; APP0 (JFIF 1.01, density 1:1, no
 * thumbnail); two DQT (Annex K's tables at libjpeg's quality scaling, zig-zag
 * order); SOF0 with the true W and H and components Y, Cb, Cr (ids 1, 2, 3) at
 * 4:4:4 or 4:2:0; four DHT (Annex K.3's typical tables: DC0, AC0, DC1, AC1); DRI
 * with the MCUs of one MCU row; SOS; one interleaved scan in which every MCU row
 * is a restart interval, padded with 1-bits and followed by RSTm (m counting mod
 * 8) except the last; EOI.  A zero byte follows every 0xFF byte of entropy data.
 * Colour is JFIF's full-range BT.601 in 16-bit fixed point, the image extends to
 * whole MCUs by repeating its last column and row, 4:2:0 chroma is the rounded
 * mean of 2 x 2 samples, the DCT is an integer one within 0.2 of the exact
 * transform, and the quantiser rounds half away from zero.  A 4:2:0 luminance
 * block that holds no pixel of the image repeats the DC of the block before it
 * in its MCU and has no AC.
 *
 * Asynchronous on `stream` (NULL = the context's stream); behind the kernel that
 * wrote `rgb` on the same stream it needs no synchronisation.  The result is a
 * pure function of the input.  Scratch is the pass's own, under an order of its
 * own: per 8 x 8 block 128 bytes of coefficients, 4 bytes of bit counts and a
 * 208-byte staging slot, bounded at 256 MiB: a job that needs more runs as
 * ranges of frames on the stream; CSG_JPEG_SCRATCH_CAP, bytes, overrides the
 * bound.
 *
 * CSG_ERR_INVALID, nothing enqueued or written: job, rgb, out or file_offsets
 * NULL; n_frames 0; width or height 0 or above 8192; quality outside 1..100;
 * a subsampling other than CSG_JPEG_444 and CSG_JPEG_420; file_offsets not
 * 8-byte aligned. */
#define CSG_JPEG_444 0u
#define CSG_JPEG_420 1u
typedef struct {
  uint32_t width, height;     /* 1..8192 each */
  uint32_t n_frames;          /* >= 1 */
  uint32_t quality;           /* 1..100 */
  uint32_t subsampling;       /* CSG_JPEG_444 = 0, CSG_JPEG_420 = 1 */
  uint32_t pad;
  const uint8_t* rgb;         /* DEVICE [n_frames][H][W][3], any alignment */
  uint8_t* out;               /* DEVICE [out_capacity] */
  uint64_t out_capacity;
  uint64_t* file_offsets;     /* DEVICE [n_frames + 1], 8-B aligned */
} csg_jpeg_job;
int csg_encode_jpeg(csg_ctx* ctx, const csg_jpeg_job* job, void* stream);

/* The RGB of a host-output batch for csg_encode_jpeg, without its trip to the
 * host: the exact counterparts of csg_keep_instance and csg_last_instance.
 * After csg_keep_rgb(ctx, 1) every later host-output batch renders its RGB into
 * the context's own device image even when csg_outputs.rgb is NULL and no file
 * kind asks for it, and copies nothing more than it did; 0 turns that off again.
 * csg_last_rgb returns the device image [n_frames][height][width][3] uint8 of the
 * context's last batch and its frame count (NULL and 0 when that batch rendered
 * no RGB, or wrote it to the caller's device memory); it stays valid until the
 * context's next batch.  Neither call touches the GPU. */
int csg_keep_rgb(csg_ctx* ctx, int32_t keep);
int csg_last_rgb(csg_ctx* ctx, const uint8_t** rgb, uint32_t* n_frames);

/* Fixed-size per-object point samples: for each slot of `info`, N pixels drawn
 * from the visible mask of the slot's label, as their indices in the image
 * (what the public loaders of DenseFusion, PVN3D or FFB6D call `choose`), their
 * points in the camera's frame, their colours and their object coordinates --
 * some 30 bytes per sample instead of the dense arrays.  A stand-alone pass on
 * device memory only, like csg_mask_spans: it needs no scene and no earlier
 * render, and the frame size is the job's own.  L = n_labels, K = per_frame,
 * N = samples, P = H * W.
 *
 * Slot liveness.  Slot [f][k] is live iff 0 <= info[f][k].label < L (the label
 * rule of the crops); its window fields are ignored, and `info` is only read.
 * Two slots may name the same label: each gets the full result.
 *
 * Rank.  Let l be a live slot's label.  The pixels of frame f whose id equals l
 * are ranked 0 .. M - 1 in row-major order p = y * W + x, the order of
 * numpy.flatnonzero(instance[f] == l).  pt_count[f][k] = M.
 *
 * Which rank sample s = 0 .. N - 1 takes:
 *   M == 0, or the slot is not live: the slot is empty -- pt_count 0, pt_choose
 *     0xFFFFFFFF, pt_xyz NaN (bits 0x7FC00000), pt_rgb 0, pt_coords 0.
 *   1 <= M <= N: rank s mod M.  Every pixel is used, then they repeat in order
 *     (numpy.pad(..., 'wrap')).
 *   M > N: stratified, one sample per stratum, in unsigned 64-bit integers:
 *     lo_s = (s * M) / N, w_s = lo_{s+1} - lo_s (>= 1),
 *     r_s = lo_s + (uint32)(((uint64)h_s * w_s) >> 32), with
 *     fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35;
 *                x ^= x >> 16 (uint32),
 *     key_f = frame_keys[f], or f when frame_keys is NULL,
 *     base = fmix32(fmix32(seed ^ key_f) ^ (uint32)l),
 *     h_s = fmix32(base ^ (s * 0x9E3779B9u)).
 *     The samples are therefore in ascending pixel order (the CPU loaders' random
 *     choice is unordered; point-set networks do not depend on the order).
 *
 * Values of a sample at pixel (px, py), p = py * W + px:
 *   pt_choose  p.
 *   pt_rgb, pt_coords  rgb[f][py][px] and obj_coords[f][py][px], bit for bit.
 *   pt_xyz     with d = depth[f][py][px] and fx, fy, cx, cy = intrinsics[f], the
 *              point in the OpenCV camera frame (x right, y down, z forward):
 *                X = ((((float)px + 0.5f) - cx) * d) / fx
 *                Y = ((((float)py + 0.5f) - cy) * d) / fy
 *                Z = d
 *              float32, each operation rounded once in the written order ('/' is
 *              the correctly rounded division): the camera point of csg_outputs
 *              .points before its rotation to the world, with y and z not negated.
 *              No value of depth or intrinsics is rejected; infinities and NaN
 *              propagate.  An X or Y that is NaN is stored as 0x7FC00000 (the
 *              sign and payload of a NaN an operation makes are the machine's);
 *              Z is d's bits.
 *
 * The output is a pure function of the inputs: no atomic decides a position,
 * nothing depends on scheduling, and a frame's result depends on its place in
 * the batch only through its key (with frame_keys, the same image under the same
 * key gives the same samples at any position).  Every element of every requested
 * output is written.  No id, label or source value yields an address outside
 * the arrays described: ids index a table only when 0 <= id < L, and lanes past
 * the image load nothing.
 *
 * Enqueues on `stream` (NULL = the context's stream) and returns; behind the
 * render that wrote the sources and the csg_crop_objects that planned `info` on
 * the same stream it needs no synchronisation.  csg_synchronize waits for it
 * under the rule for the crops.  The pass has scratch of its own (4 bytes per
 * frame, label and 4096 pixels, and 4 per frame and label), grown to the job; an
 * event orders passes on different streams; it never touches the render's work
 * buffers.
 *
 * CSG_ERR_INVALID, nothing enqueued or written: job NULL; n_frames == 0; width
 * or height outside 1..8192; n_labels == 0; per_frame outside 1..64; samples not
 * a multiple of 4 in 16..16384; instance or info NULL; pt_xyz without depth or
 * intrinsics, pt_rgb without rgb, pt_coords without obj_coords; no output at
 * all; a pointer that is not aligned to its element (4 bytes for instance, info,
 * depth, intrinsics, frame_keys, pt_count, pt_choose, pt_xyz and pt_rgb; 2 for
 * obj_coords and pt_coords).  CSG_ERR_LIMIT: n_labels above CSG_SPAN_MAX_LABELS. */
typedef struct {
  uint32_t width, height;      /* of the frames: 1..8192 each */
  uint32_t n_labels;           /* L: 1..CSG_SPAN_MAX_LABELS */
  uint32_t per_frame;          /* K: slots per frame, 1..64 */
  uint32_t samples;            /* N: samples per slot, a multiple of 4, 16..16384 */
  uint32_t seed;
  /* sources, device memory */
  const int32_t*  instance;    /* [n][H][W], always */
  const csg_crop_info* info;   /* [n][K], always; read only, only `label` is used */
  const float*    depth;       /* [n][H][W], iff pt_xyz */
  const float*    intrinsics;  /* [n][4] = fx, fy, cx, cy, iff pt_xyz */
  const uint8_t*  rgb;         /* [n][H][W][3], iff pt_rgb */
  const uint16_t* obj_coords;  /* [n][H][W][3], iff pt_coords */
  const uint32_t* frame_keys;  /* [n], or NULL: the key of frame f is f */
  /* outputs, device memory; any may be NULL, not all */
  uint32_t* pt_count;          /* [n][K]: M, the pixels of the slot's label */
  uint32_t* pt_choose;         /* [n][K][N] */
  float*    pt_xyz;            /* [n][K][N][3] */
  uint8_t*  pt_rgb;            /* [n][K][N][3], 4-B aligned */
  uint16_t* pt_coords;         /* [n][K][N][3] */
} csg_point_job;
int csg_sample_object_points(csg_ctx* ctx, const csg_point_job* job, uint32_t n_frames, void* stream);

/* The world-space points of a host-output batch for csg_voxel_cloud, without
 * their trip to the host: the exact counterparts of csg_keep_rgb and
 * csg_last_rgb.  After csg_keep_points(ctx, 1) every later host-output batch
 * renders its points into the context's own device image even when
 * csg_outputs.points is NULL and no file kind asks for them, and copies nothing
 * more than it did; 0 turns that off again.  csg_last_points returns the device
 * image [n_frames][height][width][3] float32 of the context's last batch and its
 * frame count (NULL and 0 when that batch rendered no points, or wrote them to
 * the caller's device memory); it stays valid until the context's next batch.
 * Neither call touches the GPU. */
int csg_keep_points(csg_ctx* ctx, int32_t keep);
int csg_last_points(csg_ctx* ctx, const float** points, uint32_t* n_frames);

/* Voxel-downsampled labelled point clouds: the points of a frame binned on a
 * grid of cubes of side s that is fixed in the world (clouds of different frames
 * line up), one record per occupied (cell, id) pair -- the centroid, the mean
 * colour, the id and the point count -- some 10^4..10^5 records of 23 bytes
 * instead of one point per pixel.  Points of two ids are never merged.  A
 * stand-alone pass on device memory only, like csg_sample_object_points: it
 * needs no scene and no earlier render, and the frame size is the job's own.
 * L = n_labels, C = capacity, s = voxel_size.
 *
 * Points and cells.
 *   A pixel is a point iff its three coordinates are finite and -1 <= id < L
 *   (id = -1 everywhere when `instance` is NULL; n_labels is then ignored).
 *   r = fl32(1.0f / s), computed once on the host.
 *   t_a = fl32(p_a * r) and c_a = floorf(t_a), per axis a.
 *   A point whose t_a is not finite, or whose c_a lies outside [-2^17, 2^17) on
 *   any axis, is dropped.  vx_dropped[f] counts these points.
 *   This range lets 3 x 18 cell bits and the 9 bits of id + 1 fit one 63-bit
 *   key.  All-ones is then free as the empty mark.
 *
 * Accumulation.
 *   frac_a = fl32(t_a - c_a).  This subtraction is exact in float32, and frac_a
 *   lies in [0, 1), except for t_a in (-0.5, 0): there c_a = -1 and t_a + 1 is
 *   rounded (by at most 2^-25), to 1.0 for t_a above -2^-25.
 *   q_a = min((uint32)(frac_a * 65536.0f), 65535), which lies in [0, 65535].
 *   A voxel is the set of kept points of one frame that share (c_x, c_y, c_z, id).
 *   Per voxel: n, the point count; S_a = sum of q_a, which needs 64 bits;
 *   R_k = sum of colour_k (0 when `rgb` is NULL).
 *
 * Record of a voxel.
 *   vx_count = n.  vx_label = id.
 *   vx_rgb_k = (2 * R_k + n) / (2n), in integer arithmetic.
 *   m_a = (2 * S_a + n) / (2n), in integer arithmetic.
 *   vx_xyz_a = fl32(fl32((float)c_a + fl32(((float)m_a + 0.5f) * (1.0f / 65536.0f))) * s).
 *   Every operation rounds once.
 *
 * Order.  Voxels are ordered ascending by the lowest row-major pixel index
 * p = y * W + x among their points.  V is their count.
 *
 * Capacity.
 *   V <= C: vx_total[f] = V.  Rows [0, V) are the records.  Rows [V, C) are
 *   filled with 0x7FC00000 for xyz, 0 for rgb and count, and -1 for label.
 *   V > C: vx_total[f] = 0xFFFFFFFF.  The frame's rows are unspecified, but
 *   nothing is written outside them.  vx_dropped[f] is still exact.
 *   Other frames of the call are unaffected.
 *
 * The result is a pure function of the inputs.  There are no float atomics, and
 * nothing depends on scheduling or on the hash.  No coordinate, id or colour
 * yields an address outside the arrays described.
 *
 * Enqueues on `stream` (NULL = the context's stream) and returns; behind the
 * render that wrote the sources on the same stream it needs no synchronisation.
 * csg_synchronize waits for it under the rule for the crops.  The pass has
 * scratch of its own (per frame a table of T slots of 64 bytes, T the smallest
 * power of two >= 2 * min(C, H * W), and H * W / 4 bytes), grown to the job and
 * bounded at 256 MiB: a job that needs more runs as ranges of frames.  An event
 * orders passes on different streams; it never touches the render's work buffers.
 *
 * CSG_ERR_INVALID, nothing enqueued or written: job NULL; n_frames == 0; width
 * or height outside 1..8192; voxel_size not finite or not > 0; capacity == 0;
 * with `instance`, n_labels == 0 or above CSG_SPAN_MAX_LABELS; points or
 * vx_total NULL; a pointer that is not aligned to its element (4 bytes for
 * points, instance, vx_xyz, vx_label, vx_count, vx_total and vx_dropped). */
typedef struct {
  uint32_t width, height;      /* of the frames: 1..8192 each */
  uint32_t n_labels;           /* L: 1..CSG_SPAN_MAX_LABELS (ignored without `instance`) */
  uint32_t capacity;           /* C >= 1: records per frame */
  float    voxel_size;         /* s: finite, > 0 */
  uint32_t pad;
  /* sources, device memory */
  const float*   points;       /* [n][H][W][3] as csg_outputs.points: world space, NaN where nothing is hit */
  const uint8_t* rgb;          /* [n][H][W][3], or NULL: colours are 0 */
  const int32_t* instance;     /* [n][H][W], or NULL: every id is -1 */
  /* outputs, device memory; any may be NULL except vx_total */
  float*    vx_xyz;            /* [n][C][3] */
  uint8_t*  vx_rgb;            /* [n][C][3] */
  int32_t*  vx_label;          /* [n][C] */
  uint32_t* vx_count;          /* [n][C] */
  uint32_t* vx_total;          /* [n] */
  uint32_t* vx_dropped;        /* [n] */
} csg_voxel_job;
int csg_voxel_cloud(csg_ctx* ctx, const csg_voxel_job* job, uint32_t n_frames, void* stream);

/* The depth image of a host-output batch for csg_sensor_depth, without its trip
 * to the host: the exact counterparts of csg_keep_points and csg_last_points.
 * After csg_keep_depth(ctx, 1) every later host-output batch renders its depth
 * into the context's own device image even when csg_outputs.depth is NULL and
 * nothing else asks for it, and copies nothing more than it did; 0 turns that
 * off again.  csg_last_depth returns the device image [n_frames][height][width]
 * float32 of the context's last batch and its frame count (NULL and 0 when that
 * batch rendered no depth, or wrote it to the caller's device memory); it stays
 * valid until the context's next batch.  Neither call touches the GPU. */
int csg_keep_depth(csg_ctx* ctx, int32_t keep);
int csg_last_depth(csg_ctx* ctx, const float** depth, uint32_t* n_frames);

/* Simulated stereo-camera depth: the ideal depth of a frame as a stereo depth
 * camera registered to the colour camera would return it -- half-occlusion holes
 * beside foreground edges, a matching window that erodes edges and drops thin
 * structure, disparity quantisation and disparity noise (both grow as z^2 in
 * depth) -- with the cause of every missing value.  A stand-alone pass on
 * device memory only, like csg_voxel_cloud: it needs no scene and no earlier
 * render, and the frame size is the job's own.  Everything is local and an
 * integer in the disparity domain, so the result is defined to the bit.  Every
 * float operation below is float32 and rounds once (no contraction); '/' is the
 * correctly rounded division.  W = width, H = height, b = baseline, r = radius.
 *
 * Geometry.  The depth image is registered to the colour camera, as in aligned
 * RGB-D datasets.  The second camera sits at (b, 0, 0) in the OpenCV camera
 * frame; b may be negative.  A point at depth z has the disparity
 * D = fx * |b| / z; the second camera sees it in column x - D for b > 0 and
 * x + D for b < 0.
 *
 * Per pixel (x, y) of frame f, p = y * W + x, d = depth[f][y][x]:
 *   fb = fl32(fx_f * |b|) with fx_f = intrinsics[f][0] (the [n][4] table of
 *     csg_point_job.intrinsics; only fx is read).
 *   D = fl32(fb / d).
 *   The pixel is a surface iff d is finite, d > 0 and D > 0 (a NaN D fails).
 *   dq, the disparity in 1/256 px: 2^30 if D is infinite or D >= 4194304.0f,
 *     otherwise (uint32) fl32(fl32(D * 256.0f) + 0.5f).
 *   u, the second camera's column in 1/256 px: 256 * x + 128 - dq for b > 0,
 *     256 * x + 128 + dq for b < 0.  It fits int32.
 *
 * Cause.  sensor_cause[f][y][x]; the first rule that applies wins:
 *   1 none     the pixel is not a surface.
 *   2 range    !(z_min <= d <= z_max).
 *   3 half-occluded   the pixel is hidden from the second camera.  b > 0: some
 *              surface pixel x' > x of the same row has u(x') <= u(x).  b < 0:
 *              some surface pixel x' < x has u(x') >= u(x).  Every surface
 *              pixel occludes, out-of-range ones included; others never do.
 *   4 band     only with CSG_SENSOR_CLIP_BAND.  b > 0: u < 0.  b < 0:
 *              u >= 256 * W.  The strip the second camera's image lacks.
 *   5 support  a pixel is lit if none of the rules 1-4 applies to it.  n counts
 *              the lit pixels (x', y') of the (2r+1)^2 window around (x, y) with
 *              |dq(x', y') - dq(x, y)| <= tol; the centre counts, pixels outside
 *              the image do not.  Cause 5 iff n < min_support.
 *   6 noise    m <= 0, with m as below.
 *   0 return   none of the rules 1-6 applies.
 *
 * Value of a return, with fmix32 as under csg_sample_object_points:
 *   key_f = frame_keys[f], or f when frame_keys is NULL.
 *   base = fmix32(seed ^ key_f), h1 = fmix32(base ^ p),
 *   h2 = fmix32(h1 ^ 0x9E3779B9u).
 *   g = (h1 & 0xFFFF) + (h1 >> 16) + (h2 & 0xFFFF) + (h2 >> 16) - 131070, in
 *     int64: a sum of four uniforms, mean 0, standard deviation 65536 / sqrt(3).
 *   e = (g * noise_k + 32768) >> 16, an arithmetic shift in int64.
 *   sh = 8 - subpixel_bits.
 *   m = (dq + e + ((1 << sh) >> 1)) >> sh, arithmetic.
 *   dn = (uint32)(m << sh), below 2^31.
 *   sensor_depth = fl32(fl32(fb * 256.0f) / (float)dn); the conversion rounds
 *     to nearest even.
 *
 * What is written.  sensor_depth is 0.0f wherever the cause is not 0: the "no
 * return" value of real depth files, and what CSG_FILE_DEPTH16_PNG maps to sample
 * 0.  sensor_count[f][c], c = 0..6, holds the pixels of each cause.  Every
 * element of every requested output is written.  The result is a pure function
 * of the inputs: no float atomics, nothing depends on scheduling or on the
 * frame's place in the batch except through its key.  No input value yields an
 * address outside the arrays described.
 *
 * sensor_depth must not overlap depth (the kernels read neighbours); no output
 * may overlap a source.  This is checked on the host.
 *
 * Enqueues on `stream` (NULL = the context's stream) and returns; behind the
 * render that wrote the sources on the same stream it needs no synchronisation.
 * csg_synchronize waits for it under the rule for the crops.  The pass has
 * scratch of its own (4 bytes per pixel and 32 per frame), grown to the job and
 * bounded at 256 MiB: a job that needs more runs as ranges of frames.  An event
 * orders passes on different streams; it never touches the render's work buffers.
 *
 * Returns -1 for a NULL ctx.  CSG_ERR_INVALID, nothing enqueued or written: job
 * NULL; n_frames == 0; width or height outside 1..8192; radius above 4;
 * min_support outside 1..(2r+1)^2; subpixel_bits above 8; noise_k above 2^20;
 * an unknown flag; baseline not finite or zero; z_min or z_max not finite, or
 * not 0 < z_min <= z_max; depth or intrinsics NULL; no output at all; an
 * output that overlaps a source; a pointer that is not aligned to its element
 * (4 bytes for all but sensor_cause). */
#define CSG_SENSOR_CLIP_BAND 1u   /* rule 4: no return outside the second camera's image */
typedef struct {
  uint32_t width, height;      /* of the frames: 1..8192 each */
  uint32_t radius;             /* r: 0..4, the matching window is (2r+1)^2 */
  uint32_t min_support;        /* 1..(2r+1)^2 */
  uint32_t tol;                /* disparity tolerance of the window, 1/256 px */
  uint32_t subpixel_bits;      /* 0..8: returned disparities are multiples of 2^-bits px */
  uint32_t noise_k;            /* 0..2^20: disparity noise, standard deviation noise_k / sqrt(3) / 256 px */
  uint32_t seed;
  uint32_t flags;              /* CSG_SENSOR_* */
  float    baseline;           /* b, metres: finite, not 0 */
  float    z_min, z_max;       /* metres: finite, 0 < z_min <= z_max */
  /* sources, device memory */
  const float*    depth;       /* [n][H][W] as csg_outputs.depth */
  const float*    intrinsics;  /* [n][4] fx fy cx cy as csg_point_job.intrinsics; only fx is read */
  const uint32_t* frame_keys;  /* [n], or NULL: key_f = f */
  /* outputs, device memory; any may be NULL, not all */
  float*    sensor_depth;      /* [n][H][W], 0.0f where there is no return */
  uint8_t*  sensor_cause;      /* [n][H][W] */
  uint32_t* sensor_count;      /* [n][7] */
} csg_sensor_job;
int csg_sensor_depth(csg_ctx* ctx, const csg_sensor_job* job, uint32_t n_frames, void* stream);

/* Farthest-point sampling of point sets: K samples of each set, the first a
 * hashed start and every later one the candidate farthest from all samples chosen
 * before it -- the reduction of a cloud to a fixed size that PointNet++, VoteNet,
 * PVN3D and FFB6D perform on their inputs, here on the outputs of
 * csg_sample_object_points (rows of a slot, pt_count as counts) and
 * csg_voxel_cloud (rows of a frame, vx_total as counts).  Every prefix of a run is
 * itself a run.  A stand-alone pass on device memory only, like csg_sensor_depth:
 * it needs no scene and no earlier render.  S = n_sets, C = rows, P = pool,
 * K = samples.  Every float operation below is float32 and rounds once (no
 * contraction).
 *
 * Rows of a set.  m_s = C when counts is NULL; m_s = 0 when counts[s] ==
 * 0xFFFFFFFF (csg_voxel_cloud's overflow mark: those rows are unspecified);
 * otherwise m_s = min(counts[s], C).
 *
 * Candidates.  c_s = min(m_s, P).  Candidate j, 0 <= j < c_s, is row
 * r_j = ((uint64)j * m_s) / c_s: j itself when m_s <= P, an even stride through
 * the rows otherwise; strictly increasing.  A candidate is valid iff its three
 * coordinates are finite.  v_s is the number of valid candidates.
 *
 * Distance.  For points a and b: dx = fl32(ax - bx), likewise dy and dz;
 *   d2 = fl32(fl32(fl32(dx*dx) + fl32(dy*dy)) + fl32(dz*dz)).
 * For valid candidates it is never NaN and never negative zero; it may be +inf.
 *
 * Start.  key_s = set_keys[s], or s when set_keys is NULL.
 *   h = fmix32(fmix32(seed ^ key_s) ^ 0x9E3779B9u), fmix32 as under
 *   csg_sample_object_points; j0 = (uint32)(((uint64)h * c_s) >> 32).
 * The start is the valid candidate j that minimises (j + c_s - j0) % c_s: the
 * first valid one at or after j0, cyclically.
 *
 * Steps.  mind_j = +inf for every valid j.  Step 0 chooses the start, and
 * fp_dist2[s][0] = +inf.  After choosing candidate a, mind_j = min(mind_j,
 * d2(p_j, p_a)) for every valid j, so mind_a becomes 0.  Step t >= 1: g is the
 * maximum of mind_j over the valid j.  If g == 0, t0 = t and the run stops (every
 * valid candidate coincides with a sample).  Otherwise the step chooses the lowest
 * j with mind_j == g, and fp_dist2[s][t] = g.  If all K steps choose, t0 = K.
 * fp_dist2[s][1 .. t0 - 1] is therefore non-increasing, and every valid
 * candidate lies within fp_dist2[s][t0 - 1] (squared) of a sample.
 *
 * Outputs.  For t < t0: fp_index[s][t] = r_j, the row within the set, and
 * fp_xyz[s][t] is that row, bit for bit.  For t >= t0 (the wrap, as the point
 * samples wrap with s mod M): fp_index and fp_xyz repeat entry t mod t0, and
 * fp_dist2 = 0.0f.  fp_count[s] = {t0, v_s}.
 * The empty set (v_s == 0): fp_count = {0, 0}, fp_index all 0xFFFFFFFF, fp_xyz
 * the bits 0x7FC00000, fp_dist2 0.0f.
 *
 * Payload gathers.  Up to 4 records {src, dst, row_bytes, fill}: src is
 * [S][C][row_bytes], dst is [S][K][row_bytes], row_bytes is 1..64, and rows are
 * copied as bytes: dst[s][t] = src[s][fp_index[s][t]]; in an empty set every byte
 * of the dst rows is `fill` (its low 8 bits).  This carries colours, labels or
 * pixel indices along without a second pass.
 *
 * Every element of every requested output is written.  The result is a pure
 * function of the inputs: it does not depend on scheduling, on the set's place
 * in the call except through its key, or on how the kernel partitions the
 * candidates (no atomics, no float reductions; ties go to the lowest j).  No
 * coordinate or count yields an address outside the arrays described.
 *
 * Enqueues on `stream` (NULL = the context's stream) and returns; behind the
 * pass that wrote the sources on the same stream it needs no synchronisation.
 * csg_synchronize waits for it under the rule for the crops.  The pass has no
 * scratch: a set's candidates live in the registers of one workgroup, which is
 * why P is at most 16384 (larger sets go through the stride of the candidates).
 *
 * Returns -1 for a NULL ctx.  CSG_ERR_INVALID, nothing enqueued or written: job
 * NULL; n_sets == 0; rows outside 1..2^24; pool outside 1..16384; samples
 * outside 1..16384; xyz NULL; no output at all (no fp_* and no payload); more
 * than 4 payloads; a payload with a NULL src or dst, or row_bytes outside
 * 1..64; an output that overlaps a source or another output; a pointer that is
 * not aligned to 4 bytes (xyz, counts, set_keys, fp_index, fp_xyz, fp_dist2 and
 * fp_count; payloads need no alignment). */
#define CSG_FPS_MAX_PAYLOADS 4u
typedef struct {            /* 24 bytes */
  const void* src;          /* [S][C][row_bytes], device memory */
  void*       dst;          /* [S][K][row_bytes], device memory */
  uint32_t    row_bytes;    /* 1..64 */
  uint32_t    fill;         /* low 8 bits: every byte of an empty set's rows */
} csg_fps_payload;
typedef struct {
  uint32_t rows;               /* C: rows per set, 1..2^24 */
  uint32_t pool;               /* P: candidates per set at most, 1..16384 */
  uint32_t samples;            /* K: 1..16384 */
  uint32_t seed;
  uint32_t n_payloads;         /* 0..CSG_FPS_MAX_PAYLOADS */
  uint32_t pad;
  /* sources, device memory */
  const float*    xyz;         /* [S][C][3], always */
  const uint32_t* counts;      /* [S], or NULL: every set has C rows */
  const uint32_t* set_keys;    /* [S], or NULL: key_s = s */
  /* outputs, device memory; any may be NULL, not all unless there is a payload */
  uint32_t* fp_index;          /* [S][K] */
  float*    fp_xyz;            /* [S][K][3] */
  float*    fp_dist2;          /* [S][K] */
  uint32_t* fp_count;          /* [S][2] = t0, v_s */
  csg_fps_payload payloads[CSG_FPS_MAX_PAYLOADS];
} csg_fps_job;
int csg_farthest_points(csg_ctx* ctx, const csg_fps_job* job, uint32_t n_sets, void* stream);

/* Lens distortion (Brown-Conrady, OpenCV's rational model): pinhole frames of a
 * "source camera" resampled into the frames of an "output camera" whose lens
 * distorts, with every label moved along -- ids, depth, object coordinates,
 * per-label boxes and keypoints.  Three calls: csg_lens_map makes the lens's
 * map on the host, once; csg_lens_remap resamples frames by a map;
 * csg_lens_points moves keypoints by the forward model.
 *
 * Pixels.  Pixel i covers [i, i + 1) and its centre is i + 0.5, in both cameras
 * (cx = width / 2 for a centred lens; OpenCV's numbers are these minus 1/2).
 *
 * Model.  Normalised pinhole (x, y) to normalised distorted (xd, yd):
 *   r2 = x^2 + y^2
 *   R  = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
 *   xd = x R + 2 p1 x y + p2 (r2 + 2 x^2)
 *   yd = y R + p1 (r2 + 2 y^2) + 2 p2 x y
 * The output pixel of a point is (fx xd + cx, fy yd + cy), its source pixel
 * (sfx x + scx, sfy y + scy).
 *
 * csg_lens_map needs no context and no GPU.  For every output pixel it inverts
 * the model by Newton's method in float64 (16 steps whatever the data, the
 * analytic Jacobian, every operation rounded once; the order of operations is
 * the header comment of csrc/csg_lens_map.h, restated by tests/lens_ref.py) and
 * writes map[j][i] = (qx, qy), the source position in 1/256 source pixel
 * (qx = floor(sx * 256 + 0.5)), or (INT32_MIN, cause) where the pixel shows
 * nothing, the first rule that applies giving the cause:
 *   1 no preimage  a value is not finite, the forward model of the result misses
 *                  the pixel's centre by more than 2^-10 output pixels, or the
 *                  Jacobian there does not have both determinant > 0 and trace
 *                  > 0 (the result lies beyond the fold of a strong barrel lens)
 *   2 outside      the source pixel (qx >> 8, qy >> 8) is not in the source frame
 * counts (or NULL) gets {valid, no preimage, outside}.  CSG_ERR_INVALID, nothing
 * written: model or map NULL, a size outside 1..8192, a number that is not
 * finite, a focal length that is not > 0.  No input yields undefined behaviour.
 *
 * csg_lens_remap: a stand-alone pass on device memory only, like
 * csg_sensor_depth; the two frame sizes are the job's own and the result is
 * defined to the bit.  W x H = the output's size, SW x SH = the source's.  Per
 * output pixel (i, j) of frame f with (qx, qy) = map[j][i] (one map for every
 * frame; it may be the caller's own, of any model):
 *   cause  qx == INT32_MIN: 1 if qy == 1, else 2.  Otherwise 2 if the source
 *          pixel (px, py) = (qx >> 8, qy >> 8) (arithmetic shifts) is not in
 *          [0, SW) x [0, SH), else 0.  No map value yields an address outside
 *          the arrays described.
 *   cause 0:
 *     lens_instance, lens_depth, lens_coords = instance, depth, obj_coords at
 *       [f][py][px], bit for bit (a NaN depth included): a label and its depth
 *       come from the same source pixel.  Depth stays the distance along the
 *       optical axis, as OpenCV's model has it for distorted cameras.
 *     lens_rgb, rgb_filter = CSG_LENS_FILTER_BILINEAR: tx = qx - 128,
 *       x0 = tx >> 8, fx8 = tx & 255, and ty, y0, fy8 likewise; the taps
 *       (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), each coordinate
 *       clamped into the source, have the weights (256 - fx8)(256 - fy8),
 *       fx8 (256 - fy8), (256 - fx8) fy8, fx8 fy8; per channel
 *       (sum of w * c + 32768) >> 16.  Colours blend across silhouettes, as in
 *       the crops.  CSG_LENS_FILTER_NEAREST: rgb[f][py][px].
 *     lens_valid = 0.
 *   any other cause: RGB 0, id -1, depth +inf, coords 0, lens_valid = cause.
 *   lens_stats[f][l] = pixels, minx, miny, maxx, maxy of label l in
 *     lens_instance (as csg_outputs.inst_stats, a label without pixels gets 0,
 *     0xFFFFFFFF, 0xFFFFFFFF, 0, 0); ids outside [0, n_labels) are counted nowhere.
 *   lens_count[f] = the frame's pixels of cause 0, 1 and 2.
 * Every element of every requested output is written; integer atomics only, so
 * the result is a pure function of the inputs.
 *
 * Enqueues on `stream` (NULL = the context's stream) and returns; behind the
 * render that wrote the sources on the same stream it needs no synchronisation.
 * csg_synchronize waits for it under the rule for the crops.  The pass has no
 * scratch and never touches the render's work buffers.
 *
 * Returns -1 for a NULL ctx.  CSG_ERR_INVALID, nothing enqueued or written: job
 * NULL; n_frames == 0; a size outside 1..8192; an unknown rgb_filter; map NULL;
 * no output at all; an output without its source (lens_rgb: rgb, lens_instance
 * and lens_stats: instance, lens_depth: depth, lens_coords: obj_coords);
 * lens_stats with n_labels == 0 (above CSG_SPAN_MAX_LABELS: CSG_ERR_LIMIT); an
 * output that overlaps a source, the map or another output; a pointer that is
 * not aligned: 8 bytes for map, 4 for instance, depth, lens_rgb, lens_instance,
 * lens_depth, lens_coords, lens_stats and lens_count, 2 for obj_coords (rgb and
 * lens_valid need none).
 *
 * csg_lens_points: the keypoints of the source render in the output camera, by
 * the forward model in float32 (the model's numbers rounded to float32 first,
 * every operation rounded once, '/' correctly rounded).  Per keypoint (u, v):
 *   x = (u - scx) / sfx, y = (v - scy) / sfy
 *   xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy, r4 = r2 * r2, r6 = r4 * r2
 *   N  = 1 + ((k1 * r2 + k2 * r4) + k3 * r6), D likewise with k4, k5, k6
 *   Np = (k1 + (2 * k2) * r2) + (3 * k3) * r4, Dp likewise
 *   R  = N / D, Rp = (Np * D - N * Dp) / (D * D)
 *   xd = (x * R + (2 * p1) * xy) + p2 * (r2 + 2 * xx)
 *   yd = (y * R + p1 * (r2 + 2 * yy)) + (2 * p2) * xy
 *   a  = ((R + (2 * xx) * Rp) + (2 * p1) * y) + (6 * p2) * x
 *   b  = ((2 * xy) * Rp + (2 * p1) * x) + (2 * p2) * y
 *   d  = ((R + (2 * yy) * Rp) + (6 * p1) * y) + (2 * p2) * x
 *   u' = fx * xd + cx, v' = fy * yd + cy
 * If one of u', v', a, b, d is not finite: lens_uv = (0, 0), lens_vis = 0.
 * Otherwise lens_uv = (u', v'), and lens_vis = 0 if the point is outside the
 * output frame (not 0 <= u' < W and 0 <= v' < H) or beyond the fold (not both
 * a * d - b * b > 0 and a + d > 0), else keypoints_vis.  It reads of the job
 * `model` (host memory, read before the call returns; its sizes as csg_lens_map
 * checks them), n_keypoints (1..65536), keypoints_uv, keypoints_vis, lens_uv and
 * lens_vis (all needed, 4-byte aligned, no output over a source).  Stream rules
 * as above. */
typedef struct {
  uint32_t width, height;          /* output camera: 1..8192 each */
  uint32_t src_width, src_height;  /* source camera: 1..8192 each */
  double fx, fy, cx, cy;           /* output camera, pixels */
  double k1, k2, p1, p2, k3, k4, k5, k6;   /* OpenCV's order */
  double sfx, sfy, scx, scy;       /* source camera, pixels */
} csg_lens_model;                  /* 144 bytes */
int csg_lens_map(const csg_lens_model* m, int32_t* map /* host [H][W][2] */, uint32_t* counts /* [3] or NULL */);

#define CSG_LENS_FILTER_BILINEAR 0u
#define CSG_LENS_FILTER_NEAREST 1u
typedef struct {
  uint32_t width, height;          /* W, H: of the output frames */
  uint32_t src_width, src_height;  /* SW, SH: of the source frames */
  uint32_t n_labels;               /* labels of lens_stats */
  uint32_t rgb_filter;             /* CSG_LENS_FILTER_* */
  const int32_t* map;              /* device [H][W][2] */
  /* sources, device memory, layouts of csg_outputs at SW x SH; any may be NULL */
  const uint8_t*  rgb;             /* [n][SH][SW][3] */
  const int32_t*  instance;        /* [n][SH][SW] */
  const float*    depth;           /* [n][SH][SW] */
  const uint16_t* obj_coords;      /* [n][SH][SW][3] */
  /* outputs, device memory; any may be NULL, not all */
  uint8_t*  lens_rgb;              /* [n][H][W][3] */
  int32_t*  lens_instance;         /* [n][H][W] */
  float*    lens_depth;            /* [n][H][W] */
  uint16_t* lens_coords;           /* [n][H][W][3] */
  uint8_t*  lens_valid;            /* [n][H][W] 0 = valid, else the cause */
  uint32_t* lens_stats;            /* [n][n_labels][5] */
  uint32_t* lens_count;            /* [n][3] = valid, no preimage, outside */
  /* csg_lens_points only */
  const csg_lens_model* model;     /* host memory */
  uint32_t n_keypoints;            /* K: 1..65536 */
  uint32_t pad;
  const float*   keypoints_uv;     /* [n][K][2] source pixels */
  const int32_t* keypoints_vis;    /* [n][K] */
  float*   lens_uv;                /* [n][K][2] output pixels */
  int32_t* lens_vis;               /* [n][K] */
} csg_lens_job;
int csg_lens_remap(csg_ctx* ctx, const csg_lens_job* job, uint32_t n_frames, void* stream);
int csg_lens_points(csg_ctx* ctx, const csg_lens_job* job, uint32_t n_frames, void* stream);

/* Stand-alone 3D->2D projection (host buffers): uv [n][2], vis [n] without a
 * depth test (1 = in front and inside the image, 0 otherwise). */
int csg_project_keypoints(csg_ctx* ctx, const float* pts_world, uint32_t n, const float* view,
                          const float* proj, float* uv_out, int32_t* vis_out);

#ifdef __cplusplus
}
#endif
#endif /* CSG_API_H */
