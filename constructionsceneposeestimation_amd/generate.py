"""Batched dataset generator: the replacement for the reference's per-frame
``generate_data()`` loop (generate_construction_data.py:1379-2094).

Per frame the reference sets the camera, waits ~5.9 s of fixed sleeps for
Kit to render (:1592-1609), then pulls RGB / depth / point cloud / boxes and
writes them (:1668-2072).  Here a shard of frames is rendered in batches on
one GPU (camera poses and object layouts from the seeded schedule, every
frame a pure function of (seed, frame)), and host writer threads emit the
same files:

  rgb/rgb_%06d.png                 (:1672-1673)
  labels/label_%06d.json           (:2071-2072, schema :2056-2064 + keypoints_2d,
                                    bbox_2d, pixel_count; + occlusion_ratio with
                                    --occlusion)
  labels/instance_mask_%06d.npy    (:2066-2069; real ids here, -1 background)
  coco/coco_%06d.json              (optional "mask_rle": the frame's COCO image record and one annotation
                                    per visible object -- bbox, area, keypoints and the object's mask as a
                                    COCO run-length string made from the GPU's mask spans; no reference
                                    counterpart.  ``python -m constructionsceneposeestimation_amd.masks
                                    merge RUN_DIR`` joins them into coco/instances.json; with "amodal_rle"
                                    as well, objects of --amodal-kinds also carry amodal_bbox, amodal_area
                                    and amodal_segmentation: the full silhouette as if nothing stood in front)
  rgb/rgb_%06d.jpg                 (optional "rgb_jpg": a baseline JPEG, --jpeg-quality, --jpeg-subsampling,
                                    encoded on the GPU from the RGB the batch keeps there; no reference
                                    counterpart)
  depth/depth_%06d.csv             (:1687-1688)
  depth/depth_%06d.png             (:1690-1709, JET colour map made on the GPU)
  depth/depth_%06d.npy             (optional)
  pointcloud/pointcloud_%06d.txt   (:1716-1757; points from the GPU resolve, text encoded on the GPU)
  pointcloud/pointcloud_%06d.ply   (optional "pointcloud_ply": the same points as a binary PLY, xyz
                                    float32 + rgb uchar, 15 B per point; no reference counterpart)
  pointcloud/voxels_%06d.ply       (optional "pointcloud_voxel_ply": the frame's points voxel-downsampled on
                                    the GPU on a world-fixed grid of --voxel-size metres, one record per
                                    (cell, object): centroid, mean colour, ``label`` = the mask's inst_idx
                                    (-1 background) and point count, 23 B per record, voxel_cloud.read_ply;
                                    + pointcloud/objects.json as obj_coords' and the grid; with
                                    --voxel-points K at most K records, chosen by farthest-point sampling
                                    on the GPU and stored in that order; no reference counterpart)
  depth/sensor16_%06d.png          (optional "depth_sensor16_png": the depth a stereo depth camera registered to
                                    the colour camera would return -- half-occlusion holes, window erosion,
                                    quantised and noisy disparity (depth_sensor.StereoModel, made on the GPU
                                    behind the render) -- as depth16_png's 16-bit PNG at the same scale, 0 = no
                                    return; + depth/sensor.json: the model, the job's integers, the seed and the
                                    run's pixels per cause; no reference counterpart)
  depth/depth16_%06d.png           (optional "depth16_png": 16-bit grey PNG at a fixed number of counts
                                    per metre, writers.depth_to_u16) + depth/depth16.json (the scale;
                                    0 = no hit)
  normals/normals_%06d.npy         (C5 normals, f16, optional)
  obj_coords/obj_coords_%06d.npy   (object coordinates / NOCS, H x W x 3 uint16, optional; no
                                    reference counterpart) + obj_coords/objects.json (each
                                    object's prim_path, class_name, inst_idx and box lo / hi)
  train_pbr/%06d/{rgb,depth,mask,mask_visib}/ + bop/frag_%06d.json
                                   (optional "bop": the BOP dataset layout, bop.py -- scene = frame // 1000;
                                    RGB (PNG, or JPEG with --bop-rgb jpg) and 16-bit depth PNGs, one
                                    mask_visib and one amodal mask PNG per listed object made on the GPU
                                    from the spans, and per-frame fragments
                                    that ``python -m constructionsceneposeestimation_amd.bop merge RUN_DIR``
                                    joins into scene_camera / scene_gt / scene_gt_info.json; no reference
                                    counterpart)
  lens/{rgb,depth16}_%06d.png + lens/coco_%06d.json + lens/lens.json
                                   (optional "lens": the frame as a camera with Brown-Conrady lens distortion
                                    shows it, lens.py -- the run's frames are the pinhole source camera, the
                                    output camera (--lens PRESET or --lens-coeffs, --lens-size) gets the widest
                                    view the source holds; RGB, 16-bit depth and ids resampled on the GPU behind
                                    the render, the COCO masks, boxes and keypoints of the distorted frame, and
                                    lens.json with the model, both cameras in both pixel conventions, the map's
                                    digest and the run's pixels per cause; the other kinds stay pinhole; no
                                    reference counterpart)
  logs/generation_summary.json     (:2090; statistics, frame_logs, counters)
  logs/generation_detail.log       (:254-263, per-frame entries + report)

The default outputs are the reference's (RGB PNG, depth CSV + PNG, point
cloud TXT, mask .npy, label JSON); ``--outputs`` picks others.

Sharding: ``--rank/--world`` (or RANK/WORLD_SIZE) pick the epochs this
process owns (shard.shard_of_range); no communication between shards.
Resume: frames whose label file already exists are skipped.

    python -m constructionsceneposeestimation_amd.generate --out /data/run0 --frames 1000
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys
import time
import multiprocessing as mp
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor
from functools import partial
from typing import List, Optional, Sequence

import numpy as np

from . import bop
from . import camera_math as cm
from . import depth_sensor
from . import lens
from . import masks
from . import prep_pool
from . import voxel_cloud
from .crops import DYNAMIC_KINDS, eligible_labels
from .object_points import intrinsics_rows
from .labels import OBJECT_LISTS, in_frustum, label_record, object_box, object_poses
from .quality_log import QualityLog
from .renderer import Renderer, make_frames, output_spec, scene_labels
from .shard import shard_of_range
from .workload import Workload
from .writer_pool import WriterPool
from .writers import JPEG_SUBSAMPLING, FragmentWriter, LabelWriter, write_jpeg
from .writer_pool import _write_png  # noqa: F401  (the generator's PNG settings; tools/gen_bench.py)


def default_writers() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    omp = int(os.environ.get("OMP_NUM_THREADS") or 0)   # the box's CPU share, when set
    return max(1, min(n, omp) if omp else n)


def _log_done(log: QualityLog, fut, log_args: dict, points: bool) -> None:
    ds = fut.result()                       # host depth counts (writer), else the GPU's
    gpu_ds = log_args.pop("gpu_depth_stats", None)
    ds = ds if ds is not None else gpu_ds
    log.frame(depth_stats=ds, points=ds["valid"] if points and ds else None, **log_args)


OUTPUTS = ("rgb", "mask", "depth_csv", "depth_png", "depth_npy", "pointcloud", "normals", "obj_coords",
           "pointcloud_ply", "depth16_png", "mask_rle", "amodal_rle", "rgb_jpg", "pointcloud_voxel_ply",
           "depth_sensor16_png")
# What the reference writes for every frame (GDP:1668-1771, 2055-2072): RGB PNG, depth CSV and
# JET depth PNG, point-cloud TXT, instance mask .npy; the label JSON is always written (it is the
# resume marker).
REFERENCE_OUTPUTS = ("rgb", "mask", "depth_csv", "depth_png", "pointcloud")
# The BOP dataset layout (bop.py): an output kind of its own, not part of "all" -- it brings its own
# image, depth and mask files and does not go with the other per-object mask outputs.
BOP_OUTPUT = "bop"
BOP_EXCLUDES = ("mask", "mask_rle", "amodal_rle")
# The frames as a camera with lens distortion shows them (lens.py): an output kind of its own, not part of
# "all" -- it brings its own camera, image, depth and annotation files under lens/; the other kinds of the
# same run stay pinhole.
LENS_OUTPUT = "lens"


# outputs encoded on the GPU in thread mode -> their csg_outputs.file_kinds kind (_lib.FILE_KINDS)
FILE_OF_OUTPUT = (("rgb", "rgb_png"), ("depth_csv", "depth_csv"), ("depth_png", "depth_png"),
                  ("pointcloud", "pointcloud_txt"), ("pointcloud_ply", "pointcloud_ply"),
                  ("depth16_png", "depth16_png"))
_PATHS = {"rgb": ("rgb", "rgb_{:06d}.png"), "depth_csv": ("depth", "depth_{:06d}.csv"),
          "depth_png": ("depth", "depth_{:06d}.png"), "pointcloud": ("pointcloud", "pointcloud_{:06d}.txt"),
          "pointcloud_ply": ("pointcloud", "pointcloud_{:06d}.ply"), "depth16_png": ("depth", "depth16_{:06d}.png"),
          "rgb_jpg": ("rgb", "rgb_{:06d}.jpg"), "pointcloud_voxel_ply": ("pointcloud", "voxels_{:06d}.ply"),
          "depth_sensor16_png": ("depth", "sensor16_{:06d}.png")}
_ENCODED_KIND = {"pointcloud": "encoded_pointcloud", "pointcloud_ply": "encoded_ply"}   # writer_pool.write_frame


def file_path(out_dir: str, output: str, frame: int) -> str:
    """The reference's file name of one output of a frame (GDP:1668-1716)."""
    d, name = _PATHS[output]
    return os.path.join(out_dir, d, name.format(frame))


def parse_outputs(spec: str) -> tuple:
    if spec in ("reference", ""):
        return REFERENCE_OUTPUTS
    if spec == "all":
        return OUTPUTS
    out = tuple(x.strip() for x in spec.split(",") if x.strip())
    bad = [x for x in out if x not in OUTPUTS + (BOP_OUTPUT, LENS_OUTPUT)]
    if bad:
        raise ValueError(f"unknown outputs {bad}; choose from {OUTPUTS + (BOP_OUTPUT, LENS_OUTPUT)}")
    check_bop(out)
    if "amodal_rle" in out and "mask_rle" not in out:
        raise ValueError("output amodal_rle adds to the annotations of mask_rle: ask for both")
    return out


def check_bop(outs) -> None:
    clash = [x for x in BOP_EXCLUDES if x in outs] if BOP_OUTPUT in outs else []
    if clash:
        raise ValueError(f"output bop writes its own per-object masks: it does not go with {clash}")
    if BOP_OUTPUT in outs and "pointcloud_voxel_ply" in outs:
        raise ValueError("output bop has no place for voxel clouds: it does not go with pointcloud_voxel_ply")
    if BOP_OUTPUT in outs and "depth_sensor16_png" in outs:
        raise ValueError("output bop has no place for sensor depth: it does not go with depth_sensor16_png")
    if BOP_OUTPUT in outs and LENS_OUTPUT in outs:
        raise ValueError("output bop has no place for lens distortion: it does not go with lens")


def lens_model(width: int, height: int, intr, preset: Optional[str] = None, coeffs=None,
               size: Optional[Sequence[int]] = None) -> "lens.LensModel":
    """The model of the lens output: the run's frames (``width`` x ``height`` with the intrinsics ``intr``) are
    the source camera; the output camera has ``size`` = (W, H) (default the frames'), the coefficients
    ``coeffs`` (k1 k2 p1 p2 k3 [k4 k5 k6]) or those of ``preset`` (lens.PRESETS, default "wide"), and the widest
    view whose every pixel the source frame holds (lens.fit_output)."""
    if coeffs is None:
        name = preset or "wide"
        if name not in lens.PRESETS:
            raise ValueError(f"lens preset {name!r}: one of {sorted(lens.PRESETS)}")
        coeffs = lens.PRESETS[name]
    elif preset is not None:
        raise ValueError("lens: a preset or coefficients, not both")
    coeffs = tuple(float(v) for v in coeffs)
    if len(coeffs) not in (5, 8) or not all(np.isfinite(coeffs)):
        raise ValueError(f"lens coefficients {coeffs!r}: 5 or 8 finite numbers k1,k2,p1,p2,k3[,k4,k5,k6]")
    W, H = (int(width), int(height)) if size is None else (int(size[0]), int(size[1]))
    if not (1 <= W <= 8192 and 1 <= H <= 8192):
        raise ValueError(f"lens size {W}x{H} outside 1..8192")
    return lens.fit_output(lens.output_camera(coeffs, W, H, 1.0),
                           (int(width), int(height), intr.fx, intr.fy, intr.cx, intr.cy))


def _write_lens_fragment(path: str, frame_id: int, **kw) -> None:
    """masks.coco_fragment of a lens frame, its image record naming the file beside it."""
    frag = masks.coco_fragment(frame_id, **kw)
    frag["image"]["file_name"] = f"rgb_{int(frame_id):06d}.png"
    with open(path, "wb") as fh:
        fh.write(masks.fragment_bytes(frag))


def sensor_model(preset: Optional[str] = None, baseline: Optional[float] = None,
                 noise_px: Optional[float] = None) -> "depth_sensor.StereoModel":
    """The stereo model of the depth_sensor16_png output: a preset of
    depth_sensor.PRESETS (default "site") with its baseline and disparity noise
    replaced where given."""
    name = preset or "site"
    if name not in depth_sensor.PRESETS:
        raise ValueError(f"depth sensor preset {name!r}: one of {sorted(depth_sensor.PRESETS)}")
    kw = {}
    if baseline is not None:
        kw["baseline"] = float(baseline)
    if noise_px is not None:
        kw["noise_sigma_px"] = float(noise_px)
    return dataclasses.replace(depth_sensor.PRESETS[name], **kw)


def render_outputs(outs: set, gpu_files: bool, host_depth: bool, occlusion: bool) -> list:
    """The renderer outputs (renderer.OUTPUT_KINDS) a run with file outputs
    ``outs`` asks for.  Label statistics and keypoints feed every label file;
    the label coverage ("covered", k_raster<true>) only ``occlusion_ratio``,
    which is not in the reference's label schema (GDP:2056-2064)."""
    if gpu_files:
        want = (["keypoints", "stats", "depth_stats"] + (["instance"] if "mask" in outs else [])
                + (["depth"] if host_depth else []) + (["depth_range"] if "depth_png" in outs else [])
                + (["normals"] if "normals" in outs else []) + (["obj_coords"] if "obj_coords" in outs else []))
    else:
        want = (["rgb", "instance", "keypoints", "stats"] + (["depth"] if host_depth else [])
                + (["depth_vis"] if "depth_png" in outs else [])
                + (["points"] if outs & {"pointcloud", "pointcloud_ply"} else [])
                + (["normals"] if "normals" in outs else []) + (["obj_coords"] if "obj_coords" in outs else []))
    return want + (["covered"] if occlusion else [])


def generate(out_dir: str, frames: List[int], workload: str = "C3", seed: int = 0, batch: int = 30,
             device: int = 0, depth: bool = False, depth_csv: bool = False, pointcloud: bool = False,
             width: Optional[int] = None, height: Optional[int] = None, writers: int = 0,
             resume: bool = True, normals: bool = False, outputs: Optional[tuple] = None,
             writer_mode: str = "thread", renderers: int = 0, object_list: str = "visible",
             occlusion: bool = False, sink: str = "disk", validate_pointcloud: bool = False,
             min_points: int = 100, max_retries: int = 5, prep_workers: int = -1,
             depth16_counts_per_metre: float = 250.0, amodal_kinds: Optional[Sequence[str]] = None,
             jpeg_quality: int = 95, jpeg_subsampling: str = "420", bop_rgb: str = "png",
             voxel_size: float = voxel_cloud.DEFAULT_VOXEL_SIZE, voxel_capacity: int = 0,
             depth_sensor_preset: Optional[str] = None, sensor_baseline: Optional[float] = None,
             sensor_noise_px: Optional[float] = None, sensor_seed: int = 0,
             voxel_points: int = 0, voxel_points_seed: int = 0, lens_preset: Optional[str] = None,
             lens_coeffs: Optional[Sequence[float]] = None, lens_size: Optional[Sequence[int]] = None) -> dict:
    """Render ``frames`` on one GPU and write them (``outputs``, default the
    reference's set; ``depth`` / ``depth_csv`` / ``pointcloud`` / ``normals``
    add the depth .npy, the depth .npy + CSV, the point cloud, the normals).
    ``writer_mode`` "thread" encodes in threads of this process (the native
    writers release the GIL), "process" in worker processes fed through
    shared memory (writer_pool.py; measured slower at 1080p C3: 184 vs 233
    frames/s, page faults on the shared ring and task pickling).
    ``object_list``: "visible" lists the objects with visible pixels in each
    label file; "frustum" also those whose 3D box meets the view frustum
    (labels.label_record; the reference lists Replicator's bounding_box_3d
    primPaths, whose inclusion rule is closed).
    ``occlusion`` adds each object's ``occlusion_ratio`` (Replicator's
    occlusionRatio) to the label files.  The reference never reads that field
    and its label schema (GDP:2056-2064) has none, so it is off by default: it
    needs the per-label unoccluded coverage, i.e. k_raster<true> (about +36%
    raster time).
    ``sink`` "discard" runs the whole pipeline (render, GPU encode, copy
    into the page-locked ring, writer threads) but writes every file to
    /dev/null: the generator's steady-state rate without a file system.
    ``validate_pointcloud`` (off by default, as ``enable_pointcloud_validation``
    in the reference, GDP:61): a frame whose point cloud has fewer than
    ``min_points`` points (GDP:59; the GPU's count of valid depth pixels) is
    rendered again from a jittered camera (Workload.camera's ``attempt``,
    GDP:1573-1581), up to ``max_retries`` attempts in all (GDP:60); a frame
    that fails them all is logged failed and writes no files (GDP:1662-1666).
    ``depth16_counts_per_metre``: the scale of the "depth16_png" output
    (default 250: 4 mm steps, 262.1 m range; recorded in depth/depth16.json).
    ``outputs`` with "mask_rle": each frame's per-object masks as COCO
    run-length strings in coco/coco_%06d.json (masks.coco_fragment).  The ids
    stay on the GPU (csg_keep_instance) and only their spans cross PCIe
    (Renderer.mask_spans_host, behind each batch; the dense ids are copied
    only when "mask" is asked for as well).
    ``outputs`` with "amodal_rle" (it needs "mask_rle"): the annotations of
    objects of ``amodal_kinds`` (default crops.DYNAMIC_KINDS; "all": every
    label) also carry ``amodal_bbox``, ``amodal_area`` and
    ``amodal_segmentation``, the object's full silhouette as if nothing stood in
    front of it, from one more pass over the scene behind each batch
    (Renderer.amodal_spans_host).
    ``outputs`` with "bop": the BOP dataset layout (bop.py) under
    ``train_pbr/``: RGB and 16-bit depth PNGs from the GPU encoders, one
    ``mask_visib`` and one ``mask`` PNG per listed object made on the GPU from
    the visible and the amodal spans (Renderer.mask_pngs_host), and a fragment
    ``bop/frag_%06d.json`` per frame for ``python -m ...bop merge``.  Listed
    are the objects of ``amodal_kinds`` with amodal pixels.  Thread writers
    only; not with "mask", "mask_rle" or "amodal_rle".
    ``outputs`` with "rgb_jpg": ``rgb/rgb_%06d.jpg``, a baseline JPEG at
    ``jpeg_quality`` (1..100) and ``jpeg_subsampling`` ("444" or "420").  With
    thread writers the batch keeps its RGB on the device (csg_keep_rgb), the
    files are encoded there behind the render (Renderer.jpegs_host,
    csg_encode_jpeg) and cross PCIe packed, in one copy; next to "rgb" both
    files are written, without it the PNG is neither encoded nor copied.
    Writer processes encode the host RGB with writers.jpeg_bytes (the same
    bytes).  ``bop_rgb`` "jpg": output "bop" writes ``rgb/%06d.jpg`` from the
    same pass instead of the RGB PNG.
    ``outputs`` with "pointcloud_voxel_ply": ``pointcloud/voxels_%06d.ply``, the
    frame's world-space points voxel-downsampled on a grid of ``voxel_size``
    metres that is fixed in the world, one labelled record per (cell, object)
    (voxel_cloud.py).  The batch keeps its points, ids and RGB on the device
    (csg_keep_points, csg_keep_instance, csg_keep_rgb), the records are made
    there behind the render (Renderer.voxel_cloud_host, csg_voxel_cloud) and only
    they cross PCIe.  ``voxel_capacity``: records per frame the pass starts with
    (0: voxel_cloud.DEFAULT_VOXEL_CAPACITY); a renderer keeps what its retries
    settled on.  Not with "bop".  ``voxel_points`` = K > 0 (at most 16384)
    reduces every cloud to at most K records by farthest-point sampling on the
    device (Renderer.voxel_cloud_host's ``keep``, csg_farthest_points), in
    farthest-point order: the first records of a file are a coarser cloud of
    the same frame.  The start is a function of ``voxel_points_seed`` and the
    frame id, not of batching or sharding.  ``pointcloud/objects.json`` and the
    summary then record ``voxel_points`` and the seed.
    ``outputs`` with "depth_sensor16_png": ``depth/sensor16_%06d.png``, the depth
    a stereo depth camera would return for the frame (depth_sensor.py): the
    model is ``depth_sensor_preset`` of depth_sensor.PRESETS (default "site")
    with ``sensor_baseline`` metres and ``sensor_noise_px`` pixels of disparity
    noise where given.  The batch keeps its depth on the device
    (csg_keep_depth), the pass runs there behind the render (csg_sensor_depth)
    and its image goes through the 16-bit depth PNG encoder
    (csg_encode_files) at ``depth16_counts_per_metre``.  A frame's noise is a
    function of ``sensor_seed`` and its frame id, not of batching or sharding.
    ``depth/sensor.json`` holds the model, the job's integers, the seed, the
    scale (``counts_per_metre``), ``invalid`` (the sample that means "no
    return", 0, as in depth/depth16.json) and the run's pixels per cause.
    Not with "bop".
    ``prep_workers``: processes that prepare batches ahead (epoch layouts,
    object poses, cameras; prep_pool.py), so that numpy work does not hold
    this process's GIL; -1 = two for runs of at least 20 batches, else none."""
    if object_list not in OBJECT_LISTS:
        raise ValueError(f"object_list {object_list!r}: choose from {OBJECT_LISTS}")
    outs = set(REFERENCE_OUTPUTS if outputs is None else outputs)
    if depth or depth_csv:
        outs.add("depth_npy")
    if depth_csv:
        outs.add("depth_csv")
    if pointcloud:
        outs.add("pointcloud")
    if normals:
        outs.add("normals")
    check_bop(outs)
    if not 0 <= int(voxel_points) <= 16384:
        raise ValueError(f"voxel_points {voxel_points!r} outside 0..16384")
    want_bop = BOP_OUTPUT in outs
    if bop_rgb not in ("png", "jpg"):
        raise ValueError(f"bop_rgb {bop_rgb!r}: 'png' or 'jpg'")
    bop_jpg = want_bop and bop_rgb == "jpg"
    want_jpg = "rgb_jpg" in outs or bop_jpg
    if want_jpg:
        if not 1 <= int(jpeg_quality) <= 100:
            raise ValueError(f"jpeg_quality {jpeg_quality!r} outside 1..100")
        if str(jpeg_subsampling) not in JPEG_SUBSAMPLING:
            raise ValueError(f"jpeg_subsampling {jpeg_subsampling!r}: '444' or '420'")
    if want_bop:
        if writer_mode != "thread":
            raise ValueError("output bop needs the GPU file encoders: writer_mode 'thread'")
        s16 = float(depth16_counts_per_metre)
        if not (np.isfinite(s16) and s16 > 0):
            raise ValueError(f"depth16_counts_per_metre {depth16_counts_per_metre!r}: a finite number > 0")
    wl = Workload(workload, seed=seed, width=width, height=height)
    if want_bop:
        bop.check_depth_scale(wl.intr.near, depth16_counts_per_metre)
    for d in ("rgb", "labels", "depth", "pointcloud", "normals", "logs"):
        os.makedirs(os.path.join(out_dir, d), exist_ok=True)
    want_vox = "pointcloud_voxel_ply" in outs
    if want_vox and not (np.isfinite(float(voxel_size)) and float(voxel_size) > 0 and int(voxel_capacity) >= 0):
        raise ValueError(f"voxel_size {voxel_size!r}: a finite number > 0; voxel_capacity {voxel_capacity!r}: >= 0")
    vox_keep = {"voxel_points": int(voxel_points), "voxel_points_seed": int(voxel_points_seed) & 0xFFFFFFFF} \
        if int(voxel_points) else {}
    want_sens = "depth_sensor16_png" in outs
    if want_sens:
        s16 = float(depth16_counts_per_metre)
        if not (np.isfinite(s16) and s16 > 0):
            raise ValueError(f"depth16_counts_per_metre {depth16_counts_per_metre!r}: a finite number > 0")
        sens_model = sensor_model(depth_sensor_preset, sensor_baseline, sensor_noise_px)
        sens_job = dict(sens_model.to_job_fields(), seed=int(sensor_seed) & 0xFFFFFFFF)
    want_lens = LENS_OUTPUT in outs
    if want_lens:
        if writer_mode != "thread":
            raise ValueError("output lens is made by GPU passes behind the render: writer_mode 'thread'")
        s16 = float(depth16_counts_per_metre)
        if not (np.isfinite(s16) and s16 > 0):
            raise ValueError(f"depth16_counts_per_metre {depth16_counts_per_metre!r}: a finite number > 0")
        lens_m = lens_model(wl.width, wl.height, wl.intr, lens_preset, lens_coeffs, lens_size)
        lens_host_map, _ = lens.build_map(lens_m)
        os.makedirs(os.path.join(out_dir, "lens"), exist_ok=True)
    if "obj_coords" in outs or want_vox:
        objs = []
        for o in wl.scene.objects:
            box = object_box(o)
            objs.append({"prim_path": o.prim_path, "class_name": o.class_name, "inst_idx": int(o.inst_idx),
                         "lo": box[0].tolist() if box else None, "hi": box[1].tolist() if box else None})
    if "obj_coords" in outs:   # the boxes that turn the maps back into metres (labels.decode_obj_coords)
        os.makedirs(os.path.join(out_dir, "obj_coords"), exist_ok=True)
        with open(os.path.join(out_dir, "obj_coords", "objects.json"), "w") as fh:
            json.dump({"objects": objs}, fh, indent=2)
    if want_vox:   # what a record's label names, and the grid
        with open(os.path.join(out_dir, "pointcloud", "objects.json"), "w") as fh:
            json.dump({"objects": objs, "voxel_size": float(np.float32(voxel_size)), **vox_keep}, fh, indent=2)
    if "amodal_rle" in outs and "mask_rle" not in outs:
        raise ValueError("output amodal_rle adds to the annotations of mask_rle: ask for both")
    if "mask_rle" in outs:
        os.makedirs(os.path.join(out_dir, "coco"), exist_ok=True)
    if "depth16_png" in outs:   # what a reader needs to turn the samples back into metres
        s16 = float(depth16_counts_per_metre)
        if not (np.isfinite(s16) and s16 > 0):
            raise ValueError(f"depth16_counts_per_metre {depth16_counts_per_metre!r}: a finite number > 0")
        with open(os.path.join(out_dir, "depth", "depth16.json"), "w") as fh:
            json.dump({"counts_per_metre": s16, "invalid": 0}, fh)
    if resume:
        frames = [f for f in frames if not os.path.exists(os.path.join(out_dir, "labels", f"label_{f:06d}.json"))]
    # batch preparation in worker processes, started (like the writer processes
    # below) before this process touches the GPU; each builds its own Workload
    n_prep = prep_workers if prep_workers >= 0 else (2 if len(frames) >= 20 * batch else 0)
    ppool = None
    if n_prep:
        ppool = ProcessPoolExecutor(max_workers=n_prep, mp_context=mp.get_context("spawn"),
                                    initializer=prep_pool.init, initargs=(workload, seed, width, height))
        for f in [ppool.submit(prep_pool.ping) for _ in range(2 * n_prep)]:   # every worker started now
            f.result()
    # Thread writers (the default): the PNGs, the depth CSV and the point
    # cloud are encoded on the GPU (Renderer.render_files, csg_encode.hip) and
    # the host only writes bytes; writer processes encode on the host (libcsgio).
    gpu_files = writer_mode == "thread"
    # (bop: its rgb and depth files are the GPU's rgb_png and depth16_png, whether or not those outputs
    # are asked for under their own names as well)
    enc_outs = outs | {"depth16_png"} | (set() if bop_jpg else {"rgb"}) if want_bop else outs
    kinds = tuple(k for o, k in FILE_OF_OUTPUT if o in enc_outs) if gpu_files else ()
    # host depth for its own files; the quality log's depth counts come from
    # the GPU (depth_stats) in thread mode, from the host depth otherwise
    host_depth = "depth_npy" in outs or (not gpu_files and bool(outs & {"depth_csv", "pointcloud", "depth16_png"}))
    log = QualityLog(os.path.join(out_dir, "logs"))
    want = render_outputs(outs, gpu_files, host_depth, occlusion)
    if validate_pointcloud and "depth_stats" not in want:
        want.append("depth_stats")   # the per-frame valid point count the validation reads
    n_writers = writers or default_writers()
    # Renderer contexts on the device, each with its own stream and work
    # buffers, rendering alternate batches from their own threads: one batch's
    # encode and copy overlap the next ones' render (C3 1080p into RAM, 16
    # writers: 1,038 frames/s with two, 846 with one; at steady state with the
    # files to /dev/null, three: 1,823 / 515 frames/s without / with the point
    # cloud, two: 1,739 / 505; profiles/r05/generate_steady.json.  Round 6, with
    # the 1-byte id wire and two prep workers, batches of 60: three 2,028-2,150,
    # four 2,029-2,041, three with batches of 120 1,912-1,975 frames/s without
    # the point cloud; profiles/r06/ab/prep_workers/).
    n_rend = renderers or (3 if gpu_files else 1)
    # the writer processes start here, before this process touches the GPU
    pool = WriterPool(output_spec(batch, wl.height, wl.width, wl.n_keypoints(), scene_labels(wl.scene), want),
                      n_writers, n_slots=2 + n_rend, mode=writer_mode, sink=sink)
    rends = [Renderer(wl.scene, wl.width, wl.height, max_frames=batch, device=device) for _ in range(n_rend)]
    r = rends[0]
    want_rle = "mask_rle" in outs
    span_cap = {}   # renderer -> the span capacity its last batch needed (mask_spans_host grows it)
    want_amodal = "amodal_rle" in outs
    amodal_cap = {}  # ... and likewise for amodal_spans_host
    amodal_el = None   # the labels that get amodal masks (None: all)
    if want_amodal and not (amodal_kinds is not None and "all" in amodal_kinds):
        amodal_el = eligible_labels(wl.scene, DYNAMIC_KINDS if amodal_kinds is None else tuple(amodal_kinds))
    fw = None       # thread mode: the native fragment writer (writers.FragmentWriter), made with the first poses
    kp_by_obj = masks.keypoints_by_object(wl.kp_table) if (want_rle and not gpu_files) or want_lens else None
    if want_rle or want_bop:    # host-output batches keep their ids on the device for the span pass
        for x in rends:
            x.keep_instance(True)
    if want_jpg and gpu_files:   # ... and their RGB for the JPEG pass, whether or not anything else needs it
        for x in rends:
            x.keep_rgb(True)
    if want_vox:    # ... and their points, ids and RGB for the voxel pass
        for x in rends:
            x.keep_points(True)
            x.keep_instance(True)
            x.keep_rgb(True)
    if want_sens:   # ... and their depth for the sensor pass
        for x in rends:
            x.keep_depth(True)
    if want_lens:   # ... and their RGB, ids and depth for the lens pass
        for x in rends:
            x.keep_rgb(True)
            x.keep_instance(True)
            x.keep_depth(True)
    lens_cap, lens_span_cap, lens_buf = {}, {}, {}   # per renderer: file bytes, span capacity, device arrays
    lens_counts = np.zeros(3, np.int64)              # the run's pixels per cause
    sens_cap = {}   # renderer -> the bytes its last batch's sensor PNGs took
    sens_buf = {}   # renderer -> its device arrays for the pass (intrinsics, keys, sensor depth, counts)
    sens_counts = np.zeros(7, np.int64)   # the run's pixels per cause
    vox_cap = {}    # renderer -> the voxel capacity its last batch needed (voxel_cloud_host grows it)
    vox_stats = {"frames": 0, "voxels": 0, "voxels_max": 0}
    jpg_cap = {}    # renderer -> the bytes its last batch's JPEG files took (jpegs_host repeats a pass that overflows)
    bop_masks, bop_em, bop_scenes = {}, {}, set()   # per renderer; per epoch (bop.epoch_models); scene folders made
    if want_bop:
        bop_el = None if amodal_kinds is not None and "all" in amodal_kinds else eligible_labels(
            wl.scene, DYNAMIC_KINDS if amodal_kinds is None else tuple(amodal_kinds))
        bop_masks = {id(x): bop.BatchMasks(x, wl.scene, bop_el) for x in rends}
        if frames and sink == "disk":
            bop.write_run_tables(out_dir, wl.scene, bop.epoch_models(wl.epoch(frames[0] // 10).object_frames),
                                 wl.intr.pixel_projection(), wl.width, wl.height, depth16_counts_per_metre)
    if gpu_files:   # page-locked slots, and buffers for the encoded files (an estimate, grown on demand)
        npx = wl.width * wl.height
        est = {"rgb_png": 2 * npx, "depth_csv": 10 * npx, "depth_png": npx, "pointcloud_txt": 48 * npx,
               "pointcloud_ply": 15 * npx + 256, "depth16_png": 2 * npx}
        pool.use_pinned(r.host_buffer, batch * sum(est[k] for k in kinds) + (1 << 20) if kinds else 0,
                        free=r.free_host_buffer)
    nk = len(kinds)
    intr = wl.intr
    # thread mode: label files written natively from the frame's arrays (no GIL)
    lw = LabelWriter(wl.kp_table, wl.intr.params(), scene_labels(wl.scene), wl.height, wl.width) if gpu_files else None
    pose_cache = {}
    pending = []
    has_points = bool(outs & {"pointcloud", "pointcloud_ply"})   # the quality log's point count

    def cov_of(out, k):   # the frame's label coverage (occlusion_ratio), when rendered
        return out["label_covered"][k] if "label_covered" in out else None

    t_render = t_slot_wait = t_prep = t_main_wait = t_labels = 0.0
    d2h = []   # bytes each batch copied to the host (files + arrays), appended by the render threads
    ids_wire = r.host_id_bytes()   # instance ids cross PCIe as 1-, 2- or 4-byte values (csg_host_id_bytes)

    def wire_bytes(out):   # the host arrays' bytes as they crossed PCIe (ids narrowed, widened on the host)
        return sum(v.nbytes for v in out.values()) - (out["instance"].size * (4 - ids_wire) if "instance" in out else 0)
    t0 = time.time()
    starts = list(range(0, len(frames), batch))

    def prepare(b: int):
        """Host state of batch b (epoch layouts, object poses, cameras), made
        ahead in its own thread so the render thread only renders."""
        fb = frames[starts[b]:starts[b] + batch]
        if ppool is not None:   # computed in a worker process, installed here
            eps, cams = ppool.submit(prep_pool.prepare, list(fb), sorted({f // 10 for f in fb})).result()
            for e, (st, poses) in eps.items():
                wl.install_epoch(e, st)
                if e not in pose_cache:
                    if len(pose_cache) >= 256:
                        pose_cache.pop(next(iter(pose_cache)))
                    pose_cache[e] = poses
            for f, cam in cams.items():
                wl.install_camera(f, cam)
            return
        for e in sorted({f // 10 for f in fb}):
            st = wl.epoch(e)
            if e not in pose_cache:
                if len(pose_cache) >= 256:   # bounded over long runs (an epoch is met once)
                    pose_cache.pop(next(iter(pose_cache)))
                pose_cache[e] = object_poses(wl.scene, st.object_frames)
        wl.frame_params(fb)

    def render_batch(b: int):
        """Batch b into its slot of the writer ring (runs one batch ahead of
        the label loop, in its own thread: the C-ABI call releases the GIL)."""
        fb = frames[starts[b]:starts[b] + batch]
        if b < len(prep_f):
            prep_f[b].result()
        slot = b % pool.n_slots
        r = rends[b % n_rend]
        tw = time.time()
        if kinds:   # files buffers this renderer replaced at an earlier batch (grow_files)
            pool.release_retired(r.free_host_buffer)
        arrays = pool.arrays(slot)          # (waits until the writers are done with the slot)
        tp = time.time()
        epochs = sorted({f // 10 for f in fb})
        set_of = {}
        for k, e in enumerate(epochs):
            st = wl.epoch(e)
            r.set_instance_transforms(k, st.models)
            r.set_keypoints(k, st.keypoints)
            if "obj_coords" in outs:
                r.set_object_frames(k, st.object_frames)
            if st.dr is not None:
                r.set_dr_light(k, st.dr.light)
                r.set_dr_textures(k, st.dr.textures)
            set_of[e] = k
        views, projs = wl.frame_params(fb)
        tr = time.time()
        sets = [set_of[f // 10] for f in fb]

        rle = [None]   # the batch's (offsets, spans) per frame, with "mask_rle"
        arle = [None]  # the batch's amodal ((offsets, spans) per frame, stats), with "amodal_rle"

        def spans_of_batch() -> int:
            ids, nf = r.last_instance()
            if not ids or nf != len(fb):
                raise RuntimeError(f"mask_rle: the batch kept {nf} id images, {len(fb)} frames rendered")
            rle[0], span_cap[id(r)] = r.mask_spans_host(len(fb), ids, capacity=span_cap.get(id(r), 0))
            nb = sum(o.nbytes + sp.nbytes for o, sp in rle[0])
            if want_amodal:   # one pass over the scene for the same cameras
                per, st_a, amodal_cap[id(r)] = r.amodal_spans_host(
                    make_frames(*cur[0], sets, fb), capacity=amodal_cap.get(id(r), 0), eligible=amodal_el)
                arle[0] = (per, st_a)
                nb += st_a.nbytes + sum(o.nbytes + sp.nbytes for o, sp in per)
            return nb

        bopr = [None]  # the batch's per-frame (listed objects, mask_visib files, mask files, amodal stats), with "bop"

        def bop_of_batch() -> int:
            ids, nf = r.last_instance()
            if not ids or nf != len(fb):
                raise RuntimeError(f"bop: the batch kept {nf} id images, {len(fb)} frames rendered")
            bopr[0], nb = bop_masks[id(r)](make_frames(*cur[0], sets, fb), ids)
            return nb

        jpgr = [None]  # the batch's .jpg files, with "rgb_jpg" or bop's jpg RGB in thread mode

        def jpgs_of_batch() -> int:
            rgb, nf = r.last_rgb()
            if not rgb or nf != len(fb):
                raise RuntimeError(f"rgb_jpg: the batch kept {nf} RGB images, {len(fb)} frames rendered")
            jpgr[0] = r.jpegs_host(len(fb), rgb=rgb, quality=jpeg_quality, subsampling=jpeg_subsampling,
                                   out_capacity=jpg_cap.get(id(r), 0), views=True)
            nb = sum(len(j) for j in jpgr[0])
            jpg_cap[id(r)] = nb + nb // 4
            return nb

        voxr = [None]  # the batch's (voxels_%06d.ply file, records) per frame, with "pointcloud_voxel_ply"

        def voxels_of_batch() -> int:
            (pts, n0), (ids, n1), (rgb, n2) = r.last_points(), r.last_instance(), r.last_rgb()
            if not pts or not ids or not rgb or {n0, n1, n2} != {len(fb)}:
                raise RuntimeError(f"pointcloud_voxel_ply: the batch kept {n0} point, {n1} id and {n2} RGB images, "
                                   f"{len(fb)} frames rendered")
            recs, vox_cap[id(r)], _ = r.voxel_cloud_host(len(fb), voxel_size, points=pts, rgb=rgb, instance=ids,
                                                         capacity=vox_cap.get(id(r), int(voxel_capacity)),
                                                         keep=int(voxel_points), keep_seed=int(voxel_points_seed),
                                                         frame_keys=np.asarray(fb, np.uint32))
            voxr[0] = [(voxel_cloud.ply_bytes(x), len(x)) for x in recs]
            return sum(x.nbytes for x in recs)

        sensr = [None]  # the batch's (sensor16_%06d.png file, pixels per cause) per frame, with "depth_sensor16_png"

        def sensor_of_batch() -> int:
            import torch
            dep, nf = r.last_depth()
            if not dep or nf != len(fb):
                raise RuntimeError(f"depth_sensor16_png: the batch kept {nf} depth images, {len(fb)} frames rendered")
            n, dev = len(fb), torch.device("cuda", r.device)
            if id(r) not in sens_buf:   # the renderer's device arrays, made once for a full batch
                sens_buf[id(r)] = (torch.empty((batch, 4), dtype=torch.float32, device=dev),
                                   torch.empty((batch,), dtype=torch.int32, device=dev),
                                   torch.empty((batch, wl.height, wl.width), dtype=torch.float32, device=dev),
                                   torch.empty((batch, 7), dtype=torch.int32, device=dev))
            d_in, d_keys, d_out, d_cnt = sens_buf[id(r)]
            d_in[:n].copy_(torch.from_numpy(intrinsics_rows(make_frames(*cur[0], sets, fb))))
            d_keys[:n].copy_(torch.from_numpy(np.asarray(fb, np.uint32).view(np.int32).copy()))   # the frame ids
            torch.cuda.current_stream(dev).synchronize()   # the uploads, before the context's stream reads them
            # on the context's stream, behind the render and in front of the encoder, which waits for both
            r.sensor_depth(n, depth=dep, intrinsics=d_in.data_ptr(), model=sens_job, frame_keys=d_keys.data_ptr(),
                           sensor_depth=d_out.data_ptr(), sensor_count=d_cnt.data_ptr())
            buf = np.empty(sens_cap.get(id(r), n * (2 * wl.width * wl.height + 4096)), np.uint8)
            offsets, need = r.encode_files(n, wl.width, wl.height, ("depth16_png",), buf, depth=d_out.data_ptr(),
                                           depth16_counts_per_metre=depth16_counts_per_metre)
            if offsets is None:   # the files did not fit: a larger buffer, no second pass
                buf = np.empty(need + need // 4, np.uint8)
                offsets = r.copy_files(buf, n)
            sens_cap[id(r)] = max(sens_cap.get(id(r), 0), need + need // 4)
            cnt = d_cnt[:n].cpu().numpy().view(np.uint32)   # (the encoder has waited for the pass)
            sensr[0] = [(buf[int(offsets[k]):int(offsets[k + 1])].tobytes(), cnt[k].astype(np.int64)) for k in range(n)]
            return int(offsets[-1]) + cnt.nbytes

        lensr = [None]  # the batch's per-frame lens files and annotation inputs, with "lens"

        def lens_of_batch(out) -> int:
            import torch
            (rgb, n0), (ids, n1), (dep, n2) = r.last_rgb(), r.last_instance(), r.last_depth()
            if not rgb or not ids or not dep or {n0, n1, n2} != {len(fb)}:
                raise RuntimeError(f"lens: the batch kept {n0} RGB, {n1} id and {n2} depth images, {len(fb)} frames rendered")
            n, dev, LW, LH, nl = len(fb), torch.device("cuda", r.device), lens_m.width, lens_m.height, r.n_labels
            if id(r) not in lens_buf:   # the renderer's device arrays, made once for a full batch
                lens_buf[id(r)] = (torch.empty((batch, LH, LW, 3), dtype=torch.uint8, device=dev),
                                   torch.empty((batch, LH, LW), dtype=torch.int32, device=dev),
                                   torch.empty((batch, LH, LW), dtype=torch.float32, device=dev),
                                   torch.empty((batch, nl, 5), dtype=torch.int32, device=dev),
                                   torch.empty((batch, 3), dtype=torch.int32, device=dev))
            d_rgb, d_ids, d_dep, d_st, d_cnt = lens_buf[id(r)]
            d_map = r.lens_map(lens_m, lens_host_map)
            have_kp = "keypoints_uv" in out
            if have_kp:
                K = out["keypoints_uv"].shape[1]
                d_uv = torch.from_numpy(np.ascontiguousarray(out["keypoints_uv"][:n])).to(dev)
                d_vis = torch.from_numpy(np.ascontiguousarray(out["keypoints_vis"][:n])).to(dev)
                o_uv, o_vis = torch.empty_like(d_uv), torch.empty_like(d_vis)
            torch.cuda.current_stream(dev).synchronize()   # the uploads, before the context's stream reads them
            # on the context's stream, behind the render and in front of the encoder, which waits for both
            r.lens_remap(n, map=d_map.data_ptr(), width=LW, height=LH, rgb=rgb, instance=ids, depth=dep,
                         lens_rgb=d_rgb.data_ptr(), lens_instance=d_ids.data_ptr(), lens_depth=d_dep.data_ptr(),
                         lens_stats=d_st.data_ptr(), lens_count=d_cnt.data_ptr())
            if have_kp:
                r.lens_points(n, lens_m, n_keypoints=K, keypoints_uv=d_uv.data_ptr(), keypoints_vis=d_vis.data_ptr(),
                              lens_uv=o_uv.data_ptr(), lens_vis=o_vis.data_ptr())
            buf = np.empty(lens_cap.get(id(r), n * (5 * LW * LH + 8192)), np.uint8)
            offsets, need = r.encode_files(n, LW, LH, ("rgb_png", "depth16_png"), buf, rgb=d_rgb.data_ptr(),
                                           depth=d_dep.data_ptr(), depth16_counts_per_metre=depth16_counts_per_metre)
            if offsets is None:   # the files did not fit: a larger buffer, no second pass
                buf = np.empty(need + need // 4, np.uint8)
                offsets = r.copy_files(buf, 2 * n)
            lens_cap[id(r)] = max(lens_cap.get(id(r), 0), need + need // 4)
            spans, lens_span_cap[id(r)] = r.mask_spans_host(n, d_ids.data_ptr(), capacity=lens_span_cap.get(id(r), 0),
                                                            height=LH, width=LW)
            st = d_st[:n].cpu().numpy().view(np.uint32)   # (the encoder has waited for the passes)
            cnt = d_cnt[:n].cpu().numpy().view(np.uint32)
            uv, vis = (o_uv.cpu().numpy(), o_vis.cpu().numpy()) if have_kp else (None, None)
            lensr[0] = [dict(rgb=buf[int(offsets[2 * k]):int(offsets[2 * k + 1])].tobytes(),
                             depth=buf[int(offsets[2 * k + 1]):int(offsets[2 * k + 2])].tobytes(), spans=spans[k],
                             stats=st[k].copy(), count=cnt[k].astype(np.int64),
                             uv=uv[k] if have_kp else None, vis=vis[k] if have_kp else None) for k in range(n)]
            return int(offsets[-1]) + st.nbytes + cnt.nbytes + sum(o.nbytes + sp.nbytes for o, sp in spans)

        cur = [None]   # the cameras of the attempt being rendered

        def run(views, projs):
            cur[0] = (views, projs)
            fr = make_frames(views, projs, sets, fb)
            if kinds:
                outs_b = {k: v[:len(fb)] for k, v in arrays.items() if k not in ("files", "file_offsets")}
                out, offsets, need = r.render_files(fr, kinds, arrays["files"], want=want, out=outs_b,
                                                    depth16_counts_per_metre=depth16_counts_per_metre)
                if offsets is None:   # the files did not fit: a larger buffer, no re-render
                    offsets = r.copy_files(pool.grow_files(slot, need + need // 4, alloc=r.host_buffer,
                                                           free=r.free_host_buffer), len(fb) * nk)
                arrays["file_offsets"] = offsets
                d2h.append(int(offsets[-1]) + wire_bytes(out) + (spans_of_batch() if want_rle else 0)
                           + (bop_of_batch() if want_bop else 0) + (jpgs_of_batch() if want_jpg else 0)
                           + (voxels_of_batch() if want_vox else 0) + (sensor_of_batch() if want_sens else 0)
                           + (lens_of_batch(out) if want_lens else 0))
            else:
                out = r.render(fr, want=want, out={k: v[:len(fb)] for k, v in arrays.items()})
                d2h.append(wire_bytes(out) + (spans_of_batch() if want_rle else 0)
                           + (jpgs_of_batch() if want_jpg and gpu_files else 0)
                           + (voxels_of_batch() if want_vox else 0) + (sensor_of_batch() if want_sens else 0))
            return out

        out = run(views, projs)
        attempts, checks, failed = [0] * len(fb), [[] for _ in fb], [False] * len(fb)
        if validate_pointcloud:   # GDP:1573-1645: retry frames whose point cloud is too small
            check = range(len(fb))
            while True:
                pts = out["depth_stats"][:len(fb), 0]
                again = []
                for k in check:
                    if pts[k] >= min_points:
                        continue
                    checks[k].append(int(pts[k]))
                    if attempts[k] + 1 < max_retries:
                        attempts[k] += 1
                        again.append(k)
                    else:
                        failed[k] = True
                if not again:
                    break
                # the whole batch again, the retried frames from their jittered cameras (the
                # others render exactly as before: every frame is a pure function of its pose)
                out = run(*wl.frame_params(fb, attempts))
                check = again
        te = time.time()
        return fb, slot, out, (te - tr, tp - tw, tr - tp), attempts, checks, failed, (rle[0], arle[0], bopr[0], jpgr[0], voxr[0], sensr[0], lensr[0])

    ahead = ThreadPoolExecutor(max_workers=n_rend)
    prep = ThreadPoolExecutor(max_workers=max(1, n_prep))
    prep_f: List = []
    kPrepAhead = 3

    def prep_until(b: int) -> None:
        while len(prep_f) < min(b, len(starts)):
            prep_f.append(prep.submit(prepare, len(prep_f)))

    try:
        prep_until(kPrepAhead + n_rend)
        queued = [ahead.submit(render_batch, b) for b in range(min(n_rend, len(starts)))]
        for b in range(len(starts)):
            tq = time.time()
            fb, slot, out, (dt, dwait, dprep), attempts, checks, failed, (rle, arle, bopr, jpgr, voxr, sensr, lensr) = queued.pop(0).result()
            t_main_wait += time.time() - tq
            t_render += dt
            t_slot_wait += dwait
            t_prep += dprep
            tl = time.time()
            prep_until(b + n_rend + kPrepAhead + 1)
            if b + n_rend < len(starts):   # (renderer b % n_rend is free again)
                queued.append(ahead.submit(render_batch, b + n_rend))
            for e in sorted({f // 10 for f in fb}):
                if e not in pose_cache:
                    pose_cache[e] = object_poses(wl.scene, wl.epoch(e).object_frames)
            for k, f in enumerate(fb):
                if failed[k]:   # every validation attempt failed: logged, nothing written (GDP:1662-1666)
                    log.frame_failed(f, wl.camera(f)[3], checks[k])
                    continue
                V, P, C, cam, aim, q = wl.camera(f, attempts[k])
                listed = (in_frustum(wl.scene, wl.epoch(f // 10).object_frames, V, P, wl.width, wl.height,
                                     intr.near, intr.far) if object_list == "frustum" else None)
                if lw is not None:
                    ep = lw.epoch(f // 10, pose_cache[f // 10])
                    lab = partial(lw.write, frame_id=f, camera_pose=cm.get_obj_pose_from_matrix(C), ep=ep,
                                  inst_stats=out["inst_stats"][k], covered=cov_of(out, k),
                                  kp_uv=out["keypoints_uv"][k], kp_vis=out["keypoints_vis"][k], listed=listed)
                    n_obj = lw.n_visible(ep, out["inst_stats"][k], listed)
                else:
                    lab = label_record(f, cm.get_obj_pose_from_matrix(C), intr.params(), pose_cache[f // 10],
                                       out["inst_stats"][k], out["keypoints_uv"][k], out["keypoints_vis"][k],
                                       wl.kp_table, wl.height, wl.width, covered=cov_of(out, k),
                                       listed=listed)
                    n_obj = lab["num_objects"]
                log_args = dict(n_objects=n_obj, kp_vis=out["keypoints_vis"][k].copy(), frame_id=f,
                                cam_pos=wl.camera(f)[3] if attempts[k] else cam, failed_checks=checks[k],
                                depth_range=out["depth_range"][k].copy() if "depth_range" in out else None)
                if "depth_stats" in out:   # valid, zero, inf, sum, min, max (csg_outputs.depth_stats)
                    v = out["depth_stats"][k].tolist()
                    log_args["gpu_depth_stats"] = {"valid": int(v[0]), "zero": int(v[1]), "inf": int(v[2]),
                                                   "total": wl.width * wl.height, "sum": v[3], "min": v[4],
                                                   "max": v[5]}
                files = []
                if kinds:   # GPU-encoded: file j = frame * nk + index of its kind
                    for o, kd in FILE_OF_OUTPUT:
                        if o in outs:
                            files.append((file_path(out_dir, o, f), _ENCODED_KIND.get(o, "encoded"),
                                          (k * nk + kinds.index(kd),)))
                elif "rgb" in outs:
                    files.append((file_path(out_dir, "rgb", f), "png", ("rgb",)))
                if "rgb_jpg" in outs:   # made on the GPU behind the batch, or by the writer from the host RGB
                    files.append((file_path(out_dir, "rgb_jpg", f), "call",
                                  (partial(bop.write_bytes, data=jpgr[k]) if gpu_files else
                                   partial(write_jpeg, rgb=out["rgb"][k].copy(), quality=jpeg_quality,
                                           subsampling=jpeg_subsampling),)))
                if want_vox:   # made on the GPU behind the batch
                    files.append((file_path(out_dir, "pointcloud_voxel_ply", f), "call",
                                  (partial(bop.write_bytes, data=voxr[k][0]),)))
                    vox_stats["frames"] += 1
                    vox_stats["voxels"] += voxr[k][1]
                    vox_stats["voxels_max"] = max(vox_stats["voxels_max"], voxr[k][1])
                if want_sens:   # made on the GPU behind the batch
                    files.append((file_path(out_dir, "depth_sensor16_png", f), "call",
                                  (partial(bop.write_bytes, data=sensr[k][0]),)))
                    sens_counts += sensr[k][1]
                if want_lens:   # made on the GPU behind the batch; the annotations from the lens frame's own arrays
                    lf = lensr[k]
                    files.append((os.path.join(out_dir, "lens", f"rgb_{f:06d}.png"), "call",
                                  (partial(bop.write_bytes, data=lf["rgb"]),)))
                    files.append((os.path.join(out_dir, "lens", f"depth16_{f:06d}.png"), "call",
                                  (partial(bop.write_bytes, data=lf["depth"]),)))
                    files.append((os.path.join(out_dir, "lens", f"coco_{f:06d}.json"), "call",
                                  (partial(_write_lens_fragment, frame_id=f, height=lens_m.height, width=lens_m.width,
                                           poses=pose_cache[f // 10], inst_stats=lf["stats"], spans=lf["spans"][1],
                                           offsets=lf["spans"][0], kp_by_obj=kp_by_obj, kp_uv=lf["uv"],
                                           kp_vis=lf["vis"]),)))
                    lens_counts += lf["count"]
                if want_bop:   # the two images from the GPU encoders, the mask files, then the fragment
                    if f // bop.FRAMES_PER_SCENE not in bop_scenes and sink == "disk":
                        bop.make_dirs(out_dir, f // bop.FRAMES_PER_SCENE)
                        bop_scenes.add(f // bop.FRAMES_PER_SCENE)
                    if bop_jpg:
                        files.append((bop.image_path(out_dir, "rgb", f, "jpg"), "call",
                                      (partial(bop.write_bytes, data=jpgr[k]),)))
                    else:
                        files.append((bop.image_path(out_dir, "rgb", f), "encoded",
                                      (k * nk + kinds.index("rgb_png"),)))
                    files.append((bop.image_path(out_dir, "depth", f), "encoded",
                                  (k * nk + kinds.index("depth16_png"),)))
                    listed, vis_png, amo_png, a_stats = bopr[k]
                    for g in range(len(listed)):
                        files.append((bop.mask_path(out_dir, "mask_visib", f, g), "call",
                                      (partial(bop.write_bytes, data=vis_png[g]),)))
                        files.append((bop.mask_path(out_dir, "mask", f, g), "call",
                                      (partial(bop.write_bytes, data=amo_png[g]),)))
                    if f // 10 not in bop_em:
                        if len(bop_em) >= 256:
                            bop_em.pop(next(iter(bop_em)))
                        bop_em[f // 10] = bop.epoch_models(wl.epoch(f // 10).object_frames)
                    files.append((bop.fragment_path(out_dir, f), "call",
                                  (partial(bop.write_fragment, frame_id=f, view=V, proj=P,
                                           counts_per_metre=depth16_counts_per_metre, scene=wl.scene,
                                           em=bop_em[f // 10], inst_stats=out["inst_stats"][k].copy(),
                                           amodal_stats=a_stats, listed=listed),)))
                if "mask" in outs:
                    files.append((os.path.join(out_dir, "labels", f"instance_mask_{f:06d}.npy"), "npy", ("instance",)))
                if want_rle:   # written by the job itself, before the label file
                    kp_k = {"kp_uv": out["keypoints_uv"][k] if "keypoints_uv" in out else None,
                            "kp_vis": out["keypoints_vis"][k] if "keypoints_vis" in out else None}
                    if arle is not None:   # the frame's amodal spans, offsets and stats
                        kp_k.update(amodal_spans=arle[0][k][1], amodal_offsets=arle[0][k][0], amodal_stats=arle[1][k])
                    if gpu_files:   # natively, without the GIL
                        if fw is None:
                            fw = FragmentWriter(pose_cache[f // 10], wl.kp_table, wl.height, wl.width)
                        job = partial(fw.write, frame_id=f, inst_stats=out["inst_stats"][k], spans=rle[k][1],
                                      offsets=rle[k][0], **kp_k)
                    else:           # writer processes: the same bytes from masks.coco_fragment (picklable)
                        job = partial(masks.write_fragment, frame_id=f, height=wl.height, width=wl.width,
                                      poses=pose_cache[f // 10], inst_stats=out["inst_stats"][k].copy(),
                                      spans=rle[k][1], offsets=rle[k][0], kp_by_obj=kp_by_obj,
                                      **{n: (v.copy() if v is not None else None) for n, v in kp_k.items()})
                    files.append((masks.fragment_path(out_dir, f), "call", (job,)))
                if "depth_npy" in outs:
                    files.append((os.path.join(out_dir, "depth", f"depth_{f:06d}.npy"), "npy", ("depth",)))
                if "depth_csv" in outs and not kinds:
                    files.append((file_path(out_dir, "depth_csv", f), "csv", ("depth",)))
                if "depth_png" in outs and not kinds:
                    files.append((file_path(out_dir, "depth_png", f), "png", ("depth_vis",)))
                if "pointcloud" in outs and not kinds:
                    files.append((file_path(out_dir, "pointcloud", f), "pointcloud", ("points", "rgb")))
                if "pointcloud_ply" in outs and not kinds:
                    files.append((file_path(out_dir, "pointcloud_ply", f), "ply", ("points", "rgb")))
                if "depth16_png" in outs and not kinds:
                    files.append((file_path(out_dir, "depth16_png", f), "depth16", ("depth",),
                                  float(depth16_counts_per_metre)))
                if "normals" in outs:
                    files.append((os.path.join(out_dir, "normals", f"normals_{f:06d}.npy"), "npy", ("normals",)))
                if "obj_coords" in outs:
                    files.append((os.path.join(out_dir, "obj_coords", f"obj_coords_{f:06d}.npy"), "npy",
                                  ("obj_coords",)))
                fut = pool.submit(slot, k, files, lab, os.path.join(out_dir, "labels", f"label_{f:06d}.json"))
                pending.append((fut, log_args))
            del out
            t_labels += time.time() - tl
            # log frames in order as they complete
            while pending and pending[0][0].done():
                _log_done(log, *pending.pop(0), has_points)
        for p in pending:
            _log_done(log, *p, has_points)
        t_done = time.time()   # every file written (teardown below: freeing page-locked buffers)
    finally:
        ahead.shutdown(wait=True)
        prep.shutdown(wait=True)
        if ppool is not None:
            ppool.shutdown(wait=True, cancel_futures=True)
        pool.close()
        t_close = time.time()
        for x in rends:
            x.close()
    wall = t_done - t0
    t_teardown = time.time() - t_close
    log.save()
    summary = log.summary()
    summary["throughput"] = {"frames": len(frames), "wall_s": round(wall, 3), "render_s": round(t_render, 3),
                             "render_thread": {"render_s": round(t_render, 3), "slot_wait_s": round(t_slot_wait, 3),
                                               "epoch_prep_s": round(t_prep, 3)},
                             "main_thread": {"wait_render_s": round(t_main_wait, 3), "labels_s": round(t_labels, 3)},
                             "frames_per_s": round(len(frames) / wall, 2) if wall > 0 else None,
                             "writers": n_writers, "writer_mode": writer_mode, "renderers": n_rend,
                             "writer_task_s": round(pool.task_s, 3), "teardown_s": round(t_teardown, 3),
                             "d2h_bytes": int(sum(d2h)), "d2h_bytes_per_frame": round(sum(d2h) / max(len(frames), 1)),
                             "d2h_gbs": round(sum(d2h) / wall / 1e9, 2) if wall > 0 else None,
                             "ids_wire_bytes": ids_wire,
                             "render_busy": round(t_render / (wall * n_rend), 3) if wall > 0 else None,
                             "sink": sink, "prep_workers": n_prep,
                             "writer_busy": round(pool.task_s / (wall * n_writers), 3) if wall > 0 else None,
                             "outputs": sorted(outs)}
    if want_sens:
        meta = {"model": sens_model.as_dict(), "job": sens_job, "seed": sens_job["seed"], "frame_key": "frame id",
                "counts_per_metre": float(depth16_counts_per_metre), "invalid": 0,
                "cause_names": list(depth_sensor.cause_names),
                "cause_totals": {name: int(sens_counts[c]) for c, name in enumerate(depth_sensor.cause_names)}}
        with open(os.path.join(out_dir, "depth", "sensor.json"), "w") as fh:
            json.dump(meta, fh, indent=2)
        summary["depth_sensor"] = meta
    if want_lens:
        meta = {"model": lens_m.as_dict(), "opencv": lens_m.opencv(),
                "pixel_convention": "model: pixel i covers [i, i + 1), centre i + 0.5; opencv: centre of pixel i at i",
                "map_sha256": lens.map_digest(lens_host_map), "counts_per_metre": float(depth16_counts_per_metre),
                "invalid": 0, "cause_names": list(lens.cause_names),
                "cause_totals": {name: int(lens_counts[c]) for c, name in enumerate(lens.cause_names)}}
        with open(os.path.join(out_dir, "lens", "lens.json"), "w") as fh:
            json.dump(meta, fh, indent=2)
        summary["lens"] = meta
    if want_vox:
        summary["voxel_cloud"] = {"voxel_size": float(np.float32(voxel_size)),
                                  "capacity": max(vox_cap.values()) if vox_cap else int(voxel_capacity),
                                  "voxels_per_frame": round(vox_stats["voxels"] / max(vox_stats["frames"], 1), 1),
                                  "voxels_max": vox_stats["voxels_max"], **vox_keep}
    return summary


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=41, help="total frames of the run (all shards)")
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--rank", type=int, default=int(os.environ.get("RANK", "0")))
    ap.add_argument("--world", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    ap.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--outputs", default="reference",
                    help=f"'reference' ({','.join(REFERENCE_OUTPUTS)}), 'all', or a comma list of {OUTPUTS + (BOP_OUTPUT, LENS_OUTPUT)}")
    ap.add_argument("--depth", action="store_true", help="add depth .npy")
    ap.add_argument("--depth-csv", action="store_true", help="add depth .npy and CSV")
    ap.add_argument("--pointcloud", action="store_true")
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--writers", type=int, default=0, help="writer processes (0: the CPUs this process may use)")
    ap.add_argument("--writer-mode", default="thread", choices=("thread", "process"))
    ap.add_argument("--renderers", type=int, default=0,
                    help="renderer contexts rendering alternate batches (0: 3 with writer threads, else 1)")
    ap.add_argument("--object-list", default="visible", choices=OBJECT_LISTS,
                    help="objects in each label file: with visible pixels, or also every one in the view frustum")
    ap.add_argument("--occlusion", action="store_true",
                    help="add occlusion_ratio per object to the label files (not in the reference's schema; "
                         "costs the unoccluded-coverage raster)")
    ap.add_argument("--no-resume", action="store_true")
    ap.add_argument("--sink", default="disk", choices=("disk", "discard"),
                    help="discard: the whole pipeline, every file written to /dev/null (steady-state measurement)")
    ap.add_argument("--validate-pointcloud", action="store_true",
                    help="re-render frames with fewer than --min-points points from a jittered camera "
                         "(the reference's enable_pointcloud_validation, off by default there too)")
    ap.add_argument("--min-points", type=int, default=100, help="point-cloud validation threshold (GDP:59)")
    ap.add_argument("--max-retries", type=int, default=5, help="validation attempts per frame (GDP:60)")
    ap.add_argument("--depth16-counts-per-metre", type=float, default=250.0,
                    help="scale of the depth16_png output (default 250: 4 mm steps, 262.1 m range)")
    ap.add_argument("--amodal-kinds", default=",".join(DYNAMIC_KINDS),
                    help="object kinds whose annotations get amodal masks with the amodal_rle output "
                         "(a comma list, or 'all' for every label)")
    ap.add_argument("--jpeg-quality", type=int, default=95, help="quality of the rgb_jpg output and of bop's jpg RGB")
    ap.add_argument("--jpeg-subsampling", default="420", choices=("444", "420"))
    ap.add_argument("--bop-rgb", default="png", choices=("png", "jpg"),
                    help="output bop: train_pbr/%%06d/rgb/%%06d.png, or .jpg (BOP's train_pbr convention)")
    ap.add_argument("--voxel-size", type=float, default=voxel_cloud.DEFAULT_VOXEL_SIZE,
                    help="side in metres of the world-fixed grid of the pointcloud_voxel_ply output")
    ap.add_argument("--voxel-capacity", type=int, default=0,
                    help=f"voxel records per frame the pass starts with (0: {voxel_cloud.DEFAULT_VOXEL_CAPACITY}; "
                         "doubled while a frame overflows, and kept)")
    ap.add_argument("--voxel-points", type=int, default=0,
                    help="keep at most this many records of each voxel cloud, chosen by farthest-point sampling on "
                         "the GPU and stored in that order (0: all; at most 16384)")
    ap.add_argument("--voxel-points-seed", type=int, default=0,
                    help="seed of the farthest-point start (a frame's key is its frame id)")
    ap.add_argument("--depth-sensor", default=None, metavar="PRESET", choices=sorted(depth_sensor.PRESETS),
                    help="stereo model of the depth_sensor16_png output (depth_sensor.PRESETS; default site)")
    ap.add_argument("--sensor-baseline", type=float, default=None,
                    help="baseline in metres of the stereo model (signed: the second camera's x), instead of the preset's")
    ap.add_argument("--sensor-noise-px", type=float, default=None,
                    help="standard deviation of the disparity noise in pixels, instead of the preset's")
    ap.add_argument("--sensor-seed", type=int, default=0, help="seed of the sensor noise (a frame's key is its frame id)")
    ap.add_argument("--lens", default=None, metavar="PRESET", choices=sorted(lens.PRESETS),
                    help="coefficients of the lens output (lens.PRESETS; default wide)")
    ap.add_argument("--lens-coeffs", default=None, metavar="k1,k2,p1,p2,k3[,k4,k5,k6]",
                    help="Brown-Conrady coefficients of the lens output in OpenCV's order, instead of a preset")
    ap.add_argument("--lens-size", default=None, metavar="WxH", help="frame size of the lens output (default the run's)")
    ap.add_argument("--prep-workers", type=int, default=-1,
                    help="processes preparing batches ahead (-1: two for runs of >= 20 batches)")
    a = ap.parse_args(argv)
    try:
        outputs = parse_outputs(a.outputs)
    except ValueError as e:
        ap.error(str(e))
    frames = shard_of_range(a.rank, a.world, a.frames)
    out = os.path.join(a.out, f"shard_{a.rank:02d}") if a.world > 1 else a.out
    summary = generate(out, frames, a.workload, a.seed, a.batch, a.device, a.depth, a.depth_csv, a.pointcloud,
                       a.width, a.height, writers=a.writers, resume=not a.no_resume, normals=a.normals,
                       outputs=outputs, writer_mode=a.writer_mode, renderers=a.renderers,
                       object_list=a.object_list, occlusion=a.occlusion, sink=a.sink,
                       validate_pointcloud=a.validate_pointcloud, min_points=a.min_points, max_retries=a.max_retries,
                       prep_workers=a.prep_workers, depth16_counts_per_metre=a.depth16_counts_per_metre,
                       amodal_kinds=tuple(x.strip() for x in a.amodal_kinds.split(",") if x.strip()),
                       jpeg_quality=a.jpeg_quality, jpeg_subsampling=a.jpeg_subsampling, bop_rgb=a.bop_rgb,
                       voxel_size=a.voxel_size, voxel_capacity=a.voxel_capacity, depth_sensor_preset=a.depth_sensor,
                       sensor_baseline=a.sensor_baseline, sensor_noise_px=a.sensor_noise_px, sensor_seed=a.sensor_seed,
                       voxel_points=a.voxel_points, voxel_points_seed=a.voxel_points_seed, lens_preset=a.lens,
                       lens_coeffs=[float(v) for v in a.lens_coeffs.split(",")] if a.lens_coeffs else None,
                       lens_size=[int(v) for v in a.lens_size.lower().split("x")] if a.lens_size else None)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
