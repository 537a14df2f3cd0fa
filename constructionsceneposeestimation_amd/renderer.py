"""Python front-end of the C-ABI: one :class:`Renderer` per GPU per process.

This is the object the reference's Camera + annotator graph collapses into:
``Camera(...)`` + ``camera.initialize()`` (generate_construction_data.py:1421,
:1451) become :class:`Renderer` construction, and each
``set_world_pose`` + ``next_update_async`` + ``get_rgba()`` / ``get_data()``
round trip (:1586-1595, :1669, :1681, :1916) becomes one row of a batched
:meth:`Renderer.render` call.  Everything numeric runs in libcsg.so on the
GPU; this module only marshals arrays.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import CsgError
from .camera_math import Intrinsics
from .crops import CROP_INFO_DTYPE, DYNAMIC_KINDS, crop_intrinsics, eligible_labels
from .labels import object_unit_transforms
from .object_points import intrinsics_rows
from .packing import PackedScene, light_constants, pack_scene
from .scene.model import Scene
from .voxel_cloud import DEFAULT_VOXEL_CAPACITY, DEFAULT_VOXEL_SIZE, RECORD_DTYPE
from .voxel_cloud import OVERFLOW as VOXEL_OVERFLOW

FRAME_DTYPE = np.dtype([("view", "<f4", 16), ("proj", "<f4", 16), ("xform_set", "<u4"), ("frame_id", "<u4"),
                        ("records_hint", "<u4"), ("bins_hint", "<u4")])
assert FRAME_DTYPE.itemsize == C.sizeof(_lib.Frame)

OUTPUT_KINDS = ("rgb", "instance", "depth", "keypoints", "stats", "normals", "points", "depth_vis", "depth_range",
                "covered", "depth_stats", "obj_coords")

# Span records per frame that Renderer.mask_spans_host starts with (it doubles on overflow).  C3 at
# 1080p has 27.8 thousand spans per frame on average, 53.7 thousand at the 99th percentile and 59.5
# thousand at most over 480 frames (profiles/mask_rle/cost.json; leaves that pass the alpha test are
# most of them): the largest count plus three eighths, 640 KiB of device memory per frame of a batch.
# Only the records in use are copied to the host.
DEFAULT_SPAN_CAPACITY = 81920
# ... and Renderer.amodal_spans_host: with every label of C3 at 1080p 30.3 thousand amodal spans per frame
# on average, 65.4 thousand at the 99th percentile and 73.0 thousand at most over 480 frames (the dynamic
# kinds alone: 1.6, 3.7 and 4.4 thousand; profiles/amodal_rle/cost.json); the same rule, 784 KiB per frame.
DEFAULT_AMODAL_SPAN_CAPACITY = 100352


def make_frames(views: np.ndarray, projs: np.ndarray, sets: Sequence[int], frame_ids: Sequence[int]) -> np.ndarray:
    n = len(frame_ids)
    fr = np.zeros(n, FRAME_DTYPE)
    fr["view"] = np.asarray(views, np.float64).reshape(n, 16).astype(np.float32)
    fr["proj"] = np.asarray(projs, np.float64).reshape(n, 16).astype(np.float32)
    fr["xform_set"] = np.asarray(sets, np.uint32)
    fr["frame_id"] = np.asarray(frame_ids, np.uint32)
    return fr


def _light_struct(light) -> "_lib.Light":
    amb, sun, d, sky = light_constants(light)
    L = _lib.Light()
    L.ambient[:] = [float(x) for x in amb]
    L.sun[:] = [float(x) for x in sun]
    L.sun_dir[:] = [float(x) for x in d]
    L.sky[:] = [int(x) for x in sky]
    return L


def scene_labels(scene: Scene) -> int:
    """Label-table length of a scene (the renderers' ``n_labels``)."""
    n = max([o.inst_idx for o in scene.objects] + [i.inst_idx for i in scene.instances] + [-1]) + 1
    return max(n, 1)


def output_spec(n: int, H: int, W: int, n_kp: int, n_labels: int, want: Iterable[str]) -> Dict[str, tuple]:
    """Host arrays a render of ``n`` frames fills for ``want``: name -> (shape, dtype)."""
    want = set(want)
    spec: Dict[str, tuple] = {}
    if "rgb" in want:
        spec["rgb"] = ((n, H, W, 3), np.uint8)
    if "instance" in want:
        spec["instance"] = ((n, H, W), np.int32)
    if "depth" in want:
        spec["depth"] = ((n, H, W), np.float32)
    if "keypoints" in want and n_kp:
        spec["keypoints_uv"] = ((n, n_kp, 2), np.float32)
        spec["keypoints_vis"] = ((n, n_kp), np.int32)
    if "stats" in want:
        spec["inst_stats"] = ((n, n_labels, 5), np.uint32)
    if "normals" in want:
        spec["normals"] = ((n, H, W, 3), np.float16)
    if "points" in want:
        spec["points"] = ((n, H, W, 3), np.float32)
    if "depth_vis" in want:   # the reference's JET depth PNG (GDP:1690-1709) and its min / max
        spec["depth_vis"] = ((n, H, W, 3), np.uint8)
    if "depth_vis" in want or "depth_range" in want:
        spec["depth_range"] = ((n, 2), np.float32)
    if "depth_stats" in want:   # the quality log's depth counts: valid, zero, inf, sum, min, max
        spec["depth_stats"] = ((n, 6), np.float64)
    if "covered" in want:     # unoccluded pixels per label (occlusionRatio)
        spec["label_covered"] = ((n, n_labels), np.uint32)
    if "obj_coords" in want:  # object coordinates (NOCS), 16 bits per axis (labels.decode_obj_coords)
        spec["obj_coords"] = ((n, H, W, 3), np.uint16)
    return spec


class Renderer:
    def __init__(self, scene: Scene, width: int, height: int, max_frames: int = 8, device: int = 0,
                 intrinsics: Optional[Intrinsics] = None, records_per_frame: int = 0, bins_per_frame: int = 0,
                 frames_per_launch: int = 0):
        self.lib = _lib.load()
        self.scene = scene
        self.width, self.height = int(width), int(height)
        self.max_frames = int(max_frames)
        self.device = int(device)
        self.intr = intrinsics or Intrinsics(self.width, self.height)
        cfg = _lib.Config(device, self.width, self.height, self.max_frames, self.intr.near, self.intr.far,
                          records_per_frame, bins_per_frame, frames_per_launch)
        ctx = C.c_void_p()
        rc = self.lib.csg_create(C.byref(cfg), C.byref(ctx))
        if rc != 0:
            raise CsgError(f"csg_create failed ({rc})")
        self.ctx = ctx
        self.packed: PackedScene = pack_scene(scene)
        self.n_inst = len(scene.instances)
        self.n_labels = max(self.packed.n_labels, 1)
        assert self.n_labels == scene_labels(scene)
        self._n_inst_labels = max(int(self.packed.inst_label.max(initial=-1)) + 1, 1)
        self.n_kp = 0
        self._pinned: List[C.c_void_p] = []
        self._upload()

    # -- lifecycle ------------------------------------------------------------
    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            msg = self.lib.csg_last_error(self.ctx).decode(errors="replace")
            raise CsgError(f"{what}: status {rc}: {msg}")

    def close(self) -> None:
        if getattr(self, "ctx", None):
            for p in getattr(self, "_pinned", []):
                self.lib.csg_host_free(self.ctx, p)
            self._pinned = []
            self.lib.csg_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- scene ---------------------------------------------------------------
    def _upload(self) -> None:
        p = self.packed
        keep = []
        meshes = (_lib.Mesh * len(self.scene.meshes))()
        for k, m in enumerate(self.scene.meshes):
            pos = np.ascontiguousarray(m.positions, np.float32)
            idx = np.ascontiguousarray(m.tris, np.uint32)
            keep += [pos, idx]
            has_uv = m.uvs.shape[0] > 0 and m.uv_tris.shape[0] == m.n_tris
            meshes[k].positions = pos.ctypes.data
            meshes[k].n_vertices = pos.shape[0]
            meshes[k].indices = idx.ctypes.data
            meshes[k].n_tris = idx.shape[0]
            if has_uv:
                uv = np.ascontiguousarray(m.uvs, np.float32)
                uvi = np.ascontiguousarray(m.uv_tris, np.uint32)
                keep += [uv, uvi]
                meshes[k].uvs, meshes[k].n_uvs, meshes[k].uv_indices = uv.ctypes.data, uv.shape[0], uvi.ctypes.data
            meshes[k].material = m.material
        mats = (_lib.Material * len(p.materials))()
        for k in range(len(p.materials)):
            mats[k].base_color[:] = [int(x) for x in p.materials[k]["base"]]
            mats[k].texture = int(p.materials[k]["texture"])
            mats[k].alpha_test = int(p.materials[k]["alpha_test"])
            mats[k].alpha_threshold = int(p.materials[k]["alpha_threshold"])
        inst = (_lib.Instance * self.n_inst)()
        for k in range(self.n_inst):
            inst[k].model[:] = [float(x) for x in p.inst_model[k]]
            inst[k].mesh = int(p.inst_mesh[k])
            inst[k].inst_idx = int(p.inst_label[k])
        self._check(self.lib.csg_upload_scene(self.ctx, meshes, len(self.scene.meshes), mats, len(p.materials), inst,
                                              self.n_inst), "upload_scene")
        for k, t in enumerate(self.scene.textures):
            a = np.ascontiguousarray(t.rgba, np.uint8)
            self._check(self.lib.csg_upload_texture(self.ctx, k, a.ctypes.data, a.shape[1], a.shape[0]),
                        "upload_texture")
        self._check(self.lib.csg_set_light(self.ctx, C.byref(_light_struct(self.scene.light))), "set_light")

    def set_dr_light(self, set_id: int, light) -> None:
        """Lighting of transform set ``set_id`` (a ``scene.model.Light``; C4 DR)."""
        self._check(self.lib.csg_set_dr_light(self.ctx, set_id, C.byref(_light_struct(light))), "set_dr_light")

    def set_dr_textures(self, set_id: int, texture_per_material) -> None:
        """Texture of each material for transform set ``set_id``: an index into
        ``scene.textures``, -1 for none, or ``_lib.KEEP_TEXTURE``."""
        t = np.ascontiguousarray(np.asarray(texture_per_material, np.int32))
        self._check(self.lib.csg_set_dr_textures(self.ctx, set_id, t.ctypes.data, t.shape[0]), "set_dr_textures")

    def set_instance_transforms(self, set_id: int, models: np.ndarray) -> None:
        m = np.ascontiguousarray(np.asarray(models, np.float64).reshape(-1, 16).astype(np.float32))
        self._check(self.lib.csg_set_instance_transforms(self.ctx, set_id, m.ctypes.data, m.shape[0]),
                    "set_instance_transforms")

    def set_keypoints(self, set_id: int, pts_world: np.ndarray) -> None:
        p = np.ascontiguousarray(np.asarray(pts_world, np.float64).reshape(-1, 3).astype(np.float32))
        self._check(self.lib.csg_set_keypoints(self.ctx, set_id, p.ctypes.data, p.shape[0]), "set_keypoints")
        self.n_kp = p.shape[0]

    def set_object_frames(self, set_id: int, object_frames) -> None:
        """Object frames of transform set ``set_id`` (``EpochState.object_frames``,
        per object of the scene) for the ``obj_coords`` output: uploads
        :func:`labels.object_unit_transforms`.  ``object_frames`` may also be
        that table itself, an (n, 3, 4) array with one matrix per label."""
        t = object_frames
        if not (isinstance(t, np.ndarray) and t.ndim == 3 and t.shape[1:] == (3, 4)):
            # (the C ABI's label table spans the instances' labels)
            t = object_unit_transforms(self.scene, object_frames)[:self._n_inst_labels]
        elif t.shape[0] == self.n_labels:
            t = t[:self._n_inst_labels]
        t = np.ascontiguousarray(t, np.float32)
        self._check(self.lib.csg_set_object_frames(self.ctx, set_id, t.ctypes.data, t.shape[0]), "set_object_frames")

    # -- rendering ------------------------------------------------------------
    def output_spec(self, n: int, want: Iterable[str]) -> Dict[str, tuple]:
        """Host arrays :meth:`render` fills for ``want``: name -> (shape, dtype)."""
        return output_spec(n, self.height, self.width, self.n_kp, self.n_labels, want)

    def render(self, frames: np.ndarray, want: Iterable[str] = ("rgb", "instance", "depth"),
               out: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
        """Render a batch to host numpy arrays (synchronous; includes D2H copies).
        ``out`` supplies the arrays (e.g. views of shared memory), shaped as
        :meth:`output_spec` says; otherwise they are allocated."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        n = frames.shape[0]
        spec = self.output_spec(n, want)
        if out is None:
            out = {k: np.empty(shape, dt) for k, (shape, dt) in spec.items()}
        else:
            for k, (shape, dt) in spec.items():
                a = out.get(k)
                if a is None or a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                    raise CsgError(f"render: out[{k!r}] must be a C-contiguous {np.dtype(dt)} array of shape {shape}")
            out = {k: out[k] for k in spec}
        for s in range(0, n, self.max_frames):
            e = min(n, s + self.max_frames)
            oo = _lib.Outputs()
            for name, key in (("rgb", "rgb"), ("instance", "instance"), ("depth", "depth"),
                              ("keypoints_uv", "keypoints_uv"), ("keypoints_vis", "keypoints_vis"),
                              ("inst_stats", "inst_stats"), ("normals", "normals"), ("points", "points"),
                              ("depth_vis", "depth_vis"), ("depth_range", "depth_range"),
                              ("label_covered", "label_covered"), ("depth_stats", "depth_stats"),
                              ("obj_coords", "obj_coords")):
                arr = out.get(key)
                if arr is not None:
                    setattr(oo, name, arr[s:e].ctypes.data)
            oo.n_labels, oo.on_device = self.n_labels, 0
            self._check(self.lib.csg_render_batch(self.ctx, frames[s:e].ctypes.data, e - s, C.byref(oo)),
                        "render_batch")
        return out

    # -- files encoded on the GPU --------------------------------------------------
    def host_buffer(self, nbytes: int) -> np.ndarray:
        """A page-locked uint8 host array of ``nbytes`` (csg_host_alloc), freed
        with the renderer; D2H copies into it run at full PCIe rate."""
        p = C.c_void_p()
        self._check(self.lib.csg_host_alloc(self.ctx, int(nbytes), C.byref(p)), "host_alloc")
        buf = (C.c_uint8 * int(nbytes)).from_address(p.value)
        arr = np.frombuffer(buf, np.uint8)
        self._pinned.append(p)
        return arr

    def free_host_buffer(self, arr: np.ndarray) -> None:
        """Release a :meth:`host_buffer` array now (instead of with the
        renderer); the caller guarantees nothing reads it any more."""
        addr = arr.ctypes.data
        for k, p in enumerate(self._pinned):
            if p.value == addr:
                self._check(self.lib.csg_host_free(self.ctx, p), "host_free")
                del self._pinned[k]
                return
        raise CsgError("free_host_buffer: not a buffer of this renderer")

    def render_files(self, frames: np.ndarray, kinds: Sequence[str], files: np.ndarray,
                     want: Iterable[str] = (), out: Optional[Dict[str, np.ndarray]] = None,
                     depth16_counts_per_metre: float = 0.0):
        """Render a batch (at most ``max_frames``) and encode ``kinds`` (of
        ``_lib.FILE_KINDS``: "rgb_png", "depth_csv", "depth_png", "pointcloud_txt",
        "pointcloud_ply", "depth16_png") on the GPU.  ``depth16_counts_per_metre``
        is the scale of "depth16_png" (0: ``_lib.DEPTH16_COUNTS_PER_METRE``; the
        quantiser is ``writers.depth_to_u16``).  The files go
        into ``files`` (uint8 host array, pinned from :meth:`host_buffer` for
        speed), growing nothing: returns (outputs dict as :meth:`render`,
        offsets) with file j = frame * len(kinds) + k (kinds in bit order) at
        ``files[offsets[j]:offsets[j + 1]]``; ``None`` offsets' last entry
        says how many bytes were needed when ``files`` was too small (the
        files stay on the device: :meth:`copy_files`)."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        n = frames.shape[0]
        if n > self.max_frames:
            raise CsgError(f"render_files: {n} frames > max_frames {self.max_frames}")
        mask = 0
        for k in kinds:
            if k not in _lib.FILE_KINDS:
                raise CsgError(f"unknown file kind {k!r}; choose from {tuple(_lib.FILE_KINDS)}")
            mask |= _lib.FILE_KINDS[k]
        spec = self.output_spec(n, want)
        if out is None:
            out = {k: np.empty(shape, dt) for k, (shape, dt) in spec.items()}
        else:
            for k, (shape, dt) in spec.items():
                a = out.get(k)
                if a is None or a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                    raise CsgError(f"render_files: out[{k!r}] must be a C-contiguous {np.dtype(dt)} array of shape {shape}")
            out = {k: out[k] for k in spec}
        nk = bin(mask).count("1")
        offsets = np.zeros(n * nk + 1, np.uint64)
        if files.dtype != np.uint8 or not files.flags.c_contiguous:
            raise CsgError("render_files: files must be a C-contiguous uint8 array")
        oo = _lib.Outputs()
        for key in ("rgb", "instance", "depth", "keypoints_uv", "keypoints_vis", "inst_stats", "normals", "points",
                    "depth_vis", "depth_range", "label_covered", "depth_stats", "obj_coords"):
            arr = out.get(key)
            if arr is not None:
                setattr(oo, key, arr.ctypes.data)
        oo.n_labels, oo.on_device = self.n_labels, 0
        oo.file_kinds, oo.files, oo.files_cap, oo.file_offsets = mask, files.ctypes.data, files.nbytes, offsets.ctypes.data
        oo.depth16_counts_per_metre = float(depth16_counts_per_metre)
        rc = self.lib.csg_render_batch(self.ctx, frames.ctypes.data, n, C.byref(oo))
        if rc == _lib.ERR_CAPACITY:
            return out, None, int(offsets[-1])
        self._check(rc, "render_batch (files)")
        return out, offsets, int(offsets[-1])

    def copy_files(self, files: np.ndarray, n_files: int) -> np.ndarray:
        """The last :meth:`render_files` batch's files again (after the
        buffer was too small): returns the offsets."""
        offsets = np.zeros(n_files + 1, np.uint64)
        self._check(self.lib.csg_copy_files(self.ctx, files.ctypes.data, files.nbytes, offsets.ctypes.data),
                    "copy_files")
        return offsets

    def encode_files(self, n: int, width: int, height: int, kinds, files: Optional[np.ndarray], *, rgb: int = 0,
                     depth_vis: int = 0, depth: int = 0, points: int = 0, depth16_counts_per_metre: float = 0.0,
                     depth_stats: bool = False):
        """Encode ``kinds`` from device arrays the caller supplies
        (csg_encode_files; raw device pointers, e.g. torch ``data_ptr()``) of
        ``n`` frames of ``width`` x ``height`` -- any size, not the
        renderer's: ``rgb`` and ``depth_vis`` (n, H, W, 3) uint8 at any
        alignment, ``depth`` (n, H, W) and ``points`` (n, H, W, 3) float32.
        ``kinds`` are names of ``_lib.FILE_KINDS`` or a CSG_FILE_* bit mask.
        Synchronous, on the renderer's stream: the arrays must be complete.
        Returns ``(offsets, need)`` as :meth:`render_files` does (``None``
        offsets when ``files`` was too small: :meth:`copy_files`), and with
        ``depth_stats`` a third item, the (n, 6) float64 statistics."""
        if isinstance(kinds, (int, np.integer)):
            mask = int(kinds)
        else:
            mask = 0
            for k in kinds:
                if k not in _lib.FILE_KINDS:
                    raise CsgError(f"unknown file kind {k!r}; choose from {tuple(_lib.FILE_KINDS)}")
                mask |= _lib.FILE_KINDS[k]
        if files is None:
            files = np.zeros(0, np.uint8)
        if files.dtype != np.uint8 or not files.flags.c_contiguous:
            raise CsgError("encode_files: files must be a C-contiguous uint8 array")
        n = int(n)
        offsets = np.zeros(n * bin(mask).count("1") + 1, np.uint64)
        stats = np.zeros((n, 6), np.float64) if depth_stats else None
        job = _lib.EncodeJob(int(width), int(height), n, mask, rgb or None, depth_vis or None, depth or None,
                             points or None, float(depth16_counts_per_metre), files.ctypes.data if files.size else None,
                             files.nbytes, offsets.ctypes.data, stats.ctypes.data if depth_stats else None)
        rc = self.lib.csg_encode_files(self.ctx, C.byref(job))
        if rc != _lib.ERR_CAPACITY:
            self._check(rc, "encode_files")
        res = (None if rc else offsets, int(offsets[-1]))
        return res + (stats,) if depth_stats else res

    def render_into(self, frames_ptr: int, n: int, frames_on_device: bool, rgb: int = 0, instance: int = 0,
                    depth: int = 0, kp_uv: int = 0, kp_vis: int = 0, stats: int = 0, stream: int = 0,
                    normals: int = 0, points: int = 0, depth_vis: int = 0, depth_range: int = 0,
                    covered: int = 0, depth_stats: int = 0, obj_coords: int = 0) -> None:
        """Enqueue a batch writing device buffers (raw pointers, e.g. torch ``data_ptr()``)."""
        o = _lib.Outputs(rgb or None, instance or None, depth or None, kp_uv or None, kp_vis or None,
                         stats or None, self.n_labels, 1, normals or None, points or None, depth_vis or None,
                         depth_range or None, covered or None, 0, 0, None, 0, None, depth_stats or None,
                         obj_coords or None)
        self._check(self.lib.csg_render_batch_async(self.ctx, frames_ptr, n, int(frames_on_device), C.byref(o),
                                                    stream or None), "render_batch_async")

    # -- object crops -----------------------------------------------------------
    def crop_objects(self, n: int, *, size: int, per_frame: int, min_pixels: int = 64, pad: float = 1.5,
                     instance: int, rgb: int = 0, obj_coords: int = 0, depth: int = 0, stats: int = 0,
                     eligible: int = 0, crop_rgb: int = 0, crop_mask: int = 0, crop_coords: int = 0,
                     crop_depth: int = 0, info: int, explicit: bool = False, stream: int = 0,
                     n_labels: Optional[int] = None, rgb_filter: str = "bilinear") -> None:
        """Enqueue the crops of ``n`` frames (csg_crop_objects_filtered; raw device
        pointers, the counterpart of :meth:`render_into`): up to ``per_frame``
        windows per frame resampled to ``size`` x ``size`` from the arrays a
        render wrote (``instance`` always; ``rgb``, ``obj_coords``, ``depth``
        for the crop image that reads them) into ``crop_rgb`` (n, K, S, S, 3)
        uint8, ``crop_mask`` (n, K, S, S) uint8 255 / 0, ``crop_coords``
        (n, K, S, S, 3) uint16 and ``crop_depth`` (n, K, S, S) float32.  The
        windows are planned from ``stats`` (the render's ``inst_stats``) for
        the labels ``eligible`` allows (a uint8 table, 0 = all) and written to
        ``info`` (n, K) of ``crops.CROP_INFO_DTYPE``; with ``explicit`` they
        are read from ``info`` instead.  ``n_labels`` is the length of the
        label tables (default: the scene's).  ``rgb_filter`` is "bilinear", or
        "area" for an exact box filter over the footprint of every crop pixel
        of a minified window (more than one source pixel per crop pixel), which
        the bilinear taps alias.  On the stream of the render no
        synchronisation is needed in between."""
        if rgb_filter not in _lib.CROP_FILTERS:
            raise ValueError(f"crop_objects: rgb_filter {rgb_filter!r} is not one of {sorted(_lib.CROP_FILTERS)}")
        job = _lib.CropJob(int(size), int(per_frame), int(min_pixels), float(pad), int(bool(explicit)),
                           self.n_labels if n_labels is None else int(n_labels), rgb or None, instance or None,
                           obj_coords or None, depth or None, stats or None, eligible or None, crop_rgb or None,
                           crop_mask or None, crop_coords or None, crop_depth or None, info or None)
        self._check(self.lib.csg_crop_objects_filtered(self.ctx, C.byref(job), _lib.CROP_FILTERS[rgb_filter], int(n),
                                                       stream or None), "crop_objects")

    def crop_amodal(self, frames: np.ndarray, *, size: int, per_frame: int, info: int, crop_amodal: int,
                    stream: int = 0) -> None:
        """Enqueue the amodal masks of the crops of ``frames`` (csg_crop_amodal;
        raw device pointers, like :meth:`crop_objects`): for each slot of
        ``info`` (n, K) the samples of its window that the slot's object
        covers with every other object taken out of the scene, into
        ``crop_amodal`` (n, K, S, S) uint8 255 / 0.  ``frames`` are the HOST
        records (``FRAME_DTYPE``) the crops were cut from; they are copied
        before the call returns.  Behind :meth:`crop_objects` on the same
        stream no synchronisation is needed in between.  ``n`` is not bound
        by ``max_frames``."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        job = _lib.AmodalJob(int(size), int(per_frame), frames.ctypes.data, info or None, crop_amodal or None)
        self._check(self.lib.csg_crop_amodal(self.ctx, C.byref(job), int(frames.shape[0]), stream or None),
                    "crop_amodal")

    def crop_amodal_geometry(self, frames: np.ndarray, *, size: int, per_frame: int, info: int, crop_amodal: int = 0,
                             crop_amodal_depth: int = 0, crop_amodal_coords: int = 0, stream: int = 0) -> None:
        """Enqueue the amodal geometry of the crops of ``frames``
        (csg_crop_amodal_geometry; arguments as :meth:`crop_amodal`): the
        object's own depth and object coordinates over its whole silhouette,
        hidden parts included, into ``crop_amodal_depth`` (n, K, S, S) float32
        (+inf off the object) and ``crop_amodal_coords`` (n, K, S, S, 3) uint16
        (0 off the object; they need the object-frame tables of
        :meth:`set_object_frames`), and the amodal mask of :meth:`crop_amodal`
        into ``crop_amodal``.  Any of the three may be 0, not all.  Under
        ``crop_mask`` the two equal ``crop_depth`` and ``crop_coords``."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        job = _lib.AmodalGeometryJob(int(size), int(per_frame), frames.ctypes.data, info or None, crop_amodal or None,
                                     crop_amodal_depth or None, crop_amodal_coords or None)
        self._check(self.lib.csg_crop_amodal_geometry(self.ctx, C.byref(job), int(frames.shape[0]), stream or None),
                    "crop_amodal_geometry")

    def render_crops(self, frames: np.ndarray, size: int = 128, per_frame: int = 8, min_pixels: int = 64,
                     pad: float = 1.5, kinds: Sequence[str] = DYNAMIC_KINDS,
                     want: Iterable[str] = ("rgb", "mask", "coords"), object_frames=None,
                     rgb_filter: str = "bilinear", samples: int = 1024, seed: int = 0,
                     sampling: str = "stratified", candidates: int = 4096) -> Dict[str, np.ndarray]:
        """Render ``frames`` and deliver only their object crops to the host:
        chunks of ``max_frames`` are rendered into device tensors (torch),
        cropped on the same stream, and the crops and their ``info`` copied to
        page-locked host arrays; whole frames never cross PCIe.  ``want``
        chooses among "rgb", "mask", "coords", "depth", "amodal" (the
        unoccluded mask of :meth:`crop_amodal`, as ``crop_amodal`` (n, K, S, S)
        uint8, made behind the crops of each chunk), "amodal_depth" and
        "amodal_coords" (``crop_amodal_depth`` float32 and
        ``crop_amodal_coords`` uint16 of :meth:`crop_amodal_geometry`, one
        geometry pass per chunk, which also makes the amodal mask when that is
        wanted with them; the coordinates need the tables "coords" needs) and
        "points" (the point samples of :meth:`sample_points` for the planned
        slots: ``pt_count`` (n, K) uint32, ``pt_choose`` (n, K, N) uint32,
        ``pt_xyz`` (n, K, N, 3) float32, ``pt_rgb`` (n, K, N, 3) uint8 and
        ``pt_coords`` (n, K, N, 3) uint16 with N = ``samples``, drawn under
        ``seed`` with the frames' own ids as keys, so a frame's samples do not
        depend on its place in ``frames``; ``pt_coords`` needs the tables
        "coords" needs).  ``sampling`` = "fps" spreads the samples in 3D: each
        chunk draws ``candidates`` = Nc stratified samples per slot (a multiple
        of 4 in 16..16384) into device buffers and :meth:`farthest_points`
        reduces them to N <= 16384 on the same stream, under the keys
        ``frame_id * 64 + slot``; only the N chosen samples cross PCIe.  The
        samples then come in farthest-point order (every prefix is a run of its
        own), ``pt_count`` is unchanged, and two keys are added:
        ``pt_spread`` (n, K) uint32, the distinct samples ``t0`` of each slot
        (later ones repeat the run), and ``pt_radius2`` (n, K) float32, the
        squared distance at which the last of them was chosen (every candidate
        lies within it of a sample).  An empty slot reads as without it;
        ``kinds`` the object
        kinds that may be cropped (:func:`crops.eligible_labels`).  Returns
        ``crop_rgb`` / ``crop_mask`` / ``crop_coords`` / ``crop_depth`` (those
        wanted, shaped as :meth:`crop_objects` says), ``info`` (n, K) and
        ``intrinsics`` (n, K, 3, 3; :func:`crops.crop_intrinsics`).
        ``rgb_filter`` as in :meth:`crop_objects` ("area" anti-aliases the RGB
        of minified windows).

        "coords" crops the ``obj_coords`` output, which needs the object-frame
        table of every transform set the frames use (:meth:`set_object_frames`;
        without one the coordinates are 0).  ``object_frames`` = {set id:
        ``EpochState.object_frames``} uploads them first; otherwise nothing is
        uploaded here."""
        if rgb_filter not in _lib.CROP_FILTERS:
            raise ValueError(f"render_crops: rgb_filter {rgb_filter!r} is not one of {sorted(_lib.CROP_FILTERS)}")
        import torch
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        n, S, K, H, W = frames.shape[0], int(size), int(per_frame), self.height, self.width
        want = set(want)
        if not want or want - {"rgb", "mask", "coords", "depth", "amodal", "amodal_depth", "amodal_coords", "points"}:
            raise CsgError(f"render_crops: want {sorted(want)} must be a non-empty subset of rgb, mask, coords, depth, "
                           "amodal, amodal_depth, amodal_coords, points")
        pts, N = "points" in want, int(samples)
        if sampling not in ("stratified", "fps"):
            raise ValueError(f"render_crops: sampling {sampling!r} is not one of 'stratified', 'fps'")
        fps, Nc = pts and sampling == "fps", int(candidates)
        if fps and not (16 <= Nc <= 16384 and Nc % 4 == 0 and 1 <= N <= 16384):
            raise CsgError(f"render_crops: sampling='fps' needs candidates {Nc} a multiple of 4 in 16..16384 and "
                           f"samples {N} in 1..16384")
        for set_id, of in (object_frames or {}).items():
            self.set_object_frames(int(set_id), of)
        dev = torch.device("cuda", self.device)
        m = min(n, self.max_frames)

        def dbuf(cond, shape, dt):
            return torch.empty(shape, dtype=dt, device=dev) if cond else None

        def ptr(t):
            return t.data_ptr() if t is not None else 0

        src = {"rgb": dbuf(pts or "rgb" in want, (m, H, W, 3), torch.uint8),
               "instance": dbuf(True, (m, H, W), torch.int32),
               "depth": dbuf(pts or "depth" in want, (m, H, W), torch.float32),
               "obj_coords": dbuf(pts or "coords" in want, (m, H, W, 3), torch.int16),
               "stats": dbuf(True, (m, self.n_labels, 5), torch.int32)}
        shapes = {"crop_rgb": ("rgb", (K, S, S, 3), torch.uint8), "crop_mask": ("mask", (K, S, S), torch.uint8),
                  "crop_coords": ("coords", (K, S, S, 3), torch.int16), "crop_depth": ("depth", (K, S, S), torch.float32),
                  "crop_amodal": ("amodal", (K, S, S), torch.uint8),
                  "crop_amodal_depth": ("amodal_depth", (K, S, S), torch.float32),
                  "crop_amodal_coords": ("amodal_coords", (K, S, S, 3), torch.int16),
                  "info": (None, (K, CROP_INFO_DTYPE.itemsize), torch.uint8)}
        if pts:
            shapes.update({"pt_count": ("points", (K,), torch.int32), "pt_choose": ("points", (K, N), torch.int32),
                           "pt_xyz": ("points", (K, N, 3), torch.float32), "pt_rgb": ("points", (K, N, 3), torch.uint8),
                           "pt_coords": ("points", (K, N, 3), torch.int16)})
            intr = torch.from_numpy(intrinsics_rows(frames)).to(dev)
            keys = torch.from_numpy(np.ascontiguousarray(frames["frame_id"]).view(np.int32)).to(dev)
        if fps:
            shapes.update({"pt_spread": ("points", (K,), torch.int32), "pt_radius2": ("points", (K,), torch.float32)})
            cand = {"pt_choose": dbuf(True, (m, K, Nc), torch.int32), "pt_xyz": dbuf(True, (m, K, Nc, 3), torch.float32),
                    "pt_rgb": dbuf(True, (m, K, Nc, 3), torch.uint8), "pt_coords": dbuf(True, (m, K, Nc, 3), torch.int16)}
            fp_d2, fp_n = dbuf(True, (m, K, N), torch.float32), dbuf(True, (m, K, 2), torch.int32)
            set_keys = torch.from_numpy(((frames["frame_id"].astype(np.uint32)[:, None] * np.uint32(64)
                                          + np.arange(K, dtype=np.uint32)[None, :]).astype(np.uint32))
                                        .view(np.int32)).to(dev)
        d_out = {k: dbuf(w is None or w in want, (m,) + sh, dt) for k, (w, sh, dt) in shapes.items()}
        h_out = {k: torch.empty((n,) + sh, dtype=dt, pin_memory=True)
                 for k, (w, sh, dt) in shapes.items() if d_out[k] is not None}
        elig = torch.from_numpy(eligible_labels(self.scene, kinds)[:self.n_labels].copy()).to(dev)
        stream = torch.cuda.Stream(dev)   # (the null stream's handle 0 would mean "the context's own stream")
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            for s in range(0, n, self.max_frames):
                e = min(n, s + self.max_frames)
                self.render_into(frames[s:e].ctypes.data, e - s, False, rgb=ptr(src["rgb"]),
                                 instance=ptr(src["instance"]), depth=ptr(src["depth"]), stats=ptr(src["stats"]),
                                 obj_coords=ptr(src["obj_coords"]), stream=stream.cuda_stream)
                self.crop_objects(e - s, size=S, per_frame=K, min_pixels=min_pixels, pad=pad,
                                  instance=ptr(src["instance"]), rgb=ptr(src["rgb"]), obj_coords=ptr(src["obj_coords"]),
                                  depth=ptr(src["depth"]), stats=ptr(src["stats"]), eligible=elig.data_ptr(),
                                  crop_rgb=ptr(d_out["crop_rgb"]), crop_mask=ptr(d_out["crop_mask"]),
                                  crop_coords=ptr(d_out["crop_coords"]), crop_depth=ptr(d_out["crop_depth"]),
                                  info=ptr(d_out["info"]), stream=stream.cuda_stream, rgb_filter=rgb_filter)
                if want & {"amodal_depth", "amodal_coords"}:   # (makes the mask too when it is wanted)
                    self.crop_amodal_geometry(frames[s:e], size=S, per_frame=K, info=ptr(d_out["info"]),
                                              crop_amodal=ptr(d_out["crop_amodal"]),
                                              crop_amodal_depth=ptr(d_out["crop_amodal_depth"]),
                                              crop_amodal_coords=ptr(d_out["crop_amodal_coords"]),
                                              stream=stream.cuda_stream)
                elif "amodal" in want:
                    self.crop_amodal(frames[s:e], size=S, per_frame=K, info=ptr(d_out["info"]),
                                     crop_amodal=ptr(d_out["crop_amodal"]), stream=stream.cuda_stream)
                if fps:
                    self.sample_points(e - s, samples=Nc, per_frame=K, seed=seed, instance=ptr(src["instance"]),
                                       info=ptr(d_out["info"]), depth=ptr(src["depth"]),
                                       intrinsics=intr.data_ptr() + 16 * s, rgb=ptr(src["rgb"]),
                                       obj_coords=ptr(src["obj_coords"]), frame_keys=keys.data_ptr() + 4 * s,
                                       pt_count=ptr(d_out["pt_count"]), pt_choose=ptr(cand["pt_choose"]),
                                       pt_xyz=ptr(cand["pt_xyz"]), pt_rgb=ptr(cand["pt_rgb"]),
                                       pt_coords=ptr(cand["pt_coords"]), stream=stream.cuda_stream)
                    self.farthest_points((e - s) * K, rows=Nc, pool=Nc, samples=N, xyz=ptr(cand["pt_xyz"]),
                                         counts=ptr(d_out["pt_count"]), set_keys=set_keys.data_ptr() + 4 * K * s,
                                         seed=seed, fp_xyz=ptr(d_out["pt_xyz"]), fp_dist2=ptr(fp_d2), fp_count=ptr(fp_n),
                                         payloads=((ptr(cand["pt_choose"]), ptr(d_out["pt_choose"]), 4, 0xFF),
                                                   (ptr(cand["pt_rgb"]), ptr(d_out["pt_rgb"]), 3, 0),
                                                   (ptr(cand["pt_coords"]), ptr(d_out["pt_coords"]), 6, 0)),
                                         stream=stream.cuda_stream)
                    d_out["pt_spread"].copy_(fp_n[:, :, 0])
                    last = (fp_n[:, :, 0].long() - 1).clamp_(0, N - 1)   # (an empty slot: entry 0, which is 0.0)
                    d_out["pt_radius2"].copy_(torch.gather(fp_d2, 2, last[:, :, None])[:, :, 0])
                elif pts:
                    self.sample_points(e - s, samples=N, per_frame=K, seed=seed, instance=ptr(src["instance"]),
                                       info=ptr(d_out["info"]), depth=ptr(src["depth"]),
                                       intrinsics=intr.data_ptr() + 16 * s, rgb=ptr(src["rgb"]),
                                       obj_coords=ptr(src["obj_coords"]), frame_keys=keys.data_ptr() + 4 * s,
                                       pt_count=ptr(d_out["pt_count"]), pt_choose=ptr(d_out["pt_choose"]),
                                       pt_xyz=ptr(d_out["pt_xyz"]), pt_rgb=ptr(d_out["pt_rgb"]),
                                       pt_coords=ptr(d_out["pt_coords"]), stream=stream.cuda_stream)
                for k, h in h_out.items():
                    h[s:e].copy_(d_out[k][:e - s], non_blocking=True)
        stream.synchronize()
        self.synchronize()
        out = {k: h.numpy() for k, h in h_out.items()}
        for k in ("crop_coords", "crop_amodal_coords", "pt_coords"):
            if k in out:
                out[k] = out[k].view(np.uint16)
        for k in ("pt_count", "pt_choose", "pt_spread"):
            if k in out:
                out[k] = out[k].view(np.uint32)
        info = out["info"].view(CROP_INFO_DTYPE).reshape(n, K)
        # (the kernel numbers frames within a chunk: here they index `frames`)
        info["frame"] = np.where(info["label"] >= 0, np.arange(n, dtype=np.uint32)[:, None], np.uint32(0))
        out["info"] = info
        out["intrinsics"] = crop_intrinsics(self.intr, info, S)
        return out

    # -- per-object point samples ---------------------------------------------------
    def sample_points(self, n: int, *, samples: int, per_frame: int, instance: int, info: int, seed: int = 0,
                      depth: int = 0, intrinsics: int = 0, rgb: int = 0, obj_coords: int = 0, frame_keys: int = 0,
                      pt_count: int = 0, pt_choose: int = 0, pt_xyz: int = 0, pt_rgb: int = 0, pt_coords: int = 0,
                      n_labels: Optional[int] = None, height: Optional[int] = None, width: Optional[int] = None,
                      stream: int = 0) -> None:
        """Enqueue the point samples of ``n`` frames (csg_sample_object_points;
        raw device pointers, like :meth:`mask_spans`): for each slot of
        ``info`` (n, K) of ``crops.CROP_INFO_DTYPE`` (only ``label`` is read:
        what :meth:`crop_objects` planned, or the caller's own) ``samples`` = N
        pixels of the visible mask of the slot's label in ``instance``
        (n, H, W) int32, into ``pt_count`` (n, K) uint32 (the label's pixels
        M), ``pt_choose`` (n, K, N) uint32 (row-major indices ``y * W + x``),
        ``pt_xyz`` (n, K, N, 3) float32 (OpenCV camera frame, from ``depth``
        (n, H, W) float32 and ``intrinsics`` (n, 4) float32 ``fx, fy, cx, cy``:
        :func:`object_points.intrinsics_rows`), ``pt_rgb`` (n, K, N, 3) uint8
        (from ``rgb``) and ``pt_coords`` (n, K, N, 3) uint16 (from
        ``obj_coords``).  Any output may be 0, not all.  With M <= N every
        pixel is used and they repeat in order (``np.pad(..., 'wrap')``); with
        M > N one pixel per stratum of the label's row-major pixel list is
        drawn under ``seed``, the frame's key (``frame_keys`` (n,) uint32; 0:
        the frame's index) and the label, so samples ascend in pixel order (a
        CPU loader's random choice is unordered).  A slot without pixels gets
        0, 0xFFFFFFFF, NaN, 0 and 0.  ``n_labels`` defaults to the scene's,
        ``height`` / ``width`` to the renderer's.  On the stream of the render
        and the crops no synchronisation is needed in between."""
        job = _lib.PointJob(self.width if width is None else int(width), self.height if height is None else int(height),
                            self.n_labels if n_labels is None else int(n_labels), int(per_frame), int(samples),
                            int(seed) & 0xFFFFFFFF, instance or None, info or None, depth or None, intrinsics or None,
                            rgb or None, obj_coords or None, frame_keys or None, pt_count or None, pt_choose or None,
                            pt_xyz or None, pt_rgb or None, pt_coords or None)
        self._check(self.lib.csg_sample_object_points(self.ctx, C.byref(job), int(n), stream or None),
                    "sample_points")

    # -- per-object run-length masks ----------------------------------------------
    def mask_spans(self, n: int, *, instance: int, spans: int, span_offsets: int, capacity: int,
                   n_labels: Optional[int] = None, height: Optional[int] = None, width: Optional[int] = None,
                   stream: int = 0) -> None:
        """Enqueue the mask spans of ``n`` frames (csg_mask_spans; raw device
        pointers, like :meth:`crop_objects`): the vertical runs of every label
        of ``instance`` (n, H, W) int32 as (start = x * H + y0, len) records in
        ``spans`` (n, capacity, 2) uint32, ordered by label then start, and
        ``span_offsets`` (n, L + 1) uint32 (label l's records of frame f are
        ``[off[f, l], off[f, l + 1])``).  ``off[f, L]`` is the frame's total
        whether or not it fits: the call is asynchronous, so a caller reads it
        after the stream completes and, where it exceeds ``capacity`` (that
        frame's records are then unspecified), repeats the pass with a larger
        one.  ``n_labels`` defaults to the scene's, ``height`` / ``width`` to
        the renderer's.  On the stream of the render that wrote ``instance`` no
        synchronisation is needed in between."""
        job = _lib.SpanJob(self.width if width is None else int(width), self.height if height is None else int(height),
                           self.n_labels if n_labels is None else int(n_labels), int(capacity), instance or None,
                           spans or None, span_offsets or None)
        self._check(self.lib.csg_mask_spans(self.ctx, C.byref(job), int(n), stream or None), "mask_spans")

    def mask_spans_host(self, n: int, instance: int, *, capacity: int = 0, n_labels: Optional[int] = None,
                        height: Optional[int] = None, width: Optional[int] = None, stream: int = 0):
        """:meth:`mask_spans` of a device id image (pointer ``instance``),
        delivered to the host: returns ``(frames, capacity)`` where ``frames``
        is a list of ``n`` pairs ``(offsets (L + 1,) uint32, spans (total, 2)
        uint32)`` and ``capacity`` the per-frame capacity that was enough.  The
        pass starts at ``capacity`` (0: ``DEFAULT_SPAN_CAPACITY``) and is
        repeated with the capacity doubled (at least the largest total seen)
        until every frame fits.  Only the offsets and the records in use cross
        PCIe: the pass runs on a stream of the wrapper's own, the offsets
        follow it into page-locked memory, and the frames' records are packed
        on the device and copied once (two waits in all, however many frames).
        ``stream`` (a raw handle, 0: none) is the stream still writing
        ``instance``, if any: it is waited for first.  Synchronous."""
        import torch
        n = int(n)
        L = self.n_labels if n_labels is None else int(n_labels)
        cap = int(capacity) or DEFAULT_SPAN_CAPACITY
        dev = torch.device("cuda", self.device)
        if stream:
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        else:
            self.synchronize()
        if getattr(self, "_span_stream", None) is None:
            self._span_stream, self._span_pin = torch.cuda.Stream(dev), {}
        st = self._span_stream

        def pinned(name: str, count: int):   # a page-locked int32 staging tensor, grown by doubling and kept
            t = self._span_pin.get(name)
            if t is None or t.numel() < count:
                t = torch.empty(max(count, 2 * (t.numel() if t is not None else 0), 1024), dtype=torch.int32,
                                pin_memory=True)
                self._span_pin[name] = t
            return t[:count]

        with torch.cuda.stream(st):
            d_off = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
            h_off = pinned("offsets", n * (L + 1)).view(n, L + 1)
            while True:
                d_sp = torch.empty((n, cap, 2), dtype=torch.int32, device=dev)
                self.mask_spans(n, instance=instance, spans=d_sp.data_ptr(), span_offsets=d_off.data_ptr(),
                                capacity=cap, n_labels=L, height=height, width=width, stream=st.cuda_stream)
                h_off.copy_(d_off, non_blocking=True)
                st.synchronize()
                off = h_off.numpy().view(np.uint32).copy()
                top = int(off[:, L].max())
                if top <= cap:
                    break
                cap = max(2 * cap, top)
            totals = off[:, L].astype(np.int64)
            ends = np.cumsum(totals)
            packed = torch.cat([d_sp[f, :int(totals[f])] for f in range(n)])   # the records in use, and no more
            h_sp = pinned("spans", 2 * int(ends[-1])).view(int(ends[-1]), 2)
            h_sp.copy_(packed, non_blocking=True)
            st.synchronize()
            sp = h_sp.numpy().view(np.uint32).copy()
        return [(off[f], sp[int(ends[f] - totals[f]):int(ends[f])]) for f in range(n)], cap

    # -- full-frame amodal masks as spans ------------------------------------------
    def amodal_spans(self, frames: np.ndarray, *, spans: int, span_offsets: int, capacity: int, amodal_stats: int = 0,
                     eligible=None, stream: int = 0) -> None:
        """Enqueue the amodal mask spans of ``frames`` (csg_amodal_spans; raw
        device pointers, like :meth:`mask_spans`): for every label its full
        silhouette over the frame as if nothing stood in front of it -- the
        pixels some triangle of the label covers, with the depth range and the
        alpha test but no depth test -- as the records :meth:`mask_spans` makes
        of the visible ids: ``spans`` (n, capacity, 2) uint32 ordered by label
        then start, ``span_offsets`` (n, L + 1) uint32 with ``off[f, L]`` the
        frame's total whether or not it fits.  Spans of different labels may
        overlap.  ``amodal_stats`` (n, L, 5) uint32, or 0, gets each mask's
        pixel count and inclusive box (the layout of ``inst_stats``).
        ``frames`` are the HOST records of the frames (FRAME_DTYPE: view, proj
        and transform set are read), copied before the call returns;
        ``eligible`` an optional mask of the labels wanted (the others get no
        spans and empty stats).  L is the uploaded scene's label-table length,
        the largest instance label + 1 (``n_labels`` unless the scene lists
        objects without instances; a longer ``eligible`` is cut to it)."""
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        el = None
        if eligible is not None:
            el = np.ascontiguousarray(np.asarray(eligible).reshape(-1)[:self._n_inst_labels]).astype(np.uint8)
            if el.shape != (self._n_inst_labels,):
                raise ValueError(f"amodal_spans: eligible has {el.shape[0]} entries, the scene {self._n_inst_labels} labels")
        job = _lib.AmodalSpanJob(int(capacity), frames.ctypes.data, el.ctypes.data if el is not None else None,
                                 spans or None, span_offsets or None, amodal_stats or None)
        self._check(self.lib.csg_amodal_spans(self.ctx, C.byref(job), int(frames.shape[0]), stream or None),
                    "amodal_spans")

    def amodal_spans_host(self, frames: np.ndarray, *, capacity: int = 0, eligible=None):
        """:meth:`amodal_spans` delivered to the host: returns ``(frames, stats,
        capacity)`` where ``frames`` is a list of ``n`` pairs ``(offsets
        (L + 1,) uint32, spans (total, 2) uint32)``, ``stats`` the (n, L, 5)
        uint32 amodal pixel counts and boxes (L = ``n_labels`` here, the table
        length of ``inst_stats``), and ``capacity`` the per-frame
        capacity that was enough.  As :meth:`mask_spans_host`: the pass starts
        at ``capacity`` (0: ``DEFAULT_AMODAL_SPAN_CAPACITY``) and is repeated
        with the capacity doubled (at least the largest total seen) until every
        frame fits; offsets and stats follow the pass into page-locked memory, and
        the records in use are packed on the device and copied once.
        Synchronous."""
        import torch
        frames = np.ascontiguousarray(frames, FRAME_DTYPE)
        n, L = int(frames.shape[0]), self._n_inst_labels
        cap = int(capacity) or DEFAULT_AMODAL_SPAN_CAPACITY
        dev = torch.device("cuda", self.device)
        self.synchronize()
        if getattr(self, "_span_stream", None) is None:
            self._span_stream, self._span_pin = torch.cuda.Stream(dev), {}
        st = self._span_stream

        def pinned(name: str, count: int):   # a page-locked int32 staging tensor, grown by doubling and kept
            t = self._span_pin.get(name)
            if t is None or t.numel() < count:
                t = torch.empty(max(count, 2 * (t.numel() if t is not None else 0), 1024), dtype=torch.int32,
                                pin_memory=True)
                self._span_pin[name] = t
            return t[:count]

        with torch.cuda.stream(st):
            d_off = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
            d_st = torch.empty((n, L, 5), dtype=torch.int32, device=dev)
            h_off = pinned("offsets", n * (L + 1)).view(n, L + 1)
            h_st = pinned("amodal_stats", n * L * 5).view(n, L, 5)
            while True:
                d_sp = torch.empty((n, cap, 2), dtype=torch.int32, device=dev)
                self.amodal_spans(frames, spans=d_sp.data_ptr(), span_offsets=d_off.data_ptr(), capacity=cap,
                                  amodal_stats=d_st.data_ptr(), eligible=eligible, stream=st.cuda_stream)
                h_off.copy_(d_off, non_blocking=True)
                h_st.copy_(d_st, non_blocking=True)
                st.synchronize()
                off = h_off.numpy().view(np.uint32).copy()
                top = int(off[:, L].max())
                if top <= cap:
                    break
                cap = max(2 * cap, top)
            stats = h_st.numpy().view(np.uint32).copy()
            totals = off[:, L].astype(np.int64)
            if self.n_labels > L:   # labels without instances: no spans, empty stats, in inst_stats' table length
                off = np.concatenate([off, np.repeat(off[:, L:], self.n_labels - L, axis=1)], axis=1)
                pad = np.tile(np.array([0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0], np.uint32), (n, self.n_labels - L, 1))
                stats = np.concatenate([stats, pad], axis=1)
            ends = np.cumsum(totals)
            packed = torch.cat([d_sp[f, :int(totals[f])] for f in range(n)])   # the records in use, and no more
            h_sp = pinned("spans", 2 * int(ends[-1])).view(int(ends[-1]), 2)
            h_sp.copy_(packed, non_blocking=True)
            st.synchronize()
            sp = h_sp.numpy().view(np.uint32).copy()
        return [(off[f], sp[int(ends[f] - totals[f]):int(ends[f])]) for f in range(n)], stats, cap

    def span_stream(self):
        """The wrapper's own stream, on which the ``*_host`` span and mask methods run (made on first use)."""
        import torch
        if getattr(self, "_span_stream", None) is None:
            self._span_stream, self._span_pin = torch.cuda.Stream(torch.device("cuda", self.device)), {}
        return self._span_stream

    # -- per-object mask PNGs from spans ------------------------------------------------
    def encode_span_masks(self, items, *, spans: int, span_offsets: int, capacity: int, out: int, out_capacity: int,
                          file_offsets: int, n_frames: int, n_labels: Optional[int] = None,
                          height: Optional[int] = None, width: Optional[int] = None, stream: int = 0) -> None:
        """Enqueue the mask PNG files of ``items`` (csg_encode_span_masks; raw
        device pointers, like :meth:`mask_spans`): item i = ``(frame, label)``
        ((n_items, 2) uint32 on the HOST, copied before the call returns) is the
        union of that label's records of that frame in ``spans`` (n_frames,
        capacity, 2) / ``span_offsets`` (n_frames, L + 1) -- what
        :meth:`mask_spans` or :meth:`amodal_spans` wrote -- as a finished 8-bit
        grey PNG (0 / 255; :func:`writers.mask_png_bytes` states the bytes) at
        ``out + file_offsets[i]``.  ``file_offsets`` (n_items + 1) uint64 gets
        exact offsets whether or not the total ``file_offsets[n_items]`` fits
        ``out_capacity``; where it does not, ``out`` is unspecified and the
        caller repeats the pass with an output of that size.  ``n_labels``
        defaults to the scene's, ``height`` / ``width`` to the renderer's."""
        it = np.ascontiguousarray(np.asarray(items).reshape(-1, 2)).astype(np.uint32)
        job = _lib.MaskPngJob(self.width if width is None else int(width), self.height if height is None else int(height),
                              int(n_frames), self.n_labels if n_labels is None else int(n_labels), int(capacity),
                              int(it.shape[0]), spans or None, span_offsets or None,
                              it.ctypes.data if it.shape[0] else None, out or None, int(out_capacity),
                              file_offsets or None)
        self._check(self.lib.csg_encode_span_masks(self.ctx, C.byref(job), stream or None), "encode_span_masks")

    def mask_pngs_host(self, items, *, spans: int, span_offsets: int, capacity: int, n_frames: int,
                       n_labels: Optional[int] = None, height: Optional[int] = None, width: Optional[int] = None,
                       out_capacity: int = 0, stream: int = 0) -> List[bytes]:
        """:meth:`encode_span_masks` delivered to the host: the files of
        ``items`` as a list of ``bytes``.  The pass runs on a stream of the
        wrapper's own into an output of ``out_capacity`` bytes (0: a guess from
        the frame size), ``file_offsets`` follow it to the host, and where the
        total overflowed the pass is repeated once with an output of the exact
        total.  The packed files cross PCIe in one copy.  ``stream`` (a raw
        handle, 0: none) is the stream still writing the spans, if any: it is
        waited for first.  Synchronous."""
        import torch
        it = np.ascontiguousarray(np.asarray(items).reshape(-1, 2)).astype(np.uint32)
        n = int(it.shape[0])
        if n == 0:
            return []
        H = self.height if height is None else int(height)
        W = self.width if width is None else int(width)
        dev = torch.device("cuda", self.device)
        if stream:
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        else:
            self.synchronize()
        st = self.span_stream()
        cap = int(out_capacity) or n * (H * (24 + W // 64) + 256)   # an empty row takes some 8 + W / 150 bytes
        with torch.cuda.stream(st):
            d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            while True:
                d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
                self.encode_span_masks(it, spans=spans, span_offsets=span_offsets, capacity=capacity,
                                       out=d_out.data_ptr(), out_capacity=cap, file_offsets=d_off.data_ptr(),
                                       n_frames=n_frames, n_labels=n_labels, height=H, width=W,
                                       stream=st.cuda_stream)
                off = d_off.cpu().numpy()   # waits for the stream
                total = int(off[n])
                if total <= cap:
                    break
                cap = total
            h_out = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            h_out.copy_(d_out[:total], non_blocking=True)
            st.synchronize()
            buf = h_out.numpy()
        return [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]

    # -- baseline JPEG files of RGB frames ------------------------------------------------
    def encode_jpeg(self, n: int, *, rgb: int, out: int, out_capacity: int, file_offsets: int, quality: int = 95,
                    subsampling: str = "420", height: Optional[int] = None, width: Optional[int] = None,
                    stream: int = 0) -> None:
        """Enqueue the JPEG files of ``n`` RGB frames (csg_encode_jpeg; raw
        device pointers, like :meth:`encode_span_masks`): frame f of ``rgb``
        (n, H, W, 3) uint8 at any alignment becomes a finished baseline JPEG
        (:func:`writers.jpeg_bytes` states the bytes) at ``out +
        file_offsets[f]``.  ``file_offsets`` (n + 1) uint64 gets exact offsets
        whether or not the total ``file_offsets[n]`` fits ``out_capacity``; a
        file that does not fit is not written, and the caller repeats the pass
        with an output of that size.  ``subsampling`` is "444" or "420",
        ``height`` / ``width`` default to the renderer's."""
        if str(subsampling) not in _lib.JPEG_SUBSAMPLING:
            raise ValueError(f"encode_jpeg: subsampling {subsampling!r} is neither '444' nor '420'")
        job = _lib.JpegJob(self.width if width is None else int(width), self.height if height is None else int(height),
                           int(n), int(quality), _lib.JPEG_SUBSAMPLING[str(subsampling)], 0, rgb or None, out or None,
                           int(out_capacity), file_offsets or None)
        self._check(self.lib.csg_encode_jpeg(self.ctx, C.byref(job), stream or None), "encode_jpeg")

    def jpegs_host(self, n: int, *, rgb: int, quality: int = 95, subsampling: str = "420",
                   height: Optional[int] = None, width: Optional[int] = None, out_capacity: int = 0,
                   stream: int = 0, views: bool = False) -> List[bytes]:
        """:meth:`encode_jpeg` delivered to the host: the files of ``n`` frames
        as a list of ``bytes`` (with ``views`` as memoryviews of the page-locked
        buffer they arrived in, which lives as long as one of them: no copy).  The pass runs on a stream of the wrapper's own
        into an output of ``out_capacity`` bytes (0: a guess from the frame
        size), ``file_offsets`` follow it to the host, and where the total
        overflowed the pass is repeated once with an output of the exact total.
        The packed files cross PCIe in one copy.  ``stream`` (a raw handle, 0:
        none) is the stream still writing ``rgb``, if any: it is waited for
        first.  Synchronous."""
        import torch
        n = int(n)
        if n == 0:
            return []
        H = self.height if height is None else int(height)
        W = self.width if width is None else int(width)
        dev = torch.device("cuda", self.device)
        if stream:
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        else:
            self.synchronize()
        st = self.span_stream()
        cap = int(out_capacity) or n * (H * W // 2 + 4096)   # a rendered frame at quality 95 takes a tenth of that
        with torch.cuda.stream(st):
            d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            while True:
                d_out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
                self.encode_jpeg(n, rgb=rgb, out=d_out.data_ptr(), out_capacity=cap, file_offsets=d_off.data_ptr(),
                                 quality=quality, subsampling=subsampling, height=H, width=W, stream=st.cuda_stream)
                off = d_off.cpu().numpy()   # waits for the stream
                total = int(off[n])
                if total <= cap:
                    break
                cap = total
            h_out = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            h_out.copy_(d_out[:total], non_blocking=True)
            st.synchronize()
            buf = h_out.numpy()
        if views:
            return [memoryview(buf[int(off[i]):int(off[i + 1])]) for i in range(n)]
        return [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]

    # -- voxel-downsampled labelled point clouds ------------------------------------------
    def voxel_cloud(self, n: int, *, voxel_size: float, capacity: int, points: int, rgb: int = 0, instance: int = 0,
                    vx_xyz: int = 0, vx_rgb: int = 0, vx_label: int = 0, vx_count: int = 0, vx_total: int = 0,
                    vx_dropped: int = 0, height: Optional[int] = None, width: Optional[int] = None,
                    n_labels: Optional[int] = None, stream: int = 0) -> None:
        """Enqueue the voxel clouds of ``n`` frames (csg_voxel_cloud; raw device
        pointers, like :meth:`sample_points`): the finite points of ``points``
        (n, H, W, 3) float32 (world space, as the "points" output) whose id in
        ``instance`` (n, H, W) int32 lies in ``[-1, n_labels)`` (0: every id is
        -1), binned on the world-fixed grid of ``voxel_size`` metres per (cell,
        id), one record per voxel in the order of the voxels' first pixels:
        ``vx_xyz`` (n, C, 3) float32 centroids, ``vx_rgb`` (n, C, 3) uint8 mean
        colours of ``rgb`` (n, H, W, 3) uint8 (0: zeros), ``vx_label`` (n, C)
        int32, ``vx_count`` (n, C) uint32, with C = ``capacity``; rows past a
        frame's voxels hold NaN, 0, -1 and 0.  ``vx_total`` (n,) uint32 gets the
        voxels of each frame, or 0xFFFFFFFF where they exceed ``capacity`` (that
        frame's rows are then unspecified: repeat with a larger one);
        ``vx_dropped`` (n,) uint32 the points beyond +-2^17 cells of the origin.
        Sums are integers: the result is the same bytes on every run.
        ``n_labels`` defaults to the scene's, ``height`` / ``width`` to the
        renderer's.  On the stream of the render that wrote the sources no
        synchronisation is needed in between."""
        job = _lib.VoxelJob(self.width if width is None else int(width), self.height if height is None else int(height),
                            self.n_labels if n_labels is None else int(n_labels), int(capacity), float(voxel_size), 0,
                            points or None, rgb or None, instance or None, vx_xyz or None, vx_rgb or None,
                            vx_label or None, vx_count or None, vx_total or None, vx_dropped or None)
        self._check(self.lib.csg_voxel_cloud(self.ctx, C.byref(job), int(n), stream or None), "voxel_cloud")

    def voxel_cloud_host(self, n: int, voxel_size: float = DEFAULT_VOXEL_SIZE, *, points: int, rgb: int = 0,
                         instance: int = 0, capacity: int = 0, height: Optional[int] = None,
                         width: Optional[int] = None, n_labels: Optional[int] = None, stream: int = 0,
                         keep: int = 0, keep_pool: int = 16384, keep_seed: int = 0, frame_keys=None):
        """:meth:`voxel_cloud` of device images (pointers ``points``, ``rgb``,
        ``instance``), delivered to the host: returns ``(frames, capacity,
        dropped)`` where ``frames`` is a list of ``n`` structured arrays of
        ``voxel_cloud.RECORD_DTYPE`` (fields ``xyz``, ``rgb``, ``label``,
        ``count``), ``capacity`` the per-frame capacity that was enough and
        ``dropped`` (n,) uint32 the dropped points.  The pass starts at
        ``capacity`` (0: ``voxel_cloud.DEFAULT_VOXEL_CAPACITY``), never above
        H * W, and is repeated with the capacity doubled, up to H * W, while
        any frame reports 0xFFFFFFFF.  Only the totals and the records in use
        cross PCIe: the pass runs on a stream of the wrapper's own, and the
        frames' records are packed on the device and copied once.  ``stream``
        (a raw handle, 0: none) is the stream still writing the sources, if
        any: it is waited for first.  Synchronous.

        ``keep`` = K > 0 reduces every cloud to at most K records by
        :meth:`farthest_points` on the device, once the capacity has settled:
        at most ``keep_pool`` records of a frame, evenly strided, are
        candidates, the start is hashed from ``keep_seed`` and the frame's key
        (``frame_keys`` (n,) uint32; None: the frame's place), and each frame
        returns its first ``min(K, t0)`` records in farthest-point order (every
        prefix of them is such a reduction too).  Only those cross PCIe."""
        import torch
        n = int(n)
        H = self.height if height is None else int(height)
        W = self.width if width is None else int(width)
        keep = int(keep)
        if keep < 0 or keep > 16384:
            raise CsgError(f"voxel_cloud_host: keep {keep} outside 0..16384")
        cap = min(int(capacity) or DEFAULT_VOXEL_CAPACITY, H * W)
        dev = torch.device("cuda", self.device)
        if stream:
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        else:
            self.synchronize()
        st = self.span_stream()
        with torch.cuda.stream(st):
            d_tot = torch.empty((2, n), dtype=torch.int32, device=dev)
            while True:
                d_xyz = torch.empty((n, cap, 3), dtype=torch.float32, device=dev)
                d_rgb = torch.empty((n, cap, 3), dtype=torch.uint8, device=dev)
                d_lab = torch.empty((n, cap), dtype=torch.int32, device=dev)
                d_cnt = torch.empty((n, cap), dtype=torch.int32, device=dev)
                self.voxel_cloud(n, voxel_size=voxel_size, capacity=cap, points=points, rgb=rgb, instance=instance,
                                 vx_xyz=d_xyz.data_ptr(), vx_rgb=d_rgb.data_ptr(), vx_label=d_lab.data_ptr(),
                                 vx_count=d_cnt.data_ptr(), vx_total=d_tot[0].data_ptr(),
                                 vx_dropped=d_tot[1].data_ptr(), height=H, width=W, n_labels=n_labels,
                                 stream=st.cuda_stream)
                tot = d_tot.cpu().numpy().view(np.uint32)   # waits for the stream
                if not (tot[0] == VOXEL_OVERFLOW).any():
                    break
                if cap >= H * W:
                    raise CsgError("voxel_cloud_host: a frame overflows a capacity of H * W")
                cap = min(2 * cap, H * W)
            totals = tot[0].astype(np.int64)
            if keep:   # the first min(K, t0) farthest-point samples of each frame instead of its records
                d_key = None if frame_keys is None else \
                    torch.from_numpy(np.ascontiguousarray(frame_keys, np.uint32).reshape(n).view(np.int32)).to(dev)
                k_xyz = torch.empty((n, keep, 3), dtype=torch.float32, device=dev)
                k_rgb = torch.empty((n, keep, 3), dtype=torch.uint8, device=dev)
                k_lab = torch.empty((n, keep), dtype=torch.int32, device=dev)
                k_cnt = torch.empty((n, keep), dtype=torch.int32, device=dev)
                k_n = torch.empty((n, 2), dtype=torch.int32, device=dev)
                self.farthest_points(n, rows=cap, pool=keep_pool, samples=keep, xyz=d_xyz.data_ptr(),
                                     counts=d_tot[0].data_ptr(), seed=keep_seed,
                                     set_keys=d_key.data_ptr() if d_key is not None else 0, fp_xyz=k_xyz.data_ptr(),
                                     fp_count=k_n.data_ptr(),
                                     payloads=((d_rgb.data_ptr(), k_rgb.data_ptr(), 3, 0),
                                               (d_lab.data_ptr(), k_lab.data_ptr(), 4, 0xFF),
                                               (d_cnt.data_ptr(), k_cnt.data_ptr(), 4, 0)), stream=st.cuda_stream)
                totals = k_n.cpu().numpy().view(np.uint32)[:, 0].astype(np.int64)   # t0 <= K
                d_xyz, d_rgb, d_lab, d_cnt = k_xyz, k_rgb, k_lab, k_cnt
            parts = []
            for t in (d_xyz, d_rgb, d_lab, d_cnt):   # the records in use, and no more
                parts.append(torch.cat([t[f, :int(totals[f])] for f in range(n)]).cpu().numpy() if n else None)
            st.synchronize()
        ends = np.cumsum(totals)
        frames = []
        for f in range(n):
            lo, hi = int(ends[f] - totals[f]), int(ends[f])
            rec = np.empty(hi - lo, RECORD_DTYPE)
            rec["xyz"].view(np.uint32)[...] = parts[0][lo:hi].view(np.uint32)   # bit copies
            rec["rgb"] = parts[1][lo:hi]
            rec["label"] = parts[2][lo:hi]
            rec["count"] = parts[3][lo:hi].view(np.uint32)
            frames.append(rec)
        return frames, cap, tot[1].copy()

    def keep_points(self, keep: bool = True) -> None:
        """Host-output batches (:meth:`render`, :meth:`render_files`) render
        their world-space points into the context's device image even when
        "points" is not among the host outputs and no file kind needs them
        (csg_keep_points): :meth:`last_points` then finds them."""
        self._check(self.lib.csg_keep_points(self.ctx, int(bool(keep))), "keep_points")

    def last_points(self):
        """``(device pointer, frames)`` of the last host-output batch's points image
        (csg_last_points), valid until the next batch; (0, 0) when it made none."""
        p, nf = C.c_void_p(), C.c_uint32()
        self._check(self.lib.csg_last_points(self.ctx, C.byref(p), C.byref(nf)), "last_points")
        return int(p.value or 0), int(nf.value)

    # -- simulated stereo-camera depth ----------------------------------------------------
    def sensor_depth(self, n: int, *, depth: int, intrinsics: int, model, seed: int = 0, frame_keys: int = 0,
                     sensor_depth: int = 0, sensor_cause: int = 0, sensor_count: int = 0,
                     height: Optional[int] = None, width: Optional[int] = None, stream: int = 0) -> None:
        """Enqueue the stereo-camera depth of ``n`` frames (csg_sensor_depth; raw
        device pointers, like :meth:`voxel_cloud`): ``depth`` (n, H, W) float32
        as the "depth" output and ``intrinsics`` (n, 4) float32 ``fx, fy, cx,
        cy`` (only fx is read) under ``model``, a :class:`depth_sensor.StereoModel`
        or a dict of the job's integers as ``StereoModel.to_job_fields`` gives
        them.  ``sensor_depth`` (n, H, W) float32 gets the depth the camera
        returns, 0.0 where it returns none; ``sensor_cause`` (n, H, W) uint8
        why (``depth_sensor.cause_names``); ``sensor_count`` (n, 7) uint32 the
        pixels of each cause.  Any output may be 0, not all; ``sensor_depth``
        must not overlap ``depth``.  The noise of a frame is a function of
        ``seed`` and its key: ``frame_keys`` (n,) uint32, or 0 for the frame's
        place in the batch.  ``height`` / ``width`` default to the renderer's.
        On the stream of the render that wrote the depth no synchronisation is
        needed in between."""
        f = model if isinstance(model, dict) else model.to_job_fields()
        job = _lib.SensorJob(self.width if width is None else int(width), self.height if height is None else int(height),
                             int(f["radius"]), int(f["min_support"]), int(f["tol"]), int(f["subpixel_bits"]),
                             int(f["noise_k"]), int(f.get("seed", seed)) & 0xFFFFFFFF, int(f["flags"]),
                             float(f["baseline"]), float(f["z_min"]), float(f["z_max"]), depth or None,
                             intrinsics or None, frame_keys or None, sensor_depth or None, sensor_cause or None,
                             sensor_count or None)
        self._check(self.lib.csg_sensor_depth(self.ctx, C.byref(job), int(n), stream or None), "sensor_depth")

    def sensor_depth_host(self, n: int, model, *, depth: int, intrinsics, frame_keys=None, seed: int = 0,
                          want=("depth", "cause", "count"), height: Optional[int] = None,
                          width: Optional[int] = None, stream: int = 0) -> dict:
        """:meth:`sensor_depth` of a device depth image (pointer ``depth``),
        delivered to the host: a dict with ``"depth"`` (n, H, W) float32,
        ``"cause"`` (n, H, W) uint8 and ``"count"`` (n, 7) uint32, as far as
        ``want`` names them.  ``intrinsics`` (n, 4) and ``frame_keys`` (n,) are
        host arrays.  The pass runs on a stream of the wrapper's own;
        ``stream`` (a raw handle, 0: none) is the stream still writing the
        depth, if any: it is waited for first.  Synchronous."""
        import torch
        n = int(n)
        H = self.height if height is None else int(height)
        W = self.width if width is None else int(width)
        bad = [k for k in want if k not in ("depth", "cause", "count")]
        if bad or not want:
            raise CsgError(f"sensor_depth_host: want {tuple(want)!r}: some of depth, cause, count")
        dev = torch.device("cuda", self.device)
        if stream:
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        else:
            self.synchronize()
        st = self.span_stream()
        with torch.cuda.stream(st):
            d_in = torch.from_numpy(np.ascontiguousarray(intrinsics, np.float32).reshape(n, 4)).to(dev)
            d_keys = None if frame_keys is None else \
                torch.from_numpy(np.ascontiguousarray(frame_keys, np.uint32).reshape(n).view(np.int32)).to(dev)
            d_out = {"depth": torch.empty((n, H, W), dtype=torch.float32, device=dev) if "depth" in want else None,
                     "cause": torch.empty((n, H, W), dtype=torch.uint8, device=dev) if "cause" in want else None,
                     "count": torch.empty((n, 7), dtype=torch.int32, device=dev) if "count" in want else None}
            ptr = {k: (t.data_ptr() if t is not None else 0) for k, t in d_out.items()}
            self.sensor_depth(n, depth=depth, intrinsics=d_in.data_ptr(), model=model, seed=seed,
                              frame_keys=d_keys.data_ptr() if d_keys is not None else 0, sensor_depth=ptr["depth"],
                              sensor_cause=ptr["cause"], sensor_count=ptr["count"], height=H, width=W,
                              stream=st.cuda_stream)
            out = {k: t.cpu().numpy() for k, t in d_out.items() if t is not None}
            st.synchronize()
        if "count" in out:
            out["count"] = out["count"].view(np.uint32)
        return out

    def keep_depth(self, keep: bool = True) -> None:
        """Host-output batches (:meth:`render`, :meth:`render_files`) render
        their depth into the context's device image even when "depth" is not
        among the host outputs and nothing else needs it (csg_keep_depth):
        :meth:`last_depth` then finds it."""
        self._check(self.lib.csg_keep_depth(self.ctx, int(bool(keep))), "keep_depth")

    def last_depth(self):
        """``(device pointer, frames)`` of the last host-output batch's depth image
        (csg_last_depth), valid until the next batch; (0, 0) when it made none."""
        p, nf = C.c_void_p(), C.c_uint32()
        self._check(self.lib.csg_last_depth(self.ctx, C.byref(p), C.byref(nf)), "last_depth")
        return int(p.value or 0), int(nf.value)

    # -- lens distortion --------------------------------------------------------------------
    def lens_map(self, model, host_map: Optional[np.ndarray] = None):
        """The device map of ``model`` (a :class:`lens.LensModel`): an (H, W, 2) int32 tensor made once by
        :func:`lens.build_map` (or uploaded from ``host_map``, the same map made earlier) and cached per model."""
        import torch
        from . import lens as _lens
        cache = self.__dict__.setdefault("_lens_maps", {})
        if model not in cache:
            mp = _lens.build_map(model)[0] if host_map is None else np.ascontiguousarray(host_map, np.int32)
            if mp.shape != (model.height, model.width, 2):
                raise CsgError(f"lens_map: a map of shape {mp.shape} for a {model.width} x {model.height} camera")
            cache[model] = torch.from_numpy(mp).to(torch.device("cuda", self.device))
        return cache[model]

    def lens_remap(self, n: int, *, map: int, width: int, height: int, src_width: Optional[int] = None,
                   src_height: Optional[int] = None, rgb: int = 0, instance: int = 0, depth: int = 0,
                   obj_coords: int = 0, lens_rgb: int = 0, lens_instance: int = 0, lens_depth: int = 0,
                   lens_coords: int = 0, lens_valid: int = 0, lens_stats: int = 0, lens_count: int = 0,
                   n_labels: Optional[int] = None, rgb_filter: str = "bilinear", stream: int = 0) -> None:
        """Enqueue the lens resampling of ``n`` frames (csg_lens_remap; raw device pointers, like
        :meth:`sensor_depth`): the sources ``rgb`` (n, SH, SW, 3) uint8, ``instance`` (n, SH, SW) int32,
        ``depth`` (n, SH, SW) float32 and ``obj_coords`` (n, SH, SW, 3) uint16 of the source camera
        (``src_width`` x ``src_height``, default the renderer's) through ``map`` (H, W, 2) int32 into
        ``lens_rgb``, ``lens_instance``, ``lens_depth``, ``lens_coords``, ``lens_valid`` (n, H, W) uint8 (0 valid,
        else ``lens.cause_names``), ``lens_stats`` (n, n_labels, 5) uint32 as ``inst_stats`` and
        ``lens_count`` (n, 3) uint32.  Any output may be 0, not all; each needs its source.  ``rgb_filter``:
        "bilinear" (8-bit fixed point, four taps) or "nearest"."""
        if rgb_filter not in _lib.LENS_FILTERS:
            raise CsgError(f"lens_remap: rgb_filter {rgb_filter!r}: one of {sorted(_lib.LENS_FILTERS)}")
        job = _lib.LensJob(int(width), int(height), self.width if src_width is None else int(src_width),
                           self.height if src_height is None else int(src_height),
                           self.n_labels if n_labels is None else int(n_labels), _lib.LENS_FILTERS[rgb_filter],
                           map or None, rgb or None, instance or None, depth or None, obj_coords or None,
                           lens_rgb or None, lens_instance or None, lens_depth or None, lens_coords or None,
                           lens_valid or None, lens_stats or None, lens_count or None)
        self._check(self.lib.csg_lens_remap(self.ctx, C.byref(job), int(n), stream or None), "lens_remap")

    def lens_points(self, n: int, model, *, n_keypoints: int, keypoints_uv: int, keypoints_vis: int, lens_uv: int,
                    lens_vis: int, stream: int = 0) -> None:
        """Enqueue the keypoints of ``n`` frames through ``model``'s forward model (csg_lens_points; raw device
        pointers): ``keypoints_uv`` (n, K, 2) float32 source pixels and ``keypoints_vis`` (n, K) int32 into
        ``lens_uv`` and ``lens_vis`` of the output camera (:func:`lens.distort_points` is the definition)."""
        m = model.to_c()
        job = _lib.LensJob()
        job.model = C.pointer(m)
        job.n_keypoints = int(n_keypoints)
        job.keypoints_uv, job.keypoints_vis = keypoints_uv or None, keypoints_vis or None
        job.lens_uv, job.lens_vis = lens_uv or None, lens_vis or None
        self._check(self.lib.csg_lens_points(self.ctx, C.byref(job), int(n), stream or None), "lens_points")

    def lens_remap_host(self, n: int, model, *, rgb: int = 0, instance: int = 0, depth: int = 0, obj_coords: int = 0,
                        keypoints_uv=None, keypoints_vis=None, n_labels: Optional[int] = None,
                        rgb_filter: str = "bilinear", stream: int = 0) -> dict:
        """:meth:`lens_remap` of the kept device images of a host-output batch (``keep_rgb`` / ``last_rgb``,
        ``keep_instance`` / ``last_instance``, ``keep_depth`` / ``last_depth``; ``obj_coords`` a pointer of the
        caller's), delivered to the host: a dict with ``"rgb"``, ``"instance"`` and ``"stats"``, ``"depth"``,
        ``"coords"`` as far as their sources are given, and always ``"valid"`` and ``"count"``.  The source
        camera of ``model`` must have the size of the images.  With ``keypoints_uv`` (n, K, 2) and
        ``keypoints_vis`` (n, K) host arrays also ``"keypoints_uv"`` and ``"keypoints_vis"`` in the output
        camera (:meth:`lens_points`).  The pass runs on a stream of the wrapper's own; ``stream`` (a raw handle,
        0: none) is the stream still writing the sources, if any: it is waited for first.  Synchronous."""
        import torch
        n = int(n)
        H, W, SH, SW = int(model.height), int(model.width), int(model.src_height), int(model.src_width)
        L = self.n_labels if n_labels is None else int(n_labels)
        dev = torch.device("cuda", self.device)
        if stream:
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        else:
            self.synchronize()
        d_map = self.lens_map(model)
        st = self.span_stream()
        with torch.cuda.stream(st):
            d_out = {"valid": torch.empty((n, H, W), dtype=torch.uint8, device=dev),
                     "count": torch.empty((n, 3), dtype=torch.int32, device=dev)}
            if rgb:
                d_out["rgb"] = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
            if instance:
                d_out["instance"] = torch.empty((n, H, W), dtype=torch.int32, device=dev)
                d_out["stats"] = torch.empty((n, L, 5), dtype=torch.int32, device=dev)
            if depth:
                d_out["depth"] = torch.empty((n, H, W), dtype=torch.float32, device=dev)
            if obj_coords:
                d_out["coords"] = torch.empty((n, H, W, 3), dtype=torch.int16, device=dev)
            ptr = {k: (d_out[k].data_ptr() if k in d_out else 0) for k in
                   ("rgb", "instance", "stats", "depth", "coords", "valid", "count")}
            self.lens_remap(n, map=d_map.data_ptr(), width=W, height=H, src_width=SW, src_height=SH, rgb=rgb,
                            instance=instance, depth=depth, obj_coords=obj_coords, lens_rgb=ptr["rgb"],
                            lens_instance=ptr["instance"], lens_depth=ptr["depth"], lens_coords=ptr["coords"],
                            lens_valid=ptr["valid"], lens_stats=ptr["stats"], lens_count=ptr["count"], n_labels=L,
                            rgb_filter=rgb_filter, stream=st.cuda_stream)
            if keypoints_uv is not None:
                uv = np.ascontiguousarray(keypoints_uv, np.float32)
                K = uv.shape[1]
                d_uv = torch.from_numpy(uv.reshape(n, K, 2)).to(dev)
                d_vis = torch.from_numpy(np.ascontiguousarray(keypoints_vis, np.int32).reshape(n, K)).to(dev)
                d_out["keypoints_uv"] = torch.empty_like(d_uv)
                d_out["keypoints_vis"] = torch.empty_like(d_vis)
                self.lens_points(n, model, n_keypoints=K, keypoints_uv=d_uv.data_ptr(), keypoints_vis=d_vis.data_ptr(),
                                 lens_uv=d_out["keypoints_uv"].data_ptr(), lens_vis=d_out["keypoints_vis"].data_ptr(),
                                 stream=st.cuda_stream)
            out = {k: t.cpu().numpy() for k, t in d_out.items()}
            st.synchronize()
        for k, dt in (("count", np.uint32), ("stats", np.uint32), ("coords", np.uint16)):
            if k in out:
                out[k] = out[k].view(dt)
        return out

    # -- farthest-point sampling ------------------------------------------------------------
    def farthest_points(self, n_sets: int, *, rows: int, pool: int = 16384, samples: int, xyz: int, counts: int = 0,
                        set_keys: int = 0, seed: int = 0, fp_index: int = 0, fp_xyz: int = 0, fp_dist2: int = 0,
                        fp_count: int = 0, payloads=(), stream: int = 0) -> None:
        """Enqueue the farthest-point samples of ``n_sets`` point sets
        (csg_farthest_points; raw device pointers, like :meth:`sample_points`):
        ``xyz`` (S, C, 3) float32 with C = ``rows``, of which set s has
        ``counts[s]`` rows in use (``counts`` (S,) uint32; 0: all C;
        0xFFFFFFFF, the voxel clouds' overflow mark: none).  At most ``pool``
        rows of a set are candidates (:func:`farthest_points.candidate_rows`);
        rows with a coordinate that is not finite are skipped.  ``samples`` = K
        are chosen: a start hashed from ``seed`` and the set's key
        (``set_keys`` (S,) uint32; 0: the set's place), then always the
        candidate farthest from those chosen, the lowest on ties.
        ``fp_index`` (S, K) uint32 gets the rows, ``fp_xyz`` (S, K, 3) float32
        their points, ``fp_dist2`` (S, K) float32 the squared distance at which
        each was chosen (+inf first, then non-increasing) and ``fp_count``
        (S, 2) uint32 ``t0`` (the distinct samples; entries past it repeat the
        run and have distance 0) and the valid candidates.  ``payloads`` is up
        to 4 tuples ``(src, dst, row_bytes, fill)``: rows of ``src``
        (S, C, row_bytes) are gathered to ``dst`` (S, K, row_bytes) by
        ``fp_index``; an empty set's rows are ``fill`` bytes.  Any output may be
        0, not all.  On the stream of the pass that wrote the sources no
        synchronisation is needed in between."""
        payloads = tuple(payloads)
        if len(payloads) > _lib.FPS_MAX_PAYLOADS:
            raise CsgError(f"farthest_points: {len(payloads)} payloads, at most {_lib.FPS_MAX_PAYLOADS}")
        job = _lib.FpsJob(int(rows), int(pool), int(samples), int(seed) & 0xFFFFFFFF, len(payloads), 0, xyz or None,
                          counts or None, set_keys or None, fp_index or None, fp_xyz or None, fp_dist2 or None,
                          fp_count or None)
        for i, (src, dst, row_bytes, fill) in enumerate(payloads):
            job.payloads[i] = _lib.FpsPayload(src or None, dst or None, int(row_bytes), int(fill) & 0xFF)
        self._check(self.lib.csg_farthest_points(self.ctx, C.byref(job), int(n_sets), stream or None),
                    "farthest_points")

    def farthest_points_host(self, xyz, counts=None, *, samples: int, pool: int = 16384, seed: int = 0,
                             set_keys=None, payloads=()) -> dict:
        """:meth:`farthest_points` of host arrays, delivered to the host:
        ``xyz`` (S, C, 3) float32, ``counts`` and ``set_keys`` (S,) uint32 or
        None, ``payloads`` up to 4 arrays (S, C, ...) of any dtype (or tuples
        ``(array, fill)``; the fill byte defaults to 0).  Returns a dict with
        ``"index"`` (S, K) uint32, ``"xyz"`` (S, K, 3) float32, ``"dist2"``
        (S, K) float32, ``"count"`` (S, 2) uint32 and ``"payloads"``, the list
        of the gathered arrays (S, K, ...).  Synchronous."""
        import torch
        xyz = np.ascontiguousarray(xyz, np.float32)
        if xyz.ndim != 3 or xyz.shape[2] != 3:
            raise CsgError(f"farthest_points_host: xyz of shape {xyz.shape} is not (S, C, 3)")
        S, Cr, K = xyz.shape[0], xyz.shape[1], int(samples)
        dev = torch.device("cuda", self.device)
        st = self.span_stream()

        def up(a):   # bit copies: torch has no unsigned 32-bit tensors
            return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to(dev)

        with torch.cuda.stream(st):
            d_xyz = up(xyz)
            d_cnt = None if counts is None else up(np.ascontiguousarray(counts, np.uint32).reshape(S))
            d_key = None if set_keys is None else up(np.ascontiguousarray(set_keys, np.uint32).reshape(S))
            d_idx = torch.empty((S, K), dtype=torch.int32, device=dev)
            d_pts = torch.empty((S, K, 3), dtype=torch.int32, device=dev)
            d_d2 = torch.empty((S, K), dtype=torch.int32, device=dev)
            d_n = torch.empty((S, 2), dtype=torch.int32, device=dev)
            pl, keep = [], []
            for p in payloads:
                arr, fill = p if isinstance(p, tuple) else (p, 0)
                arr = np.ascontiguousarray(arr)
                if arr.ndim < 2 or arr.shape[:2] != (S, Cr):
                    raise CsgError(f"farthest_points_host: a payload of shape {arr.shape} is not (S, C, ...)")
                rb = arr.dtype.itemsize * int(np.prod(arr.shape[2:], dtype=np.int64))
                d_src = up(arr)
                d_dst = torch.empty((S, K, rb), dtype=torch.uint8, device=dev)
                keep.append((arr, d_src, d_dst))
                pl.append((d_src.data_ptr(), d_dst.data_ptr(), rb, fill))
            self.farthest_points(S, rows=Cr, pool=pool, samples=K, xyz=d_xyz.data_ptr(),
                                 counts=d_cnt.data_ptr() if d_cnt is not None else 0,
                                 set_keys=d_key.data_ptr() if d_key is not None else 0, seed=seed,
                                 fp_index=d_idx.data_ptr(), fp_xyz=d_pts.data_ptr(), fp_dist2=d_d2.data_ptr(),
                                 fp_count=d_n.data_ptr(), payloads=pl, stream=st.cuda_stream)
            out = {"index": d_idx.cpu().numpy().view(np.uint32), "xyz": d_pts.cpu().numpy().view(np.float32),
                   "dist2": d_d2.cpu().numpy().view(np.float32), "count": d_n.cpu().numpy().view(np.uint32),
                   "payloads": [d_dst.cpu().numpy().reshape(-1).view(arr.dtype).reshape((S, K) + arr.shape[2:])
                                for arr, _, d_dst in keep]}
            st.synchronize()
        return out

    def keep_rgb(self, keep: bool = True) -> None:
        """Host-output batches (:meth:`render`, :meth:`render_files`) render
        their RGB into the context's device image even when "rgb" is not among
        the host outputs and no file kind needs it (csg_keep_rgb):
        :meth:`last_rgb` then finds it."""
        self._check(self.lib.csg_keep_rgb(self.ctx, int(bool(keep))), "keep_rgb")

    def last_rgb(self):
        """``(device pointer, frames)`` of the last host-output batch's RGB image
        (csg_last_rgb), valid until the next batch; (0, 0) when it made none."""
        p, nf = C.c_void_p(), C.c_uint32()
        self._check(self.lib.csg_last_rgb(self.ctx, C.byref(p), C.byref(nf)), "last_rgb")
        return int(p.value or 0), int(nf.value)

    def keep_instance(self, keep: bool = True) -> None:
        """Host-output batches (:meth:`render`, :meth:`render_files`) keep their
        instance ids on the device even when "instance" is not among the host
        outputs (csg_keep_instance): :meth:`last_instance` then finds them."""
        self._check(self.lib.csg_keep_instance(self.ctx, int(bool(keep))), "keep_instance")

    def last_instance(self):
        """``(device pointer, frames)`` of the last host-output batch's id image
        (csg_last_instance), valid until the next batch; (0, 0) when it made none."""
        p, nf = C.c_void_p(), C.c_uint32()
        self._check(self.lib.csg_last_instance(self.ctx, C.byref(p), C.byref(nf)), "last_instance")
        return int(p.value or 0), int(nf.value)

    def instance_bounds(self, set_id: int = 0) -> np.ndarray:
        """(I, 2, 3) float32 world-space AABB of every instance under a transform set (GPU reduction)."""
        out = np.empty((self.n_inst, 6), np.float32)
        self._check(self.lib.csg_instance_bounds(self.ctx, set_id, out.ctypes.data), "instance_bounds")
        return out.reshape(-1, 2, 3)

    def host_id_bytes(self) -> int:
        """Bytes per instance id on the host wire of host-output batches (1, 2 or 4; csg_host_id_bytes)."""
        n = self.lib.csg_host_id_bytes(self.ctx)
        if n < 0:
            self._check(n, "host_id_bytes")
        return int(n)

    def synchronize(self) -> None:
        self._check(self.lib.csg_synchronize(self.ctx), "synchronize")

    def batch_stats(self) -> Dict[str, float]:
        st = _lib.BatchStats()
        self._check(self.lib.csg_get_batch_stats(self.ctx, C.byref(st)), "get_batch_stats")
        return {n: getattr(st, n) for n, _ in _lib.BatchStats._fields_}

    def size_work(self, frames, n: Optional[int] = None, on_device: bool = False,
                  margin: float = 0.25) -> Dict[str, float]:
        """Size the work buffers from a sizing pass over ``frames``
        (csg_size_work): a FRAME_DTYPE array, or with ``on_device`` a device
        pointer (int) to ``n`` frame records.  Writes each frame's work hints
        (``records_hint``, ``bins_hint``) into the records passed -- the array
        itself, or the device records -- so later batches of those records get
        regions of their own size.  Returns :meth:`work_info`."""
        info = _lib.WorkInfo()
        if on_device:
            self._check(self.lib.csg_size_work(self.ctx, int(frames), int(n), 1, float(margin), C.byref(info)),
                        "size_work")
        else:
            fr = np.ascontiguousarray(frames, FRAME_DTYPE)
            self._check(self.lib.csg_size_work(self.ctx, fr.ctypes.data, fr.shape[0], 0, float(margin),
                                               C.byref(info)), "size_work")
            if fr is not frames:   # a converted copy: hand the hints back
                frames["records_hint"] = fr["records_hint"]
                frames["bins_hint"] = fr["bins_hint"]
        return {k: getattr(info, k) for k, _ in _lib.WorkInfo._fields_ if k != "pad"}

    def work_info(self) -> Dict[str, float]:
        """Current work-buffer caps, the last sizing pass and the buffers' device bytes."""
        info = _lib.WorkInfo()
        self._check(self.lib.csg_get_work_info(self.ctx, C.byref(info)), "get_work_info")
        return {k: getattr(info, k) for k, _ in _lib.WorkInfo._fields_ if k != "pad"}

    def timing_reset(self) -> None:
        self._check(self.lib.csg_timing_reset(self.ctx), "timing_reset")

    def timing_read(self) -> Dict[str, float]:
        t = _lib.Timing()
        self._check(self.lib.csg_timing_read(self.ctx, C.byref(t)), "timing_read")
        return {n: getattr(t, n) for n, _ in _lib.Timing._fields_}

    def project_keypoints(self, pts_world: np.ndarray, view: np.ndarray, proj: np.ndarray):
        p = np.ascontiguousarray(np.asarray(pts_world).reshape(-1, 3), np.float32)
        v = np.ascontiguousarray(np.asarray(view).reshape(16), np.float32)
        pr = np.ascontiguousarray(np.asarray(proj).reshape(16), np.float32)
        uv = np.empty((p.shape[0], 2), np.float32)
        vis = np.empty(p.shape[0], np.int32)
        self._check(self.lib.csg_project_keypoints(self.ctx, p.ctypes.data, p.shape[0], v.ctypes.data, pr.ctypes.data,
                                                   uv.ctypes.data, vis.ctypes.data), "project_keypoints")
        return uv, vis
