"""Object crops (zoom-in patches), host side: the slot records of
``csg_crop_objects`` (include/csg_api.h), which labels may be cropped, and the
geometry that goes with a crop -- its intrinsics and the keypoints in its
pixels.  The crops themselves are made on the GPU
(:meth:`renderer.Renderer.crop_objects`, :meth:`renderer.Renderer.render_crops`),
and so are their amodal masks (:meth:`renderer.Renderer.crop_amodal`) and the
amodal depth and object coordinates (:meth:`renderer.Renderer.crop_amodal_geometry`).

A crop of side ``S`` samples the square source window ``x0, y0, side`` at
``x0 + (i + 0.5) * step``, ``step = side / S``: source pixel coordinate ``u``
(pixel centres at .5, as ``keypoints_uv``) is crop coordinate ``(u - x0) / step``.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from .scene.model import Scene

CROP_INFO_DTYPE = np.dtype([("label", "<i4"), ("pixels", "<u4"), ("x0", "<f4"), ("y0", "<f4"), ("side", "<f4"),
                            ("frame", "<u4"), ("reserved", "<u4", 2)])
assert CROP_INFO_DTYPE.itemsize == C.sizeof(_lib.CropInfo) == 32

DYNAMIC_KINDS = ("crane", "dumper", "human", "trafficcone")


def eligible_labels(scene: Scene, kinds: Sequence[str] = DYNAMIC_KINDS) -> np.ndarray:
    """uint8 table over the scene's labels (``renderer.scene_labels`` long):
    1 where the label belongs to an object of one of ``kinds``.  Static
    geometry is left out by default: ground and buildings cover most of every
    frame and would win every slot."""
    n = max([o.inst_idx for o in scene.objects] + [i.inst_idx for i in scene.instances] + [-1]) + 1
    t = np.zeros(max(n, 1), np.uint8)
    kinds = set(kinds)
    for o in scene.objects:
        if o.kind in kinds and o.inst_idx >= 0:
            t[o.inst_idx] = 1
    return t


def visible_fraction(crop_mask: np.ndarray, crop_amodal: np.ndarray) -> np.ndarray:
    """Per slot, the visible share of the object inside its crop: float64
    ``crop_mask.sum() / crop_amodal.sum()`` over the S x S samples (set samples
    counted, whatever non-zero value marks them), shaped like the leading
    dimensions (..., S, S) -> (...).  NaN where the amodal mask is empty (an
    empty slot, or an object wholly outside its window)."""
    vis = np.count_nonzero(np.asarray(crop_mask), axis=(-2, -1)).astype(np.float64)
    amo = np.count_nonzero(np.asarray(crop_amodal), axis=(-2, -1)).astype(np.float64)
    out = np.full(amo.shape, np.nan, np.float64)
    np.divide(vis, amo, out=out, where=amo > 0)
    return out


def hidden_mask(crop_mask: np.ndarray, crop_amodal: np.ndarray) -> np.ndarray:
    """The hidden samples of each crop, bool, shaped like the masks: on the
    object (``crop_amodal`` set) and not visible (``crop_mask`` clear) -- where
    ``crop_amodal_depth`` and ``crop_amodal_coords``
    (:meth:`renderer.Renderer.crop_amodal_geometry`) say what ``crop_depth``
    and ``crop_coords`` cannot."""
    return (np.asarray(crop_amodal) != 0) & (np.asarray(crop_mask) == 0)


def _steps(info: np.ndarray, S: int):
    info = np.asarray(info)
    live = info["label"] >= 0
    side = np.where(live, info["side"].astype(np.float64), np.nan)   # empty slots: NaN throughout
    return side / float(S), info["x0"].astype(np.float64), info["y0"].astype(np.float64)


def crop_intrinsics(intr, info: np.ndarray, S: int) -> np.ndarray:
    """The 3x3 pinhole matrix of each crop, float64, shaped ``info.shape + (3, 3)``:
    ``fx / step, fy / step, (cx - x0) / step, (cy - y0) / step`` with the
    frame's ``intr`` (``camera_math.Intrinsics``).  It uses the image
    convention of ``keypoints_uv`` (u right, v down, both positive focal
    lengths) and the renderer's continuous pixel coordinates: crop sample
    (i, j) lies at (i + 1/2, j + 1/2).  (``bop.cam_K`` alone uses OpenCV's
    pixel-centre convention, half a pixel less.)  Empty slots (label -1) get NaN."""
    step, x0, y0 = _steps(info, S)
    K = np.zeros(step.shape + (3, 3), np.float64)
    K[..., 0, 0] = intr.fx / step
    K[..., 1, 1] = intr.fy / step
    K[..., 0, 2] = (intr.cx - x0) / step
    K[..., 1, 2] = (intr.cy - y0) / step
    K[..., 2, 2] = 1.0
    K[np.isnan(step)] = np.nan
    return K


def crop_points_2d(uv: np.ndarray, info: np.ndarray, S: int) -> np.ndarray:
    """Frame pixel coordinates ``uv`` (..., P, 2) (e.g. ``keypoints_uv``) in the
    pixels of each crop: ``info`` (...) broadcasts against the leading
    dimensions of ``uv``; returns float64 ``(u - x0) / step, (v - y0) / step``
    shaped (..., P, 2).  Points outside ``[0, S)`` lie outside the crop."""
    step, x0, y0 = _steps(info, S)
    uv = np.asarray(uv, np.float64)
    out = np.empty(np.broadcast_shapes(uv.shape[:-2], step.shape) + uv.shape[-2:], np.float64)
    out[..., 0] = (uv[..., 0] - x0[..., None]) / step[..., None]
    out[..., 1] = (uv[..., 1] - y0[..., None]) / step[..., None]
    return out
