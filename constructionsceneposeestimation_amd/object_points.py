"""Per-object point samples, host side: what goes with the arrays of
``csg_sample_object_points`` (include/csg_api.h), which are made on the GPU
(:meth:`renderer.Renderer.sample_points`, ``render_crops(want=(..., "points"))``).

A slot's ``pt_choose`` (N,) are row-major pixel indices ``y * W + x`` in
ascending order where the object has more than N pixels (wrapped repeats of
all of them otherwise), ``pt_xyz`` the pixels' points in the OpenCV camera
frame (x right, y down, z forward, metres), ``pt_rgb`` their colours and
``pt_coords`` their 16-bit object coordinates.  The CPU loaders of the
point-based pose networks draw an unordered random choice; point-set networks
do not depend on the order.
"""
from __future__ import annotations

import numpy as np

EMPTY_CHOOSE = 0xFFFFFFFF  # pt_choose of a slot without pixels


def intrinsics_rows(frames: np.ndarray) -> np.ndarray:
    """``fx, fy, cx, cy`` float32 (n, 4) of frame records (``renderer.FRAME_DTYPE``),
    read from each frame's pixel projection (``camera_math.Intrinsics.pixel_projection``:
    rows ``[fx, 0, -cx, 0]`` and ``[0, -fy, -cy, 0]``): the ``intrinsics`` source of
    :meth:`renderer.Renderer.sample_points`.  They keep the renderer's convention,
    in which pixel (x, y) is sampled at (x + 1/2, y + 1/2) (``bop.cam_K`` alone
    uses OpenCV's pixel-centre convention, half a pixel less)."""
    proj = np.asarray(frames["proj"], np.float32).reshape(-1, 16)
    return np.ascontiguousarray(np.stack([proj[:, 0], -proj[:, 5], -proj[:, 2], -proj[:, 6]], axis=1), np.float32)


def choose_in_box(choose: np.ndarray, width: int, box) -> np.ndarray:
    """``pt_choose`` (...,) re-indexed inside the integer box ``(x0, y0, x1, y1)``
    (inclusive corners, as ``bbox_2d``): ``(y - y0) * (x1 - x0 + 1) + (x - x0)`` as
    int64, which is the ``choose`` of a loader that crops the image to the box
    first.  -1 for a pixel outside the box and for an empty slot's samples."""
    choose = np.asarray(choose).astype(np.int64)
    x0, y0, x1, y1 = (int(v) for v in box)
    y, x = np.divmod(choose, int(width))
    inside = (choose != EMPTY_CHOOSE) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    return np.where(inside, (y - y0) * (x1 - x0 + 1) + (x - x0), -1)


def to_object_frame(pt_coords: np.ndarray, lo, hi) -> np.ndarray:
    """``pt_coords`` (..., 3) uint16 in metres in the object's frame, float64:
    ``lo + q / 65535 * (hi - lo)`` with the object's box corners ``lo``, ``hi``
    (3,) (the dequantisation of ``labels.decode_obj_coords``).  An empty
    slot's zeros map to ``lo``: mask them with ``pt_count`` first."""
    from .labels import decode_obj_coords
    return decode_obj_coords(pt_coords, lo, hi)
