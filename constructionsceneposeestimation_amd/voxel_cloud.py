"""Voxel-downsampled labelled point clouds, host side: what goes with the
records of ``csg_voxel_cloud`` (include/csg_api.h), which are made on the GPU
(:meth:`renderer.Renderer.voxel_cloud`, :meth:`renderer.Renderer.voxel_cloud_host`,
``--outputs pointcloud_voxel_ply``).

A frame's records are a structured array of :data:`RECORD_DTYPE`: ``xyz`` the
voxel's centroid in the world (metres), ``rgb`` its mean colour, ``label`` the
``inst_idx`` its points carry in the mask (-1: background; points of two labels
never share a record) and ``count`` the pixels it stands for.  The grid is
fixed in the world, so records of different frames line up: :func:`cell_of`
gives the cell of a centroid.  The file form is a binary little-endian PLY of
23 bytes per record.
"""
from __future__ import annotations

import os
from typing import Union

import numpy as np

# one record in memory (Renderer.voxel_cloud_host) ...
RECORD_DTYPE = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3), ("label", "<i4"), ("count", "<u4")])
# ... and in the file
PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                      ("label", "<i4"), ("count", "<u4")])
assert RECORD_DTYPE.itemsize == 23 and PLY_DTYPE.itemsize == 23

OVERFLOW = 0xFFFFFFFF           # vx_total of a frame with more voxels than the capacity
DEFAULT_VOXEL_SIZE = 0.05       # metres
# Records per frame that Renderer.voxel_cloud_host starts with (it doubles on overflow, up to H * W)
DEFAULT_VOXEL_CAPACITY = 262144


def ply_header(n: int) -> bytes:
    """Header of a voxel PLY of ``n`` records, one property per line as CSG_FILE_POINTCLOUD_PLY's."""
    return (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
            b"property float x\nproperty float y\nproperty float z\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\n"
            b"property int label\nproperty uint count\nend_header\n" % n)


def ply_bytes(records: np.ndarray) -> bytes:
    """A frame's records (:data:`RECORD_DTYPE`) as a binary little-endian PLY:
    ``float x y z``, ``uchar red green blue``, ``int label``, ``uint count``,
    23 bytes per record, in the records' order.  The floats are copied bit for bit."""
    rec = np.ascontiguousarray(records, RECORD_DTYPE).reshape(-1)
    return ply_header(rec.size) + rec.tobytes()   # the two layouts are the same 23 bytes


def read_ply(path_or_bytes: Union[str, bytes, bytearray, memoryview, "os.PathLike"]) -> np.ndarray:
    """The inverse of :func:`ply_bytes`: the records (:data:`RECORD_DTYPE`) of a
    voxel PLY given as its bytes or its path."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("read_ply: not a PLY file")
    head = data[:end + 11]
    n = None
    for line in head.split(b"\n"):
        if line.startswith(b"element vertex "):
            n = int(line[15:])
    if n is None or head != ply_header(n):
        raise ValueError("read_ply: not a voxel PLY (x y z red green blue label count)")
    body = data[end + 11:]
    if len(body) != n * RECORD_DTYPE.itemsize:
        raise ValueError(f"read_ply: {len(body)} bytes of records, {n * RECORD_DTYPE.itemsize} expected")
    return np.frombuffer(body, RECORD_DTYPE).copy()


def cell_of(xyz: np.ndarray, voxel_size: float) -> np.ndarray:
    """The integer cell (..., 3) int32 of points ``xyz`` (..., 3) on the grid of
    ``voxel_size``, by the pass's own rule: ``floor(fl32(p * fl32(1 / s)))`` in
    float32.  This is the cell a point is binned in.  A record's centroid maps
    back to its voxel's cell unless it lies within float32 rounding of a cell
    face (the centroid is rounded three times on its way out)."""
    r = np.float32(1.0) / np.float32(voxel_size)
    t = np.asarray(xyz, np.float32) * r
    return np.floor(t).astype(np.int32)
