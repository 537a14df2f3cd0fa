"""ctypes binding of libcsgio.so (include/csg_io.h): native writers of the
generator's on-disk formats (generate_construction_data.py: PNG :1672-1673,
``.npy`` :2066-2069, depth CSV :1688, point-cloud TXT :769-770).

Each call encodes and writes one file with the GIL released, so a thread
pool of writers runs in parallel with the GPU rendering the next batch.  The
text formats are byte-identical to the ``np.savetxt`` calls of the reference.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .build import IO_LIB, build_io, needs_build, IO_DEPS

ABI_VERSION = 6  # CSGIO_ABI_VERSION in include/csg_io.h
EXPORTED = ("csgio_abi_version", "csgio_write_png_rgb", "csgio_write_npy", "csgio_write_depth_csv",
            "csgio_write_pointcloud_txt", "csgio_depth_stats", "csgio_write_label_json", "csgio_spans_to_rle",
            "csgio_write_coco_fragment", "csgio_write_coco_fragment_amodal")
PNG_STRATEGY = {"default": 0, "rle": 1, "huffman": 2}
_lib: Optional[C.CDLL] = None


class CsgIoError(OSError):
    pass


class Label(C.Structure):   # csgio_label
    _fields_ = [("frame_id", C.c_uint32), ("height", C.c_uint32), ("width", C.c_uint32),
                ("n_objects", C.c_uint32), ("n_labels", C.c_uint32), ("n_kp", C.c_uint32),
                ("camera_pose", C.c_void_p), ("camera_params", C.c_char_p), ("class_mapping", C.c_char_p),
                ("obj_head", C.c_void_p), ("obj_label", C.c_void_p), ("obj_kp_off", C.c_void_p),
                ("obj_kp", C.c_void_p), ("inst_stats", C.c_void_p), ("covered", C.c_void_p),
                ("kp_uv", C.c_void_p), ("kp_vis", C.c_void_p), ("kp_name", C.c_void_p),
                ("obj_listed", C.c_void_p)]


class Coco(C.Structure):   # csgio_coco
    _fields_ = [("frame_id", C.c_uint32), ("height", C.c_uint32), ("width", C.c_uint32),
                ("n_objects", C.c_uint32), ("n_labels", C.c_uint32), ("n_kp", C.c_uint32),
                ("obj_label", C.c_void_p), ("obj_class", C.c_void_p), ("obj_path", C.c_void_p),
                ("obj_kp_off", C.c_void_p), ("obj_kp", C.c_void_p), ("inst_stats", C.c_void_p),
                ("spans", C.c_void_p), ("span_offsets", C.c_void_p), ("kp_uv", C.c_void_p), ("kp_vis", C.c_void_p)]


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if needs_build(IO_LIB, IO_DEPS):
        try:
            build_io()
        except Exception as e:  # pragma: no cover - surfaced below
            if not os.path.exists(IO_LIB):
                raise CsgIoError(f"libcsgio.so missing and could not be built: {e}") from e
    lib = C.CDLL(IO_LIB)
    vp, u32, u64, cp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_char_p
    lib.csgio_abi_version.argtypes = []
    lib.csgio_write_png_rgb.argtypes = [cp, vp, u32, u32, C.c_int, C.c_int]
    lib.csgio_depth_stats.argtypes = [vp, u64, vp]
    lib.csgio_write_npy.argtypes = [cp, vp, u64, cp, vp, u32]
    lib.csgio_write_depth_csv.argtypes = [cp, vp, u32, u32]
    lib.csgio_write_pointcloud_txt.argtypes = [cp, vp, vp, u64]
    lib.csgio_write_label_json.argtypes = [cp, C.POINTER(Label)]
    lib.csgio_spans_to_rle.argtypes = [vp, vp, u32, u32, u32, vp, u64, vp, vp, u64, vp]
    lib.csgio_write_coco_fragment.argtypes = [cp, C.POINTER(Coco)]
    lib.csgio_write_coco_fragment_amodal.argtypes = [cp, C.POINTER(Coco), vp, vp, vp]
    if lib.csgio_abi_version() != ABI_VERSION:
        raise CsgIoError(f"libcsgio.so ABI {lib.csgio_abi_version()} != binding ABI {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def _check(rc: int, what: str, path: str) -> None:
    if rc != 0:
        raise CsgIoError(-rc, f"{what} failed: {os.strerror(-rc)}", path)


def write_png(path: str, rgb: np.ndarray, level: int = 1, strategy: str = "default") -> None:
    a = np.ascontiguousarray(rgb, np.uint8)
    assert a.ndim == 3 and a.shape[2] == 3, a.shape
    _check(load().csgio_write_png_rgb(path.encode(), a.ctypes.data, a.shape[1], a.shape[0], level,
                                      PNG_STRATEGY[strategy]), "write_png", path)


def depth_stats(depth: np.ndarray) -> dict:
    """Counts of one depth image in one native pass (GIL released):
    valid (finite, > 0), zero and infinite pixels, sum / min / max of the valid."""
    a = np.ascontiguousarray(depth, np.float32)
    out = np.zeros(6, np.float64)
    _check(load().csgio_depth_stats(a.ctypes.data, a.size, out.ctypes.data), "depth_stats", "")
    return {"valid": int(out[0]), "zero": int(out[1]), "inf": int(out[2]), "total": int(a.size),
            "sum": float(out[3]), "min": float(out[4]), "max": float(out[5])}


def write_npy(path: str, arr: np.ndarray) -> None:
    a = np.ascontiguousarray(arr)
    descr = np.lib.format.dtype_to_descr(a.dtype)
    shape = (C.c_uint64 * max(a.ndim, 1))(*a.shape)
    _check(load().csgio_write_npy(path.encode(), a.ctypes.data, a.nbytes, descr.encode(), shape, a.ndim),
           "write_npy", path)


def write_depth_csv(path: str, depth: np.ndarray) -> None:
    a = np.ascontiguousarray(depth, np.float32)
    _check(load().csgio_write_depth_csv(path.encode(), a.ctypes.data, a.shape[1], a.shape[0]), "write_depth_csv", path)


def write_pointcloud_txt(path: str, points: np.ndarray, rgb: np.ndarray) -> None:
    """``points`` (..., 3) float32 world xyz (NaN = no hit), ``rgb`` (..., 3) uint8."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    assert p.shape == c.shape
    _check(load().csgio_write_pointcloud_txt(path.encode(), p.ctypes.data, c.ctypes.data, p.shape[0]),
           "write_pointcloud_txt", path)


# -- the compact kinds (no reference counterpart): binary PLY, 16-bit depth PNG ------
PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
assert PLY_DTYPE.itemsize == 15


def ply_header(n: int) -> bytes:
    """Header of a binary PLY of ``n`` points (CSG_FILE_POINTCLOUD_PLY, include/csg_api.h)."""
    return (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
            b"property float x\nproperty float y\nproperty float z\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % n)


def pointcloud_ply_bytes(points: np.ndarray, rgb: np.ndarray) -> bytes:
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    assert p.shape == c.shape
    keep = ~np.isnan(p).any(axis=1)   # the TXT writer's rule: a point has no NaN in x, y, z
    rec = np.empty(int(keep.sum()), PLY_DTYPE)
    # (bit copies: the float fields are assigned as uint32 views, so -0.0 and NaN payloads survive)
    bits = p[keep].view(np.uint32)
    for k, name in enumerate(("x", "y", "z")):
        rec[name].view(np.uint32)[...] = bits[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rec[name] = c[keep, k]
    return ply_header(rec.shape[0]) + rec.tobytes()


def write_pointcloud_ply(path: str, points: np.ndarray, rgb: np.ndarray) -> None:
    """The point cloud as a binary PLY, 15 bytes per point: ``points`` (..., 3)
    float32 world xyz (NaN = no hit), ``rgb`` (..., 3) uint8; row-major."""
    with open(path, "wb") as fh:
        fh.write(pointcloud_ply_bytes(points, rgb))


def depth_to_u16(depth: np.ndarray, counts_per_metre: float = 250.0) -> np.ndarray:
    """The 16-bit depth sample of CSG_FILE_DEPTH16_PNG, in float32 throughout:
    0 where the depth is not finite or <= 0; else t = d * s (rounded to
    float32), 65535 where t >= 65535, else the integer part of t + 0.5
    (rounded to float32).  A valid depth below half a count reads 0 like "no
    hit"; depths beyond 65535 / s saturate."""
    d = np.asarray(depth, np.float32)
    s = np.float32(counts_per_metre)
    ok = np.isfinite(d) & (d > 0)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.where(ok, d, np.float32(0)) * s
        sat = t >= np.float32(65535)
        v = (np.where(sat, np.float32(0), t) + np.float32(0.5)).astype(np.uint32)
    return np.where(sat, 65535, v).astype(np.uint16)


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    import struct
    import zlib
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def depth16_png_bytes(u16: np.ndarray, level: int = 1) -> bytes:
    """A 16-bit greyscale PNG (bit depth 16, colour type 0) of an (H, W) uint16
    array: filter Sub on every row (distance 2 bytes), one IDAT chunk."""
    import struct
    import zlib
    a = np.ascontiguousarray(u16, np.uint16)
    assert a.ndim == 2, a.shape
    H, W = a.shape
    raw = a.astype(">u2").view(np.uint8).reshape(H, 2 * W)
    filt = np.empty((H, 2 * W + 1), np.uint8)
    filt[:, 0] = 1
    filt[:, 1:3] = raw[:, :2]
    filt[:, 3:] = raw[:, 2:] - raw[:, :-2]
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16, 0, 0, 0, 0))
            + _png_chunk(b"IDAT", zlib.compress(filt.tobytes(), level)) + _png_chunk(b"IEND", b""))


def write_depth16_png(path: str, depth: np.ndarray, counts_per_metre: float = 250.0) -> None:
    """``depth`` (H, W) float32 metres as a 16-bit PNG at ``counts_per_metre`` (:func:`depth_to_u16`)."""
    with open(path, "wb") as fh:
        fh.write(depth16_png_bytes(depth_to_u16(depth, counts_per_metre)))


MASK_PNG_IDAT_BYTES = 2048   # dfl::kIdatBytes: zlib bytes per IDAT chunk of a mask PNG


def _fixed_code(sym: int):
    """(code, bits) of literal / length symbol ``sym`` in deflate's fixed
    Huffman code (RFC 1951 3.2.6), the code bit-reversed for LSB-first output."""
    if sym < 144:
        v, n = 0x30 + sym, 8
    elif sym < 256:
        v, n = 0x190 + sym - 144, 9
    elif sym < 280:
        v, n = sym - 256, 7
    else:
        v, n = 0xC0 + sym - 280, 8
    return int(format(v, f"0{n}b")[::-1], 2), n


def _length_token(length: int):
    """(value, bits) of a distance-1 match of ``length`` 3..258: the fixed code
    of its length symbol, the extra bits, and the 5-bit distance code 0."""
    if length <= 10:
        sym, ne, ex = 254 + length, 0, 0
    elif length == 258:
        sym, ne, ex = 285, 0, 0
    else:
        l = length - 3
        ne = l.bit_length() - 3
        sym, ex = 257 + 4 * ne + 4 + (l >> ne) - 4, l & ((1 << ne) - 1)
    code, n = _fixed_code(sym)
    return code | (ex << n), n + ne + 5


def mask_png_bytes(mask: np.ndarray) -> bytes:
    """The mask PNG of csg_encode_span_masks (``Renderer.mask_pngs_host``), byte
    for byte, of an (H, W) mask (non-zero = 255): an 8-bit grey PNG, filter 0
    on every row, whose zlib stream is ``78 01``, ONE fixed-Huffman deflate
    block and the Adler-32, cut into IDAT chunks of 2048 bytes.  Each row's
    1 + W bytes are tokenised on their own: every maximal run of equal bytes
    (the filter byte joins a leading run of zeros) is one literal, distance-1
    matches of at most 258 bytes and a remainder below 3 bytes as literals;
    one end-of-block code follows the last row.  Plain Python, for tests and
    readers of the format (csrc/csg_mask_png.h is the native statement)."""
    import struct
    import zlib
    m = np.asarray(mask)
    assert m.ndim == 2 and m.shape[0] >= 1 and m.shape[1] >= 1, m.shape
    H, W = m.shape
    raw = np.zeros((H, W + 1), np.uint8)
    raw[:, 1:] = np.where(m != 0, 255, 0)
    lit = {0: _fixed_code(0), 255: _fixed_code(255)}
    acc, nbits = 0x0178 | (0b011 << 16), 19          # 78 01, BFINAL = 1, BTYPE = 01
    z = bytearray()

    def put(value_bits):
        nonlocal acc, nbits
        acc |= value_bits[0] << nbits
        nbits += value_bits[1]

    for row in raw:
        z += (acc & ((1 << (nbits & ~7)) - 1)).to_bytes(nbits >> 3, "little")   # the whole bytes so far
        acc, nbits = acc >> (nbits & ~7), nbits & 7
        cuts = np.flatnonzero(row[1:] != row[:-1]) + 1
        starts = np.concatenate([[0], cuts])
        for s, e in zip(starts.tolist(), np.concatenate([cuts, [W + 1]]).tolist()):
            b, rem = int(row[s]), e - s - 1
            put(lit[b])
            while rem >= 3:
                n = min(rem, 258)
                put(_length_token(n))
                rem -= n
            for _ in range(rem):
                put(lit[b])
    put(_fixed_code(256))
    z = bytes(z) + acc.to_bytes((nbits + 7) // 8, "little") + struct.pack(">I", zlib.adler32(raw.tobytes()) & 0xFFFFFFFF)
    idat = b"".join(_png_chunk(b"IDAT", z[k:k + MASK_PNG_IDAT_BYTES]) for k in range(0, len(z), MASK_PNG_IDAT_BYTES))
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0, 0, 0, 0)) + idat
            + _png_chunk(b"IEND", b""))


def spans_to_rle(spans: np.ndarray, offsets: np.ndarray, height: int, width: int):
    """One frame's mask spans (``Renderer.mask_spans``: ``spans`` (total, 2)
    uint32 start / len, ``offsets`` (L + 1,) uint32) as COCO run-length masks,
    natively with the GIL released (csgio_spans_to_rle; ``masks.spans_to_counts``
    and ``masks.counts_to_string`` are its NumPy restatement).  Returns
    ``(counts, counts_off, string, string_off)``: label l's counts are
    ``counts[counts_off[l]:counts_off[l + 1]]`` (uint32) and its compressed
    string ``string[string_off[l]:string_off[l + 1]]`` (bytes); labels without
    spans have empty ranges."""
    off = np.ascontiguousarray(offsets, np.uint32).reshape(-1)
    L = off.shape[0] - 1
    total = int(off[L])
    sp = np.ascontiguousarray(spans, np.uint32).reshape(-1, 2)
    if L < 0 or sp.shape[0] < total:
        raise CsgIoError(f"spans_to_rle: {sp.shape[0]} spans, offsets end at {total}")
    n_counts = 2 * total + L + 1          # at most 2 k + 1 counts for a label's k spans
    counts = np.empty(n_counts, np.uint32)
    text = np.empty(6 * n_counts, np.uint8)  # a count (or its difference) has at most 6 groups of 5 bits
    c_off = np.zeros(L + 1, np.uint64)
    s_off = np.zeros(L + 1, np.uint64)
    _check(load().csgio_spans_to_rle(sp.ctypes.data, off.ctypes.data, L, int(height), int(width), counts.ctypes.data,
                                     counts.shape[0], c_off.ctypes.data, text.ctypes.data, text.shape[0],
                                     s_off.ctypes.data), "spans_to_rle", "")
    return counts[:int(c_off[L])], c_off, text[:int(s_off[L])].tobytes(), s_off


class LabelWriter:
    """Label files written natively (csgio_write_label_json, GIL released):
    byte-identical to ``save_label_json(label_record(...))`` (labels.py) for
    one workload's keypoint table and camera intrinsics.  The fixed JSON
    pieces are rendered once (per workload; object poses once per epoch) with
    the same encoder that writes the Python path."""

    def __init__(self, kp_table, camera_params: dict, n_labels: int, height: int, width: int):
        from .identity import CONSTRUCTION_CLASS
        from .labels import label_json_bytes
        self._enc = label_json_bytes
        self.height, self.width, self.n_labels = int(height), int(width), int(n_labels)
        self.camera_params = label_json_bytes(camera_params).replace(b"\n", b"\n  ")
        self.class_mapping = label_json_bytes(dict(CONSTRUCTION_CLASS)).replace(b"\n", b"\n  ")
        names = [label_json_bytes(n) for _, n in kp_table]
        self._names = names
        self.kp_name = (C.c_char_p * max(len(names), 1))(*names)
        self.n_kp = len(names)
        n_obj = max([j for j, _ in kp_table] + [-1]) + 1
        self._kp_by_obj = [[] for _ in range(n_obj)]
        for k, (j, _) in enumerate(kp_table):
            self._kp_by_obj[j].append(k)
        self._epochs = {}

    def epoch(self, e: int, poses):
        """The per-epoch pieces for ``object_poses`` of epoch e (cached)."""
        hit = self._epochs.get(e)
        if hit is not None:
            return hit
        heads = []
        for p in poses:
            t = self._enc(p)                       # {\n  "inst_idx": ..\n}
            heads.append(b"    " + t[2:-2].replace(b"\n", b"\n    "))
        n = len(poses)
        kp_lists = [self._kp_by_obj[j] if j < len(self._kp_by_obj) else [] for j in range(n)]
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(x) for x in kp_lists])
        idx = np.array([k for x in kp_lists for k in x] or [0], np.uint32)
        labels = np.array([p["inst_idx"] for p in poses] or [0], np.int32)
        labels = np.where(labels < 0, labels + self.n_labels, labels).astype(np.int32)   # Python indexing
        st = {"heads": heads, "head_arr": (C.c_char_p * max(n, 1))(*heads), "n": n, "off": off, "idx": idx,
              "labels": labels}
        if len(self._epochs) >= 64:
            self._epochs.pop(next(iter(self._epochs)))
        self._epochs[e] = st
        return st

    def n_visible(self, ep: dict, inst_stats: np.ndarray, listed: Optional[np.ndarray] = None) -> int:
        """Objects the label file lists: those with visible pixels (and, with
        ``listed``, those flagged there; labels.label_record's rule)."""
        lab = ep["labels"][:ep["n"]]
        ok = (lab >= 0) & (lab < inst_stats.shape[0])
        vis = np.zeros(ep["n"], bool)
        vis[ok] = inst_stats[lab[ok], 0] != 0
        if listed is not None:
            vis |= ok & np.asarray(listed, bool)[:ep["n"]]
        return int(np.count_nonzero(vis))

    def write(self, path: str, frame_id: int, camera_pose, ep: dict, inst_stats: np.ndarray,
              covered: Optional[np.ndarray], kp_uv: np.ndarray, kp_vis: np.ndarray,
              listed: Optional[np.ndarray] = None) -> None:
        pose = np.ascontiguousarray(np.asarray(camera_pose, np.float64).reshape(7))
        st = np.ascontiguousarray(inst_stats, np.uint32)
        cv = np.ascontiguousarray(covered, np.uint32) if covered is not None else None
        uv = np.ascontiguousarray(kp_uv, np.float32)
        vis = np.ascontiguousarray(kp_vis, np.int32)
        lst = np.ascontiguousarray(listed, np.uint8) if listed is not None else None
        if lst is not None and lst.shape[0] < ep["n"]:
            raise CsgIoError(f"write_label_json: listed has {lst.shape[0]} entries, {ep['n']} objects")
        L = Label(int(frame_id), self.height, self.width, ep["n"], st.shape[0], self.n_kp, pose.ctypes.data,
                  self.camera_params, self.class_mapping, C.cast(ep["head_arr"], C.c_void_p).value,
                  ep["labels"].ctypes.data, ep["off"].ctypes.data, ep["idx"].ctypes.data, st.ctypes.data,
                  cv.ctypes.data if cv is not None else None, uv.ctypes.data, vis.ctypes.data,
                  C.cast(self.kp_name, C.c_void_p).value, lst.ctypes.data if lst is not None else None)
        _check(load().csgio_write_label_json(path.encode(), C.byref(L)), "write_label_json", path)


class FragmentWriter:
    """COCO fragments written natively (csgio_write_coco_fragment, GIL
    released): byte-identical to ``masks.write_fragment`` for one scene's
    objects (``poses`` of any epoch, labels.object_poses: inst_idx, class_id and
    prim_path do not change between epochs) and keypoint table."""

    def __init__(self, poses, kp_table, height: int, width: int):
        import json
        self.height, self.width = int(height), int(width)
        n = len(poses)
        self.n = n
        self.labels = np.array([p["inst_idx"] for p in poses] or [0], np.int32)
        self.classes = np.array([p["class_id"] for p in poses] or [0], np.int32)
        self._paths = [json.dumps(p["prim_path"], ensure_ascii=False).encode("utf-8") for p in poses]
        self.paths = (C.c_char_p * max(n, 1))(*self._paths)
        by = [[] for _ in range(n)]
        for k, (j, _) in enumerate(kp_table):
            if j < n:
                by[j].append(k)
        self.n_kp = len(kp_table)
        self.kp_off = np.zeros(n + 1, np.uint32)
        self.kp_off[1:] = np.cumsum([len(x) for x in by])
        self.kp_idx = np.array([k for x in by for k in x] or [0], np.uint32)

    def write(self, path: str, frame_id: int, inst_stats: np.ndarray, spans: np.ndarray, offsets: np.ndarray,
              kp_uv: Optional[np.ndarray] = None, kp_vis: Optional[np.ndarray] = None,
              amodal_spans: Optional[np.ndarray] = None, amodal_offsets: Optional[np.ndarray] = None,
              amodal_stats: Optional[np.ndarray] = None) -> None:
        """With the three amodal arrays (one frame of ``Renderer.amodal_spans``)
        the fragment carries the amodal keys of ``masks.coco_fragment``
        (csgio_write_coco_fragment_amodal)."""
        st = np.ascontiguousarray(inst_stats, np.uint32)
        off = np.ascontiguousarray(offsets, np.uint32).reshape(-1)
        sp = np.ascontiguousarray(spans, np.uint32).reshape(-1, 2)
        if off.shape[0] != st.shape[0] + 1 or sp.shape[0] < int(off[-1]):
            raise CsgIoError(f"write_coco_fragment: {st.shape[0]} labels, {off.shape[0]} offsets, {sp.shape[0]} spans")
        n_kp = self.n_kp if kp_uv is not None and kp_vis is not None else 0
        uv = np.ascontiguousarray(kp_uv, np.float32) if n_kp else None
        vis = np.ascontiguousarray(kp_vis, np.int32) if n_kp else None
        if n_kp and (uv.size < 2 * n_kp or vis.size < n_kp):
            raise CsgIoError(f"write_coco_fragment: {n_kp} keypoints in the table, {vis.size} in the frame")
        F = Coco(int(frame_id), self.height, self.width, self.n, st.shape[0], n_kp, self.labels.ctypes.data,
                 self.classes.ctypes.data, C.cast(self.paths, C.c_void_p).value, self.kp_off.ctypes.data,
                 self.kp_idx.ctypes.data, st.ctypes.data, sp.ctypes.data if sp.size else None, off.ctypes.data,
                 uv.ctypes.data if n_kp else None, vis.ctypes.data if n_kp else None)
        if amodal_spans is None and amodal_offsets is None and amodal_stats is None:
            _check(load().csgio_write_coco_fragment(path.encode(), C.byref(F)), "write_coco_fragment", path)
            return
        if amodal_spans is None or amodal_offsets is None or amodal_stats is None:
            raise CsgIoError("write_coco_fragment: amodal_spans, amodal_offsets and amodal_stats go together")
        ast = np.ascontiguousarray(amodal_stats, np.uint32)
        aoff = np.ascontiguousarray(amodal_offsets, np.uint32).reshape(-1)
        asp = np.ascontiguousarray(amodal_spans, np.uint32).reshape(-1, 2)
        if ast.shape != st.shape or aoff.shape[0] != off.shape[0] or asp.shape[0] < int(aoff[-1]):
            raise CsgIoError(f"write_coco_fragment: amodal arrays of {ast.shape[0]} labels, {aoff.shape[0]} offsets, "
                             f"{asp.shape[0]} spans")
        _check(load().csgio_write_coco_fragment_amodal(path.encode(), C.byref(F), ast.ctypes.data,
                                                       asp.ctypes.data if asp.size else None, aoff.ctypes.data),
               "write_coco_fragment_amodal", path)


# ---- baseline JPEG (csrc/csg_jpeg.h) ----------------------------------------------------

JPEG_SUBSAMPLING = {"444": 0, "420": 1}
JPEG_HEAD_BYTES = 629       # jpg::kHeadBytes: SOI .. SOS header
JPEG_DCT_SHIFT = 20         # jpg::kDctShift: jpeg_fdct's results are coefficients * 2^20
JPEG_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                        13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                        45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
_JPEG_BASE_Q = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
     87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
     72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99]
    + [99] * 36])
_JPEG_DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
_JPEG_AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
_JPEG_AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    bytes.fromhex(
    "0001020311040521310612415107617113223281081442 91a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
_JPEG_K = (None, 8035, 7568, 6811, 5793, 4551, 3135, 1598)   # round(2^14 * cos(j pi / 16) / 2)


def jpeg_quant_tables(quality: int) -> np.ndarray:
    """(2, 64) luminance and chrominance quantisers in zig-zag order: Annex K
    scaled by libjpeg's quality rule."""
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"jpeg quality {quality} outside 1..100")
    s = 5000 // int(quality) if quality < 50 else 200 - 2 * int(quality)
    return np.clip((_JPEG_BASE_Q * s + 50) // 100, 1, 255)[:, JPEG_ZIGZAG]


def _jpeg_canonical(bits, vals):
    codes, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            codes[vals[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    return codes


def jpeg_huffman_codes():
    """[(dc, ac)] for the luminance and the chrominance tables of Annex K.3:
    dicts symbol -> (code, bits)."""
    return [(_jpeg_canonical(_JPEG_DC_BITS[c], bytes(range(12))), _jpeg_canonical(_JPEG_AC_BITS[c], _JPEG_AC_VALS[c]))
            for c in range(2)]


def _jpeg_dct8(a: np.ndarray, rnd: int, shift: int) -> np.ndarray:
    """jpg::dct8 along the last axis of an int64 array."""
    _, k1, k2, k3, k4, k5, k6, k7 = _JPEG_K
    s = a[..., :4] + a[..., :3:-1]
    d = a[..., :4] - a[..., :3:-1]
    s0, s1, s2, s3 = (s[..., i] for i in range(4))
    d0, d1, d2, d3 = (d[..., i] for i in range(4))
    out = np.stack([k4 * (s0 + s1 + s2 + s3),
                    k1 * d0 + k3 * d1 + k5 * d2 + k7 * d3,
                    k2 * (s0 - s3) + k6 * (s1 - s2),
                    k3 * d0 - k7 * d1 - k1 * d2 - k5 * d3,
                    k4 * (s0 - s1 - s2 + s3),
                    k5 * d0 - k1 * d1 + k7 * d2 + k3 * d3,
                    k6 * (s0 - s3) - k2 * (s1 - s2),
                    k7 * d0 - k5 * d1 + k3 * d2 - k1 * d3], axis=-1)
    return (out + rnd) >> shift


def jpeg_fdct(blocks: np.ndarray) -> np.ndarray:
    """jpg::fdct8x8 of (..., 8, 8) level-shifted integer samples: int64
    coefficients * 2^JPEG_DCT_SHIFT, [..., v, u]."""
    t = _jpeg_dct8(np.asarray(blocks).astype(np.int64), 128, 8)                        # rows
    return np.swapaxes(_jpeg_dct8(np.swapaxes(t, -1, -2), 0, 0), -1, -2)              # columns


def jpeg_ycc(rgb: np.ndarray):
    """jpg::ycc of an (..., 3) uint8 array: int64 Y, Cb, Cr in 0..255."""
    r, g, b = (np.asarray(rgb)[..., i].astype(np.int64) for i in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
            (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16)


def jpeg_samples(rgb: np.ndarray, subsampling: str = "420"):
    """The level-shifted sample blocks of an (H, W, 3) uint8 image in the
    scan's order: int64 (MCU rows, blocks per row, 8, 8), and the component
    (0 Y, 1 Cb, 2 Cr) of each block of a row."""
    sub = JPEG_SUBSAMPLING[str(subsampling)]
    H, W = rgb.shape[:2]
    m = 16 if sub else 8
    my, mx = -(-H // m), -(-W // m)
    ext = np.pad(rgb, ((0, my * m - H), (0, mx * m - W), (0, 0)), mode="edge")
    planes = [p - 128 for p in jpeg_ycc(ext)]

    def cut(p):   # (rows of blocks, blocks, 8, 8)
        return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).swapaxes(1, 2)

    if sub:
        y = cut(planes[0]).reshape(my, 2, mx, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my, mx, 4, 8, 8)
        c = [cut(((p + 128).reshape(my * 8, 2, mx * 8, 2).sum(axis=(1, 3)) + 2 >> 2) - 128) for p in planes[1:]]
        blocks = np.concatenate([y, c[0][:, :, None], c[1][:, :, None]], axis=2)
        comp = [0, 0, 0, 0, 1, 2]
    else:
        blocks = np.stack([cut(p) for p in planes], axis=2)
        comp = [0, 1, 2]
    return blocks.reshape(my, mx * len(comp), 8, 8), np.array(comp * mx)


def jpeg_coefficients(rgb: np.ndarray, quality: int = 95, subsampling: str = "420"):
    """The quantised coefficients of jpeg_bytes in the scan's order: int64
    (MCU rows, blocks per row, 64) in zig-zag order with the DC absolute, and
    each block's component."""
    blocks, comp = jpeg_samples(rgb, subsampling)
    F = jpeg_fdct(blocks).reshape(*blocks.shape[:2], 64)[..., JPEG_ZIGZAG]
    d = jpeg_quant_tables(quality)[np.minimum(comp, 1)].astype(np.int64) << JPEG_DCT_SHIFT   # (blocks, 64)
    q = np.sign(F) * ((np.abs(F) + (d >> 1)) // d)
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    if JPEG_SUBSAMPLING[str(subsampling)]:
        # a luminance block with no pixel of the image repeats the DC of the block before it in its MCU
        # and has no AC (jpg::luma_source)
        H, W = rgb.shape[:2]
        mcu = q.reshape(q.shape[0], -1, 6, 64)
        col = (np.arange(mcu.shape[1]) * 16 + 8 < W)[None, :]
        row = (np.arange(mcu.shape[0]) * 16 + 8 < H)[:, None]
        s1 = np.where(col, 1, 0) + np.zeros_like(row, int)
        source = {1: s1, 2: np.where(row, 2, s1), 3: np.where(row, np.where(col, 3, 2), s1)}
        dc = mcu[..., 0].copy()
        for k, src in source.items():
            empty = src != k
            mcu[:, :, k][empty] = 0
            mcu[:, :, k, 0][empty] = np.take_along_axis(dc, src[..., None], 2)[..., 0][empty]
    return q, comp


def jpeg_header(width: int, height: int, quality: int = 95, subsampling: str = "420") -> bytes:
    """SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS header of jpeg_bytes."""
    import struct
    sub = JPEG_SUBSAMPLING[str(subsampling)]
    q = jpeg_quant_tables(quality)
    mx = -(-width // (16 if sub else 8))
    h = b"\xff\xd8\xff\xe0" + struct.pack(">H5sHBHHBB", 16, b"JFIF\0", 0x0101, 0, 1, 1, 0, 0)
    for c in range(2):
        h += b"\xff\xdb" + struct.pack(">HB", 67, c) + bytes(q[c].tolist())
    h += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, height, width, 3)
    h += bytes([1, 0x22 if sub else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for c in range(2):
        h += b"\xff\xc4" + struct.pack(">HB", 31, c) + bytes(_JPEG_DC_BITS[c]) + bytes(range(12))
        h += b"\xff\xc4" + struct.pack(">HB", 181, 0x10 | c) + bytes(_JPEG_AC_BITS[c]) + _JPEG_AC_VALS[c]
    h += b"\xff\xdd" + struct.pack(">HH", 4, mx)
    h += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(h) == JPEG_HEAD_BYTES
    return h


def jpeg_bytes(rgb: np.ndarray, quality: int = 95, subsampling: str = "420") -> bytes:
    """The JPEG of csg_encode_jpeg (``Renderer.jpegs_host``), byte for byte, of
    an (H, W, 3) uint8 image: a baseline JFIF file laid out as libjpeg writes
    one with a restart interval per MCU row, Y Cb Cr in one scan at 4:4:4 or
    4:2:0, Annex K's tables at libjpeg's quality scaling, and the integer
    colour conversion, chroma mean, DCT and quantiser of csrc/csg_jpeg.h (the
    native statement).  NumPy and plain Python, for tests, the CPU writer path
    and readers of the format."""
    a = np.asarray(rgb)
    if a.dtype != np.uint8:
        raise TypeError(f"jpeg_bytes: image of {a.dtype}, not uint8")
    if a.ndim != 3 or a.shape[2] != 3 or not (1 <= a.shape[0] <= 8192 and 1 <= a.shape[1] <= 8192):
        raise ValueError(f"jpeg_bytes: image of shape {a.shape}, not (H, W, 3) with H, W in 1..8192")
    if str(subsampling) not in JPEG_SUBSAMPLING:
        raise ValueError(f"jpeg_bytes: subsampling {subsampling!r} is neither '444' nor '420'")
    H, W = a.shape[:2]
    out = bytearray(jpeg_header(W, H, quality, subsampling))
    coef, comp = jpeg_coefficients(a, quality, subsampling)
    codes = jpeg_huffman_codes()
    n_comp = 3
    for r in range(coef.shape[0]):
        acc, nbits = 0, 0
        pred = [0] * n_comp
        for zz, c in zip(coef[r].tolist(), comp.tolist()):
            dc, ac = codes[min(c, 1)]
            diff = max(-2047, min(2047, zz[0] - pred[c]))
            pred[c] = zz[0]
            s = abs(diff).bit_length()
            code, n = dc[s]
            acc = (((acc << n) | code) << s) | ((diff - 1 if diff < 0 else diff) & ((1 << s) - 1))
            nbits += n + s
            run = 0
            for v in zz[1:]:
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    code, n = ac[0xF0]
                    acc = (acc << n) | code
                    nbits += n
                    run -= 16
                s = abs(v).bit_length()
                code, n = ac[(run << 4) | s]
                acc = (((acc << n) | code) << s) | ((v - 1 if v < 0 else v) & ((1 << s) - 1))
                nbits += n + s
                run = 0
            if run:
                code, n = ac[0]
                acc = (acc << n) | code
                nbits += n
        pad = -nbits % 8
        data = ((acc << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big")
        out += data.replace(b"\xff", b"\xff\x00")
        if r + 1 < coef.shape[0]:
            out += bytes([0xFF, 0xD0 + (r & 7)])
    return bytes(out + b"\xff\xd9")


def write_jpeg(path: str, rgb: np.ndarray, quality: int = 95, subsampling: str = "420") -> None:
    """``jpeg_bytes`` of an (H, W, 3) uint8 image to ``path`` (the generator's writer processes)."""
    with open(path, "wb") as fh:
        fh.write(jpeg_bytes(rgb, quality, subsampling))
