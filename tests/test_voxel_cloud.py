"""csg_voxel_cloud (include/csg_api.h) restated in NumPy, and the
properties of the definition checked on the restatement: frac is exact and in
[0, 1) (but for t in (-0.5, 0), where it is rounded and q clamped), q <= 65535, the order rule, the rounding of the means, the 64-bit sum
of a frame in one voxel, and the centroid's distance from the float64 mean.
Then the host side: the PLY form and its inverse, the header text, the
exports, the ABI version, the loaded library's entry point and the generator's
output kind.  tests/test_gpu_voxel_cloud.py compares the GPU with
:func:`restate_voxels` bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from constructionsceneposeestimation_amd import voxel_cloud as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = 0x7FC00000
OVERFLOW = 0xFFFFFFFF
F32 = np.float32
SHAPES = [(1, 1), (3, 5), (64, 64), (131, 517), (240, 320)]


def cells_and_q(points, s):
    """Per point and axis: t = fl32(p * fl32(1 / s)), c = floorf(t), frac = t - c, q, and `inside` (t
    finite and c in [-2^17, 2^17) on every axis).  ``points`` (P, 3) float32, all finite."""
    r = F32(1.0) / F32(s)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (points.astype(F32) * r).astype(F32)
        c = np.floor(t)
        inside = (np.isfinite(t) & (c >= F32(-131072.0)) & (c < F32(131072.0))).all(axis=1)
        frac = (t - c).astype(F32)
        q = np.minimum(np.where(inside[:, None], frac * F32(65536.0), 0).astype(np.uint32), 65535)
    return t, c, frac, q, inside


def restate_frame(points, rgb, ids, L, s, C_):
    """One frame by the definition -> dict(vx_xyz (C, 3) float32, vx_rgb (C, 3) uint8, vx_label (C,) int32,
    vx_count (C,) uint32, total, dropped); the rows are None where the frame overflows."""
    P = points.shape[0] * points.shape[1]
    p = np.ascontiguousarray(points, F32).reshape(P, 3)
    col = np.zeros((P, 3), np.uint8) if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(P, 3)
    idv = np.full(P, -1, np.int64) if ids is None else np.asarray(ids).reshape(P).astype(np.int64)
    Lx = 0 if ids is None else int(L)
    is_point = np.isfinite(p).all(axis=1) & (idv >= -1) & (idv < Lx)
    pix = np.flatnonzero(is_point)
    t, c, frac, q, inside = cells_and_q(p[pix], s)
    dropped = int((~inside).sum())
    pix, c, q = pix[inside], c[inside].astype(np.int64), q[inside].astype(np.uint64)
    key = ((c[:, 0] + 131072) << 45) | ((c[:, 1] + 131072) << 27) | ((c[:, 2] + 131072) << 9) | (idv[pix] + 1)
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)   # first: lowest pixel (pix ascends)
    V = len(uniq)
    out = dict(total=V if V <= C_ else OVERFLOW, dropped=dropped, vx_xyz=None, vx_rgb=None, vx_label=None,
               vx_count=None)
    if V > C_:
        return out
    order = np.argsort(first, kind="stable")          # ascending by the voxel's lowest row-major pixel
    rank = np.empty(V, np.int64)
    rank[order] = np.arange(V)
    slot = rank[inv.reshape(-1)]
    n = np.bincount(slot, minlength=V).astype(np.uint64)
    S = np.zeros((V, 3), np.uint64)
    R = np.zeros((V, 3), np.uint64)
    for a in range(3):
        np.add.at(S[:, a], slot, q[:, a])
        np.add.at(R[:, a], slot, col[pix, a].astype(np.uint64))
    m = (2 * S + n[:, None]) // (2 * n[:, None])
    cell = np.empty((V, 3), np.int64)
    cell[slot] = c
    lab = np.empty(V, np.int64)
    lab[slot] = idv[pix]
    xyz = np.full((C_, 3), 0, np.uint32)
    xyz[:] = NAN_BITS
    xyz = xyz.view(F32)
    inner = ((m.astype(F32) + F32(0.5)) * (F32(1.0) / F32(65536.0))).astype(F32)
    xyz[:V] = ((cell.astype(F32) + inner).astype(F32) * F32(s)).astype(F32)
    out["vx_xyz"] = xyz
    out["vx_rgb"] = np.zeros((C_, 3), np.uint8)
    out["vx_rgb"][:V] = ((2 * R + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    out["vx_label"] = np.full(C_, -1, np.int32)
    out["vx_label"][:V] = lab
    out["vx_count"] = np.zeros(C_, np.uint32)
    out["vx_count"][:V] = n
    return out


def restate_voxels(points, rgb, ids, L, s, C_):
    """A batch: ``points`` (n, H, W, 3), ``rgb`` (n, H, W, 3) or None, ``ids`` (n, H, W) or None -> a list of
    :func:`restate_frame` results."""
    return [restate_frame(points[f], None if rgb is None else rgb[f], None if ids is None else ids[f], L, s, C_)
            for f in range(points.shape[0])]


def records_of(fr):
    """A restated frame as voxel_cloud.RECORD_DTYPE records (what voxel_cloud_host and the PLY hold)."""
    V = fr["total"]
    rec = np.empty(V, vc.RECORD_DTYPE)
    rec["xyz"].view(np.uint32)[...] = fr["vx_xyz"][:V].view(np.uint32)
    rec["rgb"], rec["label"], rec["count"] = fr["vx_rgb"][:V], fr["vx_label"][:V], fr["vx_count"][:V]
    return rec


def same_records(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# -- synthetic frames shared with the GPU test ----------------------------------------------------------

def random_cloud(n, H, W, L, rng, extent=1.5, bad=True):
    """Points around the origin (negative cells), ids in [-1, L) with some outside that range, random colours;
    with ``bad`` a sprinkle of NaN, +-inf and 1e7 coordinates."""
    pts = rng.uniform(-extent, extent, (n, H, W, 3)).astype(F32)
    if bad and H * W >= 4:
        k = max(1, H * W // 16)
        for val in (np.nan, np.inf, -np.inf, 1e7, -1e7):
            f, y, x, a = rng.integers(0, n, k), rng.integers(0, H, k), rng.integers(0, W, k), rng.integers(0, 3, k)
            pts[f, y, x, a] = val
    ids = rng.integers(-1, L, (n, H, W)).astype(np.int32)
    if bad:
        out = rng.random((n, H, W)) < 0.05
        ids[out] = rng.choice(np.array([-2, L, L + 1, -2 ** 31, 2 ** 31 - 1], np.int64), int(out.sum())).astype(np.int32)
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return pts, rgb, ids


def one_voxel_frame(H, W, s=0.05):
    """Every pixel in one voxel, frac near 1 on every axis."""
    pts = np.empty((H, W, 3), F32)
    pts[...] = F32(3 * s) - F32(s) * F32(2.0 ** -12) * (1 + (np.arange(H * W).reshape(H, W, 1) % 3)).astype(F32)
    return pts


# -- the definition's properties ------------------------------------------------------------------------

def test_frac_is_exact_and_q_fits_16_bits():
    rng = np.random.default_rng(1)
    for s in (0.05, 0.1, 0.013, 1.0, 7.5):
        p = np.concatenate([rng.uniform(-3, 3, (4000, 3)), rng.uniform(-1500, 1500, (4000, 3)),
                            np.arange(-30, 30)[:, None] * np.float64(F32(s)) * np.ones(3)]).astype(F32)
        t, c, frac, q, inside = cells_and_q(p, s)
        assert inside.all()
        exact = frac.astype(np.float64) == t.astype(np.float64) - c.astype(np.float64)
        rounds = (t > F32(-0.5)) & (t < 0)          # c = -1 and t + 1 needs a bit below the ulp of [0.5, 1)
        assert exact[~rounds].all() and (c[rounds] == -1).all()
        assert (np.abs(frac.astype(np.float64) - (t.astype(np.float64) + 1))[rounds] <= 2.0 ** -25).all()
        assert (frac >= 0).all() and (frac[~rounds] < 1).all() and (frac <= 1).all()
        assert q.max() <= 65535 and (q == np.minimum(np.floor(frac.astype(np.float64) * 65536), 65535)).all()
    # the one value the rounding can reach: t just below zero gives frac = 1.0, and q is clamped
    t, c, frac, q, inside = cells_and_q(np.array([[-1e-9, -0.3, -2.0 ** -27 * 0.05]], F32), 0.05)
    assert inside.all() and (c[0, ::2] == -1).all() and (frac[0, ::2] == 1.0).all() and q[0, ::2].tolist() == [65535] * 2
    assert c[0, 1] == -6 and 0 <= frac[0, 1] < 1
    # floor, not truncation, below zero; and the far cells are dropped
    t, c, frac, q, inside = cells_and_q(np.array([[-0.01, 0.01, -0.05 * 3]], F32), 0.05)
    assert c[0, 0] == -1 and c[0, 1] == 0 and c[0, 2] in (-3, -4)
    far = np.array([[1e7, 0, 0], [0, -1e7, 0], [3e38, 0, 0], [0.05 * 131071.5, 0, 0], [-0.05 * 131071.5, 0, 0]], F32)
    assert cells_and_q(far, 0.05)[4].tolist() == [False, False, False, True, True]


def test_order_is_by_lowest_pixel_and_labels_never_merge():
    s = 0.5
    pts = np.full((2, 4, 3), np.nan, F32)
    ids = np.zeros((2, 4), np.int32)
    #            pixel: 0 cell B   1 cell A    2 cell B (label 1)  3 NaN
    pts[0, 0], pts[0, 1], pts[0, 2] = (1.1, 0.1, 0.1), (0.1, 0.1, 0.1), (1.2, 0.2, 0.2)
    ids[0] = [0, 0, 1, 0]
    #            pixel: 4 cell A   5 cell B    6 id out of range   7 cell A, background
    pts[1, 0], pts[1, 1], pts[1, 2], pts[1, 3] = (0.3, 0.3, 0.3), (1.3, 0.3, 0.3), (0.1, 0.1, 0.1), (0.2, 0.2, 0.2)
    ids[1] = [0, 0, 2, -1]
    fr = restate_frame(pts, None, ids, 2, s, 8)
    assert fr["total"] == 4 and fr["dropped"] == 0
    assert fr["vx_label"].tolist() == [0, 0, 1, -1, -1, -1, -1, -1]
    assert fr["vx_count"].tolist() == [2, 2, 1, 1, 0, 0, 0, 0]
    assert vc.cell_of(fr["vx_xyz"][:4], s).tolist() == [[2, 0, 0], [0, 0, 0], [2, 0, 0], [0, 0, 0]]
    assert (fr["vx_xyz"][4:].view(np.uint32) == NAN_BITS).all() and not fr["vx_rgb"].any()
    assert restate_frame(pts, None, ids, 2, s, 3)["total"] == OVERFLOW
    assert restate_frame(pts, None, ids, 2, s, 4)["total"] == 4
    no_ids = restate_frame(pts, None, None, 2, s, 8)      # every id is -1: cell A and cell B, nothing else
    assert no_ids["total"] == 2 and no_ids["vx_count"][:2].tolist() == [3, 4] and (no_ids["vx_label"] == -1).all()


def test_means_round_half_up_in_integers():
    s = 1.0
    # q of these fracs: 0, 1, 1 -> S = 2, n = 3: m = (4 + 3) // 6 = 1; and 0, 0, 1 -> S = 1: m = (2 + 3) // 6 = 0
    u = 1.0 / 65536
    pts = np.array([[[0.0, 0.0, 5.0], [u, 0.0, 5.0], [u, u, 5.0]]], F32)
    rgb = np.array([[[0, 1, 255], [1, 1, 255], [1, 2, 254]]], np.uint8)    # R = 2, 4, 764 over n = 3
    fr = restate_frame(pts, rgb, None, 0, s, 1)
    assert fr["total"] == 1 and fr["vx_count"][0] == 3
    assert fr["vx_rgb"][0].tolist() == [(4 + 3) // 6, (8 + 3) // 6, (1528 + 3) // 6] == [1, 1, 255]
    exp = [F32(0) + (F32(1) + F32(0.5)) * F32(u), F32(0) + (F32(0) + F32(0.5)) * F32(u), F32(5) + F32(0.5) * F32(u)]
    assert fr["vx_xyz"][0].tolist() == [float(F32(e)) for e in exp]
    # a tie rounds up: q = 0 and 1, n = 2: (2 + 2) // 4 = 1
    fr = restate_frame(np.array([[[0.0, 0.0, 0.0], [u, 0.0, 0.0]]], F32), np.array([[[0, 0, 0], [1, 0, 0]]], np.uint8),
                       None, 0, s, 1)
    assert fr["vx_xyz"][0, 0] == F32(1.5) * F32(u) and fr["vx_rgb"][0, 0] == 1


def test_one_voxel_frame_needs_more_than_32_bits():
    H, W, s = 240, 320, 0.05
    pts = one_voxel_frame(H, W, s)
    t, c, frac, q, inside = cells_and_q(pts.reshape(-1, 3), s)
    assert inside.all() and (c == 2).all() and q.min() >= 65000
    S = q.astype(np.uint64).sum(axis=0)
    assert (S > 2 ** 32).all()
    fr = restate_frame(pts, None, None, 0, s, 1)
    assert fr["total"] == 1 and fr["vx_count"][0] == H * W
    m = (2 * S + H * W) // (2 * H * W)
    wrong = (2 * (S % 2 ** 32) + H * W) // (2 * H * W)      # what 32-bit sums would give
    assert (m != wrong).all()
    assert fr["vx_xyz"][0].tolist() == [float(F32(F32(F32(2) + F32((F32(v) + F32(0.5)) * F32(2.0 ** -16))) * F32(s)))
                                        for v in m]


def test_centroid_is_near_the_float64_mean_on_a_smooth_surface():
    s = 0.05
    H, W = 96, 128
    y, x = np.mgrid[0:H, 0:W]
    u, v = (x - W / 2) * 0.004, (y - H / 2) * 0.004
    pts = np.stack([1.2 + u, -1.1 + v, 1.1 + 0.3 * u - 0.2 * v + 0.05 * np.sin(9 * u)], axis=-1).astype(F32)
    fr = restate_frame(pts, None, None, 0, s, H * W)
    V = fr["total"]
    assert 100 < V < H * W // 4
    p = pts.reshape(-1, 3)
    cell = vc.cell_of(p, s)
    key = [tuple(k) for k in cell.tolist()]
    groups = {}
    for i, k in enumerate(key):
        groups.setdefault(k, []).append(i)
    order = sorted(groups.values(), key=lambda g: g[0])
    assert len(order) == V
    worst = 0.0
    for k, g in enumerate(order):
        mean = p[g].astype(np.float64).mean(axis=0)
        bound = s / 65536 + 4 * float(np.spacing(F32(np.linalg.norm(mean))))
        err = np.abs(fr["vx_xyz"][k].astype(np.float64) - mean)
        worst = max(worst, float(err.max()))
        assert (err <= bound).all(), (k, err, bound)
        assert fr["vx_count"][k] == len(g)
    assert worst > 0


def test_dropped_points_are_counted_and_not_binned():
    rng = np.random.default_rng(5)
    pts, rgb, ids = random_cloud(1, 131, 517, 4, rng)
    fr = restate_frame(pts[0], rgb[0], ids[0], 4, 0.05, 131 * 517)
    p = pts[0].reshape(-1, 3)
    isp = np.isfinite(p).all(axis=1) & (ids[0].reshape(-1) >= -1) & (ids[0].reshape(-1) < 4)
    far = isp & (np.abs(p) > 1e6).any(axis=1)
    assert fr["dropped"] == int(far.sum()) > 0
    assert int(fr["vx_count"].sum()) == int(isp.sum()) - fr["dropped"]
    assert np.isfinite(fr["vx_xyz"][:fr["total"]]).all() and fr["vx_label"][:fr["total"]].min() >= -1


# -- the PLY form -----------------------------------------------------------------------------------------

def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    pts, rgb, ids = random_cloud(1, 64, 64, 7, rng)
    rec = records_of(restate_frame(pts[0], rgb[0], ids[0], 7, 0.1, 4096))
    assert len(rec) > 100 and rec.dtype == vc.RECORD_DTYPE
    data = vc.ply_bytes(rec)
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
            b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty int label\n"
            b"property uint count\nend_header\n" % len(rec))
    assert data.startswith(head) and len(data) == len(head) + 23 * len(rec)
    assert same_records(vc.read_ply(data), rec) and same_records(vc.read_ply(bytearray(data)), rec)
    path = tmp_path / "voxels_000000.ply"
    path.write_bytes(data)
    assert same_records(vc.read_ply(str(path)), rec) and same_records(vc.read_ply(path), rec)
    first = np.frombuffer(data[len(head):len(head) + 23], vc.PLY_DTYPE)[0]
    assert (first["x"], first["y"], first["z"]) == tuple(rec["xyz"][0]) and first["label"] == rec["label"][0]
    assert first["count"] == rec["count"][0] and (first["red"], first["green"], first["blue"]) == tuple(rec["rgb"][0])
    empty = vc.ply_bytes(np.empty(0, vc.RECORD_DTYPE))      # a frame with no voxel
    assert empty.endswith(b"end_header\n") and b"element vertex 0\n" in empty and len(vc.read_ply(empty)) == 0
    for bad in (data[:-1], data + b"\0", b"ply\nend_header\n", b"not a ply", data.replace(b"int label", b"int thing")):
        with pytest.raises(ValueError):
            vc.read_ply(bad)


def test_cell_of_is_the_pass_rule():
    p = np.array([[-0.01, 0.0, 0.049999], [0.05, 0.1, -0.1], [1e3, -1e3, 2.5]], F32)
    t, c, _, _, _ = cells_and_q(p, 0.05)
    assert np.array_equal(vc.cell_of(p, 0.05), c.astype(np.int32)) and vc.cell_of(p, 0.05).dtype == np.int32
    assert vc.cell_of(p[0], 0.05).tolist() == [-1, 0, 0]


# -- header, exports, library, generator ----------------------------------------------------------------

def test_header_exports_and_abi():
    from constructionsceneposeestimation_amd import _lib
    text = open(os.path.join(ROOT, "include", "csg_api.h")).read()
    assert re.search(r"#define CSG_ABI_VERSION 14\b", text) and _lib.ABI_VERSION == 14
    for name in ("csg_voxel_cloud", "csg_keep_points", "csg_last_points"):
        assert name in _lib.EXPORTED and re.search(r"\bint %s\(csg_ctx\* ctx" % name, text), name
    assert "int csg_voxel_cloud(csg_ctx* ctx, const csg_voxel_job* job, uint32_t n_frames, void* stream);" in text
    for phrase in ("A pixel is a point iff its three coordinates are finite and -1 <= id < L",
                   "r = fl32(1.0f / s), computed once on the host.",
                   "q_a = min((uint32)(frac_a * 65536.0f), 65535), which lies in [0, 65535].",
                   "m_a = (2 * S_a + n) / (2n), in integer arithmetic.",
                   "vx_xyz_a = fl32(fl32((float)c_a + fl32(((float)m_a + 0.5f) * (1.0f / 65536.0f))) * s).",
                   "V > C: vx_total[f] = 0xFFFFFFFF."):
        assert phrase in text, phrase
    fields = [f for f, _ in _lib.VoxelJob._fields_]
    assert fields == ["width", "height", "n_labels", "capacity", "voxel_size", "pad", "points", "rgb", "instance",
                      "vx_xyz", "vx_rgb", "vx_label", "vx_count", "vx_total", "vx_dropped"]
    assert C.sizeof(_lib.VoxelJob) == 24 + 9 * 8
    struct = text[text.index("typedef struct {", text.index("Voxel-downsampled labelled point clouds")):
                  text.index("} csg_voxel_job;")]
    # the header's fields, in order, as the binding's
    names = re.findall(r"(\w+)(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    assert [n for pair in names for n in pair if n] == fields


def test_library_has_the_entry_points():
    from constructionsceneposeestimation_amd import _lib
    lib = _lib.load()
    job = _lib.VoxelJob()
    assert lib.csg_voxel_cloud(None, C.byref(job), 1, None) == -1      # a null context: CSG_ERR_INVALID
    assert lib.csg_keep_points(None, 1) == -1
    p, nf = C.c_void_p(), C.c_uint32()
    assert lib.csg_last_points(None, C.byref(p), C.byref(nf)) == -1


def test_generator_knows_the_output():
    from constructionsceneposeestimation_amd.generate import (OUTPUTS, REFERENCE_OUTPUTS, file_path, main,
                                                              parse_outputs)
    assert "pointcloud_voxel_ply" in OUTPUTS and parse_outputs("all") == OUTPUTS
    assert parse_outputs("reference") == REFERENCE_OUTPUTS == ("rgb", "mask", "depth_csv", "depth_png", "pointcloud")
    assert parse_outputs("rgb,mask,pointcloud_voxel_ply") == ("rgb", "mask", "pointcloud_voxel_ply")
    assert file_path("/d", "pointcloud_voxel_ply", 12) == os.path.join("/d", "pointcloud", "voxels_000012.ply")
    with pytest.raises(ValueError):
        parse_outputs("bop,pointcloud_voxel_ply")
    with pytest.raises(SystemExit):
        main(["--out", "/nonexistent", "--outputs", "pointcloud_voxel"])
    assert vc.DEFAULT_VOXEL_SIZE == 0.05 and vc.DEFAULT_VOXEL_CAPACITY == 262144
