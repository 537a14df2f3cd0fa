"""CPU test of csg_alpha_box.h, the upload-time scan behind the alpha trim: a
stand-alone driver (tests/alpha_box_host.cpp, built with AddressSanitizer and
UBSan) computes the opaque uv box of seeded triangles, and a brute-force NumPy
scan of the same textures checks them:

* safe: the box holds every passing alpha quad whose cell lies within the guard
  band (2 texels, Chebyshev) of the uv triangle, widened by the 0.5-texel margin
  -- the scan may look at more quads than that, never fewer;
* not loose: the box lies inside that of the passing quads within the triangle's
  bounding rectangle dilated by the guard band;
* "full" exactly when the dilated texel box exceeds one repeat (or the
  coordinates leave +-2^22 texels), "empty" when no quad in reach passes.

Textures: 16 x 16, 13 x 7, 1 x 1 and 5 x 1; triangles inside one repeat, across
the seams, repeats away, of zero uv area (a point and a segment), and huge."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G, M = 2.0, 0.5


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("alpha_box") / "alpha_box_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "alpha_box_host.cpp"), "-o", out], check=True)
    return out


def _boxes(exe, alpha, thr, uv):
    h, w = alpha.shape
    text = [f"{w} {h} {thr} {len(uv)}", " ".join(str(int(a)) for a in alpha.reshape(-1))]
    text += [" ".join(f"{b:08x}" for b in t.reshape(-1).view(np.uint32)) for t in uv]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True)
    rows = [[int(x, 16) for x in line.split()] for line in r.stdout.splitlines()]
    return np.array(rows, np.uint32).view(np.float32)


def _passing(alpha, thr):
    q = np.maximum(np.maximum(alpha, np.roll(alpha, -1, 1)), np.roll(np.maximum(alpha, np.roll(alpha, -1, 1)), -1, 0))
    return q > thr


def _tri_hits_rect(tx, ty, x0, y0, x1, y1):
    """Separating axes: the triangle (tx, ty) against the rectangle [x0, x1] x [y0, y1], touching counts."""
    if tx.max() < x0 or tx.min() > x1 or ty.max() < y0 or ty.min() > y1:
        return False
    cx, cy = np.array([x0, x1, x1, x0]), np.array([y0, y0, y1, y1])
    for k in range(3):
        nx, ny = -(ty[(k + 1) % 3] - ty[k]), tx[(k + 1) % 3] - tx[k]
        a, b = nx * tx + ny * ty, nx * cx + ny * cy
        if a.max() < b.min() or a.min() > b.max():
            return False
    return True


def _reference(alpha, thr, uv):
    """(kind, inner, outer): kind "full" / "box"; inner and outer are quad boxes x0 x1 y0 y1 or None."""
    h, w = alpha.shape
    ok = _passing(alpha.astype(np.int64), thr)
    t = uv.astype(np.float64)
    tx, ty = t[:, 0] * w - 0.5, (1.0 - t[:, 1]) * h - 0.5
    if not (np.abs(tx) < 2.0 ** 22).all() or not (np.abs(ty) < 2.0 ** 22).all():
        return "full", None, None
    i0, i1 = int(np.floor(tx.min() - G)), int(np.floor(tx.max() + G))
    j0, j1 = int(np.floor(ty.min() - G)), int(np.floor(ty.max() + G))
    if i1 - i0 + 1 > w or j1 - j0 + 1 > h:
        return "full", None, None
    inner, outer = [], []
    for j in range(j0, j1 + 1):
        for i in range(i0, i1 + 1):
            if ok[j % h, i % w]:
                outer.append((i, j))
                if _tri_hits_rect(tx, ty, i - G, j - G, i + 1 + G, j + 1 + G):
                    inner.append((i, j))

    def box(q):
        if not q:
            return None
        q = np.array(q)
        return q[:, 0].min(), q[:, 0].max(), q[:, 1].min(), q[:, 1].max()
    return "box", box(inner), box(outer)


def _uv_box(q, w, h):
    x0, x1, y0, y1 = q
    return (x0 + 0.5 - M) / w, (x1 + 1.5 + M) / w, 1.0 - (y1 + 1.5 + M) / h, 1.0 - (y0 + 0.5 - M) / h


def _triangles(rng, w, h):
    n = 60
    small = rng.uniform(-0.3, 1.0, (n, 1, 2)) + rng.uniform(0.0, 1.0, (n, 3, 2)) * rng.uniform(0.0, 0.7, (n, 1, 2))
    away = small[:20] + rng.integers(-5000, 5000, (20, 1, 2))
    point = np.repeat(rng.uniform(-1.0, 2.0, (6, 1, 2)), 3, 1)                       # zero uv area: a point
    seg = rng.uniform(0.0, 0.4, (6, 1, 2)) + np.array([0.0, 0.5, 1.0])[None, :, None] * rng.uniform(0.0, 0.5, (6, 1, 2))
    huge = rng.uniform(-3.0, 3.0, (6, 3, 2))
    limit = np.array([[[0.0, 0.0], [0.1, 0.1], [2.0 ** 22 / w, 0.0]], [[0.0, -2.0 ** 23], [0.1, 0.1], [0.0, 0.2]]])
    nan = np.array([[[np.nan, 0.0], [0.1, 0.1], [0.2, 0.0]], [[0.0, 0.0], [np.inf, 0.1], [0.2, 0.0]]])
    return np.concatenate([small, away, point, seg, huge, limit, nan]).astype(np.float32)


@pytest.mark.parametrize("size", [(16, 16), (13, 7), (1, 1), (5, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("thr", [0, 127, 254])
def test_boxes_against_brute_force(exe, size, thr):
    w, h = size
    rng = np.random.default_rng(1000 * w + 10 * h + thr)
    kinds = {"full": 0, "empty": 0, "box": 0}
    for density in (0.0, 0.04, 0.5):
        alpha = np.where(rng.uniform(size=(h, w)) < density, rng.choice([thr + 1, 255], size=(h, w)),
                         rng.choice([0, thr], size=(h, w))).astype(np.uint8)
        uv = _triangles(rng, w, h)
        got = _boxes(exe, alpha, thr, uv)
        for t in range(len(uv)):
            kind, inner, outer = _reference(alpha, thr, uv[t])
            b = got[t].astype(np.float64)
            what = f"{w}x{h} thr {thr} density {density} triangle {t}: uv {uv[t].tolist()} box {b.tolist()}"
            if kind == "full":
                assert np.isinf(b).all() and b[0] < 0 < b[1] and b[2] < 0 < b[3], what
                kinds["full"] += 1
                continue
            assert not (np.isinf(b).all() and b[0] < b[1]), f"full, not expected: {what}"
            if outer is None:
                assert b[0] > b[1] and b[2] > b[3], f"empty expected: {what}"
            if b[0] > b[1]:                                    # empty: nothing in reach may pass
                assert inner is None, what
                kinds["empty"] += 1
                continue
            kinds["box"] += 1
            assert np.isfinite(b).all(), what
            if inner is not None:                              # safe
                lo = _uv_box(inner, w, h)
                assert b[0] <= lo[0] and b[1] >= lo[1] and b[2] <= lo[2] and b[3] >= lo[3], f"unsafe: {what}"
            hi = _uv_box(outer, w, h)                          # not loose (one float ulp of outward rounding)
            e = 1e-6 * (1.0 + np.abs(b).max())
            assert b[0] >= hi[0] - e and b[1] <= hi[1] + e and b[2] >= hi[2] - e and b[3] <= hi[3] + e, f"loose: {what}"
    if (w, h) == (16, 16):
        assert min(kinds.values()) > 0, kinds
