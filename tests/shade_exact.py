"""Scenes whose float32 depth, uv and shading arithmetic is exact, and their expected
images in integers and rationals.  It continues
tests/raster_exact.py, which pins coverage (items 3 and 4) the same way; nothing here
is shared with the oracle or the kernels (of the package only the scene model and
``packing.light_constants``, whose float32 constants are the light's inputs, are used).

* Camera: V = M = identity, P = ``raster_exact.projection`` (fx = fy = 256, integer
  cx, cy), near = 1/2, far = 256: both range bounds are powers of two.  (tests/pose_exact.py carries
  these frames into posed worlds: other V, M and P under which the same arithmetic stays exact.)
* A triangle is three 24.8 fixed-point screen vertices (U_k, V_k) on multiples of 16
  units, each with its own W_k = 2^j (1/4 .. 1024), and optionally uvs on multiples of
  1/256.  One edge is axis-aligned with length 2^p and the third vertex lies 2^q across
  it, so |2 area| = 2^(p+q) and ``det``, ``invdet`` are powers of two.  "Flat" triangles
  have one W, "tilted" ones up to three.
* ``planes_exact`` evaluates items 1, 2, 3, 5 and 6 in NumPy float32 in the written
  order and compares with rationals: the vertices are float32s, clip X, Y, W, the
  snapped vertices, the edge rows, det, invdet and the D, U, V planes are exact, and so
  are the three plane sums at every pixel centre of the frame.  The generators keep only
  triangles that pass (``assert_planes_exact`` for a whole frame).
* With exact planes 1/W at a centre is Z / 2^42 with an integer Z (``_grid_ints``), u/W
  likewise.  Only two steps round: depth = rn32(2^42 / Z), checked by integer
  cross-multiplication, and u = rn32((u/W) * depth), a product of two float32s, which a
  float64 holds exactly.  Texel coordinates, floor, wrap, 8-bit weights and the filter
  are integers on the exact value of t = u tw - 1/2 (40 fractional bits).
* ids: the largest Z among fragments that are covered (``raster_exact.edge_cover``),
  lie in 2^-8 <= 1/W <= 2 and pass their alpha test; a tie goes to the smaller
  ``instance << 20 | triangle``.
* The near plane (item 3).  A vertex may have W = +-2^j in front of the near plane
  (1/8, 1/4) or behind the camera (negative); it is then given by its virtual screen
  position, clip X = U W / 256 as before.  Clipping interpolates X and Y only; depth,
  uv, det and the normal come from the original triangle's edge rows, so ``planes_exact``
  and ``_grid_ints`` hold unchanged (the affine function that takes 1 / W_k at virtual
  vertex k is the D plane, whatever the signs).  ``clip_exact`` is Sutherland-Hodgman
  against W >= 1/2 in rationals over v0 -> v1, v1 -> v2, v2 -> v0 and the fan (q0, q_f,
  q_f+1).  tt = (near - Wa) / (Wb - Wa) is in general no float32, but the clip vertex is
  snapped to 24.8: a triangle is kept only if the exact 256 u and 256 v of every clip
  vertex lie MARGIN_Q away from a rounding tie and below 2^19 px, and the float32 chain
  in the written order snaps to the same integers.  Then the sub-triangles are integer
  triangles, and a clipped triangle covers the union of ``edge_cover`` of them (zero
  area drops one, negative area swaps), cut to 2^-8 <= 1/W <= 2 on the exact grid
  integers.  A vertex with W = 0 (``tri_w0``) has no virtual position: its planes come
  from the rational edge rows (``_grid_ints_w0``), with the same float32 check.
* Texture tables.  A frame may carry a per-material table (an index, -1, KEEP_TEXTURE)
  as ``csg_set_dr_textures`` takes it; ``render`` resolves every material through it, so
  size, wrap, weights and alpha are the swapped texture's.

Undecided fragments.  The kernels evaluate t in float32 (two or three roundings).  A
fragment whose exact 256 t lies within max(2^-12, the sum of those roundings' half ulps)
of an integer, in x or y, and whose float32 evaluation is not exact, may land on either
side of a weight step: its pixel is left out of the id / rgb / depth / normal / point
comparison, and its label out of the covered / amodal comparison at that pixel.  (The
half-ulp term exceeds 2^-12 from |t| = 8 on; leaving it out would compare pixels whose
weight the spec's own float32 arithmetic moves by one.)  Frames of flat triangles with
power-of-two textures have none: there the float32 evaluation is asserted exact.

Shading.  Per triangle and light, q = (int)((amb + sun c) 256 + 1/2) and the f16
normal are decided by exact comparison of squares (c^2 = (n.L)^2 / n.n over the
rationals, the light's float32 constants taken as rationals).  A triangle is kept only
if the true (amb + sun c) 256 + 1/2 is 2^-10 away from an integer, c is 2^-18 (relative)
away from a q step, every normal component is 2^-18 (relative) away from an f16 rounding
boundary, and the float32 cross product is within 2^-21 |n| of the true one: the eight
roundings after it (n.n twice, sqrt, n.L twice, the division, and the shade's two) stay
below 2^-19, so rgb and normals are determined.  Per size 101 tilted and 140 flat triangles
are kept, in both vertex orders; the generators rejected 167 candidates at 96 x 64 and 65 at
67 x 35 on one of these conditions or on ``planes_exact``.  The normal's sign is geometric here:
the output faces the camera (n . p0 < 0); tests/test_shade_exact.py asserts that this is
the spec's "flipped iff det > 0".

How close the depth cases get (power-of-two W and exact planes):
* ``cross`` holds pairs of nearly parallel triangles (the second is the first with its
  vertices moved by 1/16 or 1/8 px along the axis-aligned edge, unequally) that cross
  inside the frame with 1/W at most ``NEAR_ULPS`` = 8 float32 ulps apart at a common
  centre, beside pairs with their W exchanged, which cross steeply.
* ``range`` has centres at 1/W = 2^-8 exactly (kept) and, on triangles found by a seeded
  search, dropped centres at most ``FAR_ULPS`` = 64 float32 ulps below 2^-8.  That is the
  nearest the generator builds, not a limit of the construction; a centre exactly one ulp
  below along an axis-aligned gradient would need an edge of 2^19 px, whose clip X is no
  float32.

Families (``FAMILIES``; the generators' docstrings say what each aims at, and
tests/test_shade_exact.py counts that the aims occur): texel (and texel_npot, the 13 x 7
texture in a frame of its own, so that the power-of-two frame can be asserted exact),
thresh, persp, cross (and cross_near, the nearly parallel pairs), tie, range, light (one
frame per light set), trim, clip (clip, clip_edge, clip_tex, clip_pair: near-clipped
triangles) and swap (seven frames that draw the same instances under seven texture
tables).  Every frame
is generated in both vertex orders; all frames of one size are one scene, frame f drawing
its own instances (transform set f holds identity for them and the zero matrix for all
others; the swap frames of one order share theirs) under its own DR light and texture
table, with N_KP keypoints of its own.
"""
import functools
import math
from fractions import Fraction as Fr

import numpy as np

from tests.raster_exact import EMPTY, SIZES, area2, edge_cover, projection, stats_of   # noqa: F401

NEAR, FAR = 0.5, 256.0
N_LABELS = 6
N_KP = 8
UVQ = 256                  # uvs are multiples of 1 / 256
IWS = 4096                 # 1 / W = IW / 4096 with an integer IW: W = 1/4 .. 1024
PQ = 30                    # |2 area| = 2^pq, pq <= 30; 1 / W = Z / 2^ZS with Z = N << (PQ - pq)
ZS = 12 + PQ
Z_FAR, Z_NEAR = 1 << (ZS - 8), 1 << (ZS + 1)
TF = 40                    # fractional bits of the fixed-point texel arithmetic
EDGES = ((1, 2), (2, 0), (0, 1))
FAMILIES = ("texel", "thresh", "persp", "cross", "tie", "range", "light", "trim", "clip", "swap")
CLIP_GUARD = 1 << 27       # a clip vertex stays below 2^19 px
KEEP_TEXTURE = -2          # a texture table's "as authored"
MARGIN_Q = Fr(1, 1 << 10)
MARGIN_REL = Fr(1, 1 << 18)
NORMAL_COND = Fr(1, 1 << 21)
NEAR_ULPS = 8              # cross: two surfaces this many float32 ulps of 1 / W apart at a common centre
FAR_ULPS = 64              # range: a dropped centre this many ulps below 1 / far = 2^-8 (ulp 2^-32 there)


def tri(xy, w, uv=None, tag=None):
    """A triangle: fixed-point vertices, one W (a float) or three, uvs in 1/256 or None.  A vertex of W < near
    (negative included) is given by its virtual screen position, X W / 256 being its clip X; ``tag`` names the
    case a generator built it for (the tests count them)."""
    w = (w, w, w) if isinstance(w, (int, float)) else tuple(w)
    t = dict(xy=[None if v is None else (int(v[0]), int(v[1])) for v in xy], w=tuple(float(v) for v in w),
             uv=None if uv is None else [(int(a), int(b)) for a, b in uv])
    if tag is not None:
        t["tag"] = tag
    return t


def tri_w0(k, clip_xy, xy, w, tag=None):
    """A triangle whose vertex k lies in the camera's plane: W = 0, clip (X, Y) = ``clip_xy`` (integers; it
    has no screen position), the two others as in ``tri``.  No uvs."""
    xy, w = list(xy), list(w)
    xy.insert(k, None)
    w.insert(k, 0.0)
    t = tri(xy, w, None, tag)
    t["clip0"] = (int(clip_xy[0]), int(clip_xy[1]))
    return t


def swapped(t):
    """The other vertex order: vertices 1 and 2 exchanged."""
    s = lambda a: None if a is None else [a[0], a[2], a[1]]      # noqa: E731
    o = dict(xy=s(t["xy"]), w=tuple(s(list(t["w"]))), uv=s(t["uv"]))
    for key in ("tag", "clip0"):
        if key in t:
            o[key] = t[key]
    return o


def vertices(t, cx, cy):
    """(3, 3) float64 camera-space vertices: ((U - 256 cx) W / 65536, -(V - 256 cy) W / 65536, -W)."""
    return np.array([[t["clip0"][0] / 256.0, -t["clip0"][1] / 256.0, 0.0] if v is None else
                     [(v[0] - 256 * cx) * w / 65536.0, -(v[1] - 256 * cy) * w / 65536.0, -w] for v, w in zip(t["xy"], t["w"])])


def _grid_ints(t, Wd, Hd):
    """Exact planes on the grid of pixel centres -> N, NU, NV (H, W) int64 and pq, with 1 / W =
    N / 2^(12 + pq), u / W = NU / 2^(20 + pq), v / W likewise: barycentric numerators e_k (they add up
    to 2 area) weighted with IW_k = 4096 / W_k and the vertex uvs."""
    xy = t["xy"]
    if "clip0" in t:
        return _grid_ints_w0(t, Wd, Hd)
    a2 = area2(xy)
    pq = abs(a2).bit_length() - 1
    assert a2 != 0 and abs(a2) == 1 << pq and pq <= PQ, "2 area is not a power of two"
    s = 1 if a2 > 0 else -1
    X = np.arange(Wd, dtype=np.int64) * 256 + 128
    Y = np.arange(Hd, dtype=np.int64) * 256 + 128
    N = np.zeros((Hd, Wd), np.int64)
    NU, NV = N.copy(), N.copy()
    span = max(max(abs(c) for v in xy for c in v), 256 * max(Wd, Hd)) * 2     # bounds every coordinate difference: no int64 overflow
    for k, (a, b) in enumerate(EDGES):
        (xa, ya), (xb, yb) = xy[a], xy[b]
        iw = IWS / t["w"][k]
        assert iw == int(iw) and 4 <= abs(iw) <= 8 * IWS
        assert 2 * span * span * abs(int(iw)) * (1 if t["uv"] is None else max(1, max(abs(c) for c in t["uv"][k]))) < 1 << 60
        e = ((xa - X)[None, :] * (yb - Y)[:, None] - (xb - X)[None, :] * (ya - Y)[:, None]) * (s * int(iw))
        N += e
        if t["uv"] is not None:
            NU += e * t["uv"][k][0]
            NV += e * t["uv"][k][1]
    return N, NU, NV, pq


def _edge_rows(v):
    """The homogeneous edge rows A, B, C and det of clip vertices (X, Y, W), in rationals."""
    A = [v[a][1] * v[b][2] - v[a][2] * v[b][1] for a, b in EDGES]
    B = [v[a][2] * v[b][0] - v[a][0] * v[b][2] for a, b in EDGES]
    C = [v[a][0] * v[b][1] - v[a][1] * v[b][0] for a, b in EDGES]
    return A, B, C, v[0][0] * A[0] + v[0][1] * B[0] + v[0][2] * C[0]


def det_exact(t):
    """det of the clip matrix, a Fraction."""
    return _edge_rows(_clip_space(t))[3]


def _grid_ints_w0(t, Wd, Hd):
    """``_grid_ints`` for a triangle with a vertex of W = 0 (no virtual screen triangle to take barycentric
    numerators of): 1 / W = (sum A x + sum B y + sum C) / det from the rational edge rows, as N / 2^ZS, or
    None if that is no integer at some centre."""
    A, B, C, det = _edge_rows(_clip_space(t))
    da, db, dc = sum(A) / det, sum(B) / det, sum(C) / det
    n0, na, nb = (da / 2 + db / 2 + dc) * (1 << ZS), da * (1 << ZS), db * (1 << ZS)
    if any(n.denominator != 1 for n in (n0, na, nb)) or abs(n0) + abs(na) * Wd + abs(nb) * Hd >= 1 << 62:
        return None
    N = int(n0) + int(na) * np.arange(Wd, dtype=np.int64)[None, :] + int(nb) * np.arange(Hd, dtype=np.int64)[:, None]
    return N, np.zeros_like(N), np.zeros_like(N), PQ


def _eq_scaled(val32, num, shift):
    """float32 array == num / 2^shift (int64 num), decided in integers."""
    v = np.ldexp(val32.astype(np.float64), shift)
    ok = (np.abs(v) < 2.0 ** 62) & (v == np.floor(v))
    return bool(ok.all()) and bool(np.array_equal(v.astype(np.int64), num))


def planes_exact(t, Wd, Hd, cx, cy):
    """Whether spec 1, 2, 3, 5 and 6 are exact in float32 for this triangle (see the module docstring)."""
    f = np.float32
    p64 = vertices(t, cx, cy)
    p = p64.astype(f)
    if not np.array_equal(p.astype(np.float64), p64):
        return False
    P = projection(cx, cy).astype(f)
    with np.errstate(all="ignore"):
        X, Y, Wc = [((P[r, 0] * p[:, 0] + P[r, 1] * p[:, 1]) + P[r, 2] * p[:, 2]) + P[r, 3] for r in (0, 1, 3)]
        eX, eY, eW = ([v[c] for v in _clip_space(t)] for c in range(3))
        same = lambda got, want: all(np.isfinite(g) and Fr(float(g)) == e for g, e in zip(got, want))   # noqa: E731
        if not (same(X, eX) and same(Y, eY) and same(Wc, eW)):
            return False
        rw = f(1.0) / Wc
        su, sv = X * rw, Y * rw
        if any(v is not None and (int(np.rint(a * f(256.0))), int(np.rint(b * f(256.0)))) != v for a, b, v in zip(su, sv, t["xy"])):
            return False
        A = [Y[a] * Wc[b] - Wc[a] * Y[b] for a, b in EDGES]
        B = [Wc[a] * X[b] - X[a] * Wc[b] for a, b in EDGES]
        C = [X[a] * Y[b] - Y[a] * X[b] for a, b in EDGES]
        eA = [eY[a] * eW[b] - eW[a] * eY[b] for a, b in EDGES]
        eB = [eW[a] * eX[b] - eX[a] * eW[b] for a, b in EDGES]
        eC = [eX[a] * eY[b] - eY[a] * eX[b] for a, b in EDGES]
        if not (same(A, eA) and same(B, eB) and same(C, eC)):
            return False
        det = (X[0] * A[0] + Y[0] * B[0]) + Wc[0] * C[0]
        edet = eX[0] * eA[0] + eY[0] * eB[0] + eW[0] * eC[0]
        if edet == 0 or not same([det], [edet]):
            return False
        invdet = f(1.0) / det
        if not same([invdet], [1 / edet]):
            return False
        uv = [(f(1.0), f(1.0))] * 3 if t["uv"] is None else [(f(a / UVQ), f(b / UVQ)) for a, b in t["uv"]]
        euv = [(Fr(1), Fr(1))] * 3 if t["uv"] is None else [(Fr(a, UVQ), Fr(b, UVQ)) for a, b in t["uv"]]
        grid = _grid_ints(t, Wd, Hd)
        if grid is None:
            return False
        N, NU, NV, pq = grid
        x = (np.arange(Wd) + 0.5).astype(f)[None, :]
        y = (np.arange(Hd) + 0.5).astype(f)[:, None]
        for c, num, shift in ((None, N, 12 + pq), (0, NU, 20 + pq), (1, NV, 20 + pq)):
            if c is not None and t["uv"] is None:
                continue
            if c is None:
                pl = [((R[0] + R[1]) + R[2]) * invdet for R in (A, B, C)]
                epl = [(R[0] + R[1] + R[2]) / edet for R in (eA, eB, eC)]
            else:
                pl = [((R[0] * uv[0][c] + R[1] * uv[1][c]) + R[2] * uv[2][c]) * invdet for R in (A, B, C)]
                epl = [(R[0] * euv[0][c] + R[1] * euv[1][c] + R[2] * euv[2][c]) / edet for R in (eA, eB, eC)]
            if not same(pl, epl):
                return False
            val = (pl[0] * x + pl[1] * y) + pl[2]
            if val.dtype != f or not np.isfinite(val).all() or not _eq_scaled(val, num, shift):
                return False
    return True


def assert_planes_exact(tris, Wd, Hd, cx, cy):
    for k, t in enumerate(tris):
        assert planes_exact(t, Wd, Hd, cx, cy), f"triangle {k} is not exact: {t}"


# -- item 3: the near plane ------------------------------------------------------------------------------
def is_clipped(t):
    return min(t["w"]) < NEAR


def _clip_space(t):
    """Clip X, Y, W of the three vertices as Fractions."""
    return [(Fr(t["clip0"][0]), Fr(t["clip0"][1]), Fr(0)) if v is None else (Fr(v[0]) * Fr(w) / 256, Fr(v[1]) * Fr(w) / 256, Fr(w))
            for v, w in zip(t["xy"], t["w"])]


def _snap_clip_vertex(a, b):
    """The vertex where the edge a -> b (clip X, Y, W, Fractions) meets W = near, snapped to 24.8: the
    intersection in rationals, accepted only if 256 u and 256 v lie MARGIN_Q away from a rounding tie, below
    CLIP_GUARD, and the float32 chain in the written order (tt, a + tt (b - a), times 1 / near, times 256,
    rint) gives the same integers -> ((U, V), whether tt is a float32), or None."""
    f = np.float32
    near = Fr(NEAR)
    tt = (near - a[2]) / (b[2] - a[2])
    with np.errstate(all="ignore"):
        tt32 = (f(NEAR) - f(a[2])) / (f(b[2]) - f(a[2]))
        out = []
        for c in (0, 1):
            e = (a[c] + tt * (b[c] - a[c])) / near * 256
            fl = e.numerator // e.denominator
            if abs(e) >= CLIP_GUARD or abs(e - fl - Fr(1, 2)) < MARGIN_Q:
                return None
            n = (e + Fr(1, 2)).numerator // (e + Fr(1, 2)).denominator
            r = f(a[c]) + tt32 * (f(b[c]) - f(a[c]))
            got = np.rint((r * (f(1.0) / f(NEAR))) * f(256.0))
            if not np.isfinite(got) or int(got) != n:
                return None
            out.append(n)
    return tuple(out), Fr(float(tt32)) == tt


@functools.lru_cache(maxsize=None)
def _clip_key(xy, w, clip0):
    v = _clip_space(dict(xy=xy, w=w, clip0=clip0))
    inside = [p[2] >= Fr(NEAR) for p in v]
    poly, tt_exact, ends = [], [], []
    for k in range(3):                               # Sutherland-Hodgman over v0 -> v1, v1 -> v2, v2 -> v0
        a, b = k, (k + 1) % 3
        if inside[a]:
            poly.append(xy[a])
        if inside[a] != inside[b]:
            r = _snap_clip_vertex(v[a], v[b])
            if r is None:
                return None
            poly.append(r[0])
            tt_exact.append(r[1])
            ends.append((NEAR - w[a]) / (w[b] - w[a]))
    subs = [[poly[0], poly[j], poly[j + 1]] for j in range(1, len(poly) - 1)]          # the fan
    return dict(code=sum(int(s) << k for k, s in enumerate(inside)), poly=poly, subs=subs, tt_exact=tt_exact, tt=ends)


def clip_exact(t):
    """Item 3 on a triangle with a vertex of W < near, in rationals: dict(code: the inside mask, poly: the
    snapped polygon, subs: its fan (q0, q_f, q_f+1), zero-area ones included, tt, tt_exact per crossing), or
    None if a clip vertex is not decided (``_snap_clip_vertex``)."""
    if not is_clipped(t):                            # (nothing to intersect: no rationals needed)
        return dict(code=7, poly=list(t["xy"]), subs=[list(t["xy"])], tt_exact=[], tt=[])
    return _clip_key(tuple(t["xy"]), tuple(t["w"]), t.get("clip0"))


def cover_of(t, Wd, Hd):
    """The pixel centres a triangle's raster sub-triangles cover (items 3 and 4; no range test)."""
    if not is_clipped(t):
        return edge_cover(t["xy"], Wd, Hd)
    c = clip_exact(t)
    assert c is not None, "a clip vertex of a generated triangle is not decided"
    cov = np.zeros((Hd, Wd), bool)
    for s in c["subs"]:
        cov |= edge_cover(s, Wd, Hd)                  # (zero area covers nothing, negative area swaps)
    return cov


# -- the two rounding steps ----------------------------------------------------------------------------
def rn32_recip(Z):
    """rn32(2^ZS / Z) for positive int64 Z, as float32.  The candidate is a float64 quotient cast to float32;
    it is accepted only if |2^ZS - d Z| <= ulp(d) Z / 2 in Python integers (no tie can occur: a
    quotient 2^ZS / Z that lies halfway between two float32s would make Z a power of two, and then it is exact)."""
    d = (2.0 ** ZS / Z.astype(np.float64)).astype(np.float32)
    m, e = np.frexp(d.astype(np.float64))
    mi = np.ldexp(m, 24).astype(np.int64).astype(object)          # d = mi 2^(e - 24), 2^23 <= mi < 2^24
    sh = (e.astype(np.int64) - 24).astype(object)
    Zo = Z.astype(object)
    up = np.maximum(-sh, 0) + 1                                     # scale both sides to integers, times 2
    want, have = (1 << ZS) * (2 ** up), mi * Zo * 2 ** (sh + up)
    lhs = abs(want - have)                                          # 2^up |2^ZS - d Z|
    rhs = Zo * 2 ** (sh + up - 1)                                   # 2^up ulp(d) Z / 2, ulp(d) = 2^sh
    low = np.asarray((mi == 1 << 23) & (want < have), bool)         # below a power of two the step is half as wide
    good = np.asarray(lhs < rhs, bool) & (~low | np.asarray(2 * lhs < rhs, bool)) | np.asarray(lhs == 0, bool)
    assert good.all(), "depth is not the correctly rounded reciprocal"
    return d


def rn32(x):
    """A Fraction rounded to the nearest float32 (ties to even), as a Fraction; normal range only."""
    if x == 0:
        return Fr(0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fr(2) ** e > a:
        e -= 1
    assert -120 < e < 120
    ulp = Fr(2) ** (e - 23)
    k = a / ulp
    n = k.numerator // k.denominator
    r = k - n
    if r > Fr(1, 2) or (r == Fr(1, 2) and n % 2):
        n += 1
    return s * n * ulp


# -- item 6: texels ------------------------------------------------------------------------------------
def _to_fixed(a32):
    """float32 array -> (int64 a 2^TF, exact?)."""
    v = np.ldexp(a32.astype(np.float64), TF)
    ok = (v == np.floor(v)) & (np.abs(v) < 2.0 ** 50)
    return np.where(ok, v, 0.0).astype(np.int64), ok


def _axis(a32, ai, ok, n, chain32, extra_half_ulp):
    """One axis of item 6 on the exact a (u, or 1 - v): g = 256 (a n - 1/2) 2^TF -> texel, weight, undecided, exact."""
    one = 1 << TF
    g = ai * (n * 256) - 128 * one
    gi = g >> TF
    r = g & (one - 1)
    dist = np.minimum(r, one - r).astype(np.float64) / one
    a = np.abs(a32.astype(np.float64))
    t = np.abs(a * n - 0.5)
    f = np.float32
    half = lambda v: np.spacing(np.maximum(v, 2.0 ** -100).astype(f)).astype(np.float64) / 2     # noqa: E731
    err = half(a * n) + half(t) + extra_half_ulp * n
    c = np.ldexp(chain32.astype(np.float64), TF + 8)
    exact = ok & (np.abs(c) < 2.0 ** 62) & (c == np.floor(c))
    exact &= np.where(exact, c, 0.0).astype(np.int64) == g
    und = ~exact & ((dist <= np.maximum(2.0 ** -12, 256.0 * err)) | ~ok)
    return gi >> 8, gi & 255, und, exact, r


def sample(tex, u32, v32):
    """Item 6 on float32 (u, v) arrays -> (n, 4) int64 RGBA, undecided (n,), exact (n,) and a dict of
    per-fragment flags the tests count (aims)."""
    th, tw = tex.shape[:2]
    f = np.float32
    ui, uok = _to_fixed(u32)
    vi, vok = _to_fixed(v32)
    one = 1 << TF
    a_v32 = f(1.0) - v32
    inexact_a = np.ldexp(a_v32.astype(np.float64), TF) != (one - vi).astype(np.float64)
    half_a = np.where(inexact_a | ~vok, np.spacing(np.abs(a_v32)).astype(np.float64) / 2, 0.0)
    tx, wx, undx, exx, rx_ = _axis(u32, ui, uok, tw, u32 * f(tw) - f(0.5), 0.0)
    ty, wy, undy, exy, ry_ = _axis(a_v32, one - vi, vok, th, a_v32 * f(th) - f(0.5), half_a)
    x0, y0 = np.mod(tx, tw), np.mod(ty, th)
    x1, y1 = np.mod(x0 + 1, tw), np.mod(y0 + 1, th)
    T = tex.astype(np.int64)
    wx_, wy_ = wx[:, None], wy[:, None]
    top = T[y0, x0] * (256 - wx_) + T[y0, x1] * wx_
    bot = T[y1, x0] * (256 - wx_) + T[y1, x1] * wx_
    out = (top * (256 - wy_) + bot * wy_ + 32768) >> 16
    flags = dict(centre=(wx == 0) & (rx_ == 0) & (wy == 0) & (ry_ == 0), edge_x=(wx == 128) & (rx_ == 0),
                 edge_y=(wy == 128) & (ry_ == 0), seam_x=x0 == tw - 1, seam_y=y0 == th - 1,
                 neg_x=tx < 0, neg_y=ty < 0, far_x=np.abs(tx) >= 3 * tw, far_y=np.abs(ty) >= 3 * th,
                 texel=tx * 4096 + ty)
    return out, undx | undy, exx & exy, flags


# -- items 7 and 8: shading ------------------------------------------------------------------------------
def light_fractions(light):
    """(amb (3), sun (3), dir (3)) as Fractions of the float32 constants, and the sky colour (3 ints)."""
    from constructionsceneposeestimation_amd.packing import light_constants
    amb, sun, d, sky = light_constants(light)
    return ([Fr(float(v)) for v in amb], [Fr(float(v)) for v in sun], [Fr(float(v)) for v in d],
            [int(v) for v in sky[:3]])


def _cmp_sqrt(lo, c2, hi):
    """lo <= sqrt(c2) <= hi for rationals, by squares."""
    return (lo <= 0 or lo * lo <= c2) and hi >= 0 and c2 <= hi * hi


def _f16_bits(v2, sign, rel):
    """f16 bits of sign sqrt(v2) (+0 for 0), or None if sqrt(v2) is within ``rel`` of a rounding boundary."""
    if v2 == 0:
        return 0
    h = np.float16(math.sqrt(float(v2)))
    for cand in (h, np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(0))):
        lo = (Fr(float(cand)) + Fr(float(np.nextafter(cand, np.float16(-np.inf))))) / 2
        hi = (Fr(float(cand)) + Fr(float(np.nextafter(cand, np.float16(np.inf))))) / 2
        if _cmp_sqrt(lo, v2, hi):
            if not _cmp_sqrt(lo * (1 + rel), v2, hi * (1 - rel)):
                return None
            b = int(np.float16(cand).view(np.uint16))
            return b if b == 0 else b | (0x8000 if sign < 0 else 0)
    return None


def shade(t, cx, cy, consts):
    """Items 7 and 8 for one triangle under one light -> dict(q (3 ints), normal (3 uint16), flipped,
    det_positive), or None if a margin of the module docstring fails."""
    amb, sun, L, _ = consts
    p = [[Fr(v) for v in row] for row in vertices(t, cx, cy).tolist()]
    e1 = [p[1][i] - p[0][i] for i in range(3)]
    e2 = [p[2][i] - p[0][i] for i in range(3)]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    nn = sum(v * v for v in n)
    if nn == 0:
        return None
    f = np.float32
    pf = vertices(t, cx, cy).astype(f)
    a, b = pf[1] - pf[0], pf[2] - pf[0]
    nf = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    err2 = sum((Fr(float(g)) - v) ** 2 for g, v in zip(nf, n))
    if err2 > NORMAL_COND ** 2 * nn:                     # the float32 cross product is too far off
        return None
    flat = err2 == 0 and n[0] == 0 and n[1] == 0
    rel = Fr(0) if flat else MARGIN_REL                  # a flat normal is (0, 0, +-1) and c = |L_z|, exactly
    toward = sum(n[i] * p[0][i] for i in range(3))       # the camera is the origin: the output has out . p0 < 0
    if toward == 0:
        return None
    flip = toward > 0
    normal = []
    for v in n:
        bits = _f16_bits(v * v / nn, (-1 if flip else 1) * (1 if v > 0 else -1), rel)
        if bits is None:
            return None
        normal.append(bits)
    s = sum(n[i] * L[i] for i in range(3))
    c2 = s * s / nn
    c = math.sqrt(float(c2))
    q = []
    for k in range(3):
        val = float(amb[k]) + float(sun[k]) * c
        qk = math.floor(val * 256 + 0.5)
        if sun[k] == 0:
            exact = amb[k] * 256 + Fr(1, 2)
            if not qk + MARGIN_Q <= exact <= qk + 1 - MARGIN_Q:
                return None
        else:
            lo, hi = (Fr(qk) - Fr(1, 2) - 256 * amb[k]) / (256 * sun[k]), (Fr(qk) + Fr(1, 2) - 256 * amb[k]) / (256 * sun[k])
            m = MARGIN_Q / (256 * sun[k])
            if not (_cmp_sqrt(lo + m, c2, hi - m) and _cmp_sqrt(lo * (1 + rel), c2, hi * (1 - rel))):
                return None
        q.append(min(max(qk, 0), 65535))
    X, Y, Wc = ([v[c] for v in _clip_space(t)] for c in range(3))
    det = (X[0] * (Y[1] * Wc[2] - Wc[1] * Y[2]) + Y[0] * (Wc[1] * X[2] - X[1] * Wc[2])
           + Wc[0] * (X[1] * Y[2] - Y[1] * X[2]))
    return dict(q=q, normal=normal, flipped=flip, det_positive=det > 0, flat=flat)


# -- a frame's expected images -------------------------------------------------------------------------
def _base255(material):
    b = np.asarray(material.base_color, np.float64) * 255.0
    assert np.array_equal(b, np.rint(b))
    return b.astype(np.int64)


def render(insts, scene, light, Wd, Hd, cx, cy, first_instance, table=None):
    """The expected outputs of one frame.  ``insts``: [(label, material, [tri, ...])], drawn as the
    scene's instances first_instance, first_instance + 1, ...; ``table``: per material of the scene the
    texture this frame gives it (an index, -1 for none, KEEP_TEXTURE), or None for the authored ones."""
    consts = light_fractions(light)
    npx = Wd * Hd
    bestZ = np.full(npx, -1, np.int64)
    bestU = np.full(npx, 1 << 62, np.int64)
    ids = np.full(npx, -1, np.int32)
    depth = np.full(npx, np.inf, np.float32)
    rgb = np.tile(np.array(consts[3], np.uint8), (npx, 1))
    normals = np.zeros((npx, 3), np.uint16)
    und_px = np.zeros(npx, bool)
    clip_win = np.zeros(npx, bool)                         # the winner is a near-clipped triangle
    masks = np.zeros((N_LABELS, npx), bool)
    und_lab = np.zeros((N_LABELS, npx), bool)
    beyond = np.zeros((N_LABELS, npx), bool)               # covered but out of range (not in any output)
    aims = dict(frags=0, alpha_tested=0, alpha_eq_thr=0, alpha_thr1=0, alpha_killed=0, ties=0,
                z_far_exact=0, z_far_gap=None, z_near_exact=0, out_far=0, affine_differs=0, textured=0,
                inexact_chain=0, min_rel_gap=None, q_clamped=0, w_ratio=1.0, min_ulp_gap=None, near_front=0, near_behind=0,
                thr_eq={}, thr_plus1={})
    for fl in ("centre", "edge_x", "edge_y", "seam_x", "seam_y", "neg_x", "neg_y", "far_x", "far_y"):
        aims[fl] = 0
    drawn = []
    for i, (label, m, tris) in enumerate(insts):
        mat = scene.materials[m]
        base = _base255(mat)
        ti = mat.texture if table is None or table[m] == KEEP_TEXTURE else int(table[m])
        tex = scene.textures[ti].rgba if ti >= 0 else None
        for k, t in enumerate(tris):
            uid = ((first_instance + i) << 20) | k
            cov = cover_of(t, Wd, Hd).ravel()
            N, NU, NV, pq = _grid_ints(t, Wd, Hd)
            Z = np.where(cov, N.ravel(), 0) << (PQ - pq)
            inr = cov & (Z >= Z_FAR) & (Z <= Z_NEAR)
            beyond[label] |= cov & ~inr
            if 0 < max(t["w"]) < NEAR and min(t["w"]) > 0:         # wholly in front of the near plane: what it would cover
                beyond[label] |= edge_cover(t["xy"], Wd, Hd).ravel()
            aims["out_far"] += int((cov & (Z < Z_FAR)).sum())
            if (cov & (Z < Z_FAR)).any():
                gap = int((Z_FAR - Z[cov & (Z < Z_FAR)]).min())
                aims["z_far_gap"] = gap if aims["z_far_gap"] is None else min(gap, aims["z_far_gap"])
            px = np.nonzero(inr)[0]
            if px.size == 0:
                continue
            aims["frags"] += px.size
            aims["w_ratio"] = max(aims["w_ratio"], max(abs(v) for v in t["w"]) / min(abs(v) for v in t["w"] if v))
            Zp = Z[px]
            aims["z_far_exact"] += int((Zp == Z_FAR).sum())
            aims["z_near_exact"] += int((Zp == Z_NEAR).sum())
            d = rn32_recip(Zp)
            passed = np.ones(px.size, bool)
            und = np.zeros(px.size, bool)
            alb = np.tile(base, (px.size, 1))
            if tex is not None and t["uv"] is not None:
                d64 = d.astype(np.float64)
                u32 = (np.ldexp(NU.ravel()[px].astype(np.float64), -(20 + pq)) * d64).astype(np.float32)
                v32 = (np.ldexp(NV.ravel()[px].astype(np.float64), -(20 + pq)) * d64).astype(np.float32)
                c, und, exact, flags = sample(tex, u32, v32)
                aims["textured"] += px.size
                aims["inexact_chain"] += int((~exact).sum())
                for fl in ("centre", "edge_x", "edge_y", "seam_x", "seam_y", "neg_x", "neg_y", "far_x", "far_y"):
                    aims[fl] += int(flags[fl].sum())
                # the affine (not perspective-correct) variant, for the persp family's aim
                e = [((t["xy"][a][0] - (px % Wd * 256 + 128)) * (t["xy"][b][1] - (px // Wd * 256 + 128))
                      - (t["xy"][b][0] - (px % Wd * 256 + 128)) * (t["xy"][a][1] - (px // Wd * 256 + 128))) for a, b in EDGES]
                ua = sum(e[j] * t["uv"][j][0] for j in range(3)) / float(area2(t["xy"]) * UVQ)
                va = sum(e[j] * t["uv"][j][1] for j in range(3)) / float(area2(t["xy"]) * UVQ)
                th_, tw_ = tex.shape[:2]
                aff = np.floor(ua * tw_ - 0.5).astype(np.int64) * 4096 + np.floor((1 - va) * th_ - 0.5).astype(np.int64)
                aims["affine_differs"] += int((aff != flags["texel"]).sum())
                alb = (c[:, :3] * base[None, :] + 127) // 255
                if mat.alpha_test:
                    thr = int(mat.alpha_threshold)
                    passed = c[:, 3] > thr
                    aims["alpha_tested"] += px.size
                    aims["alpha_eq_thr"] += int((c[:, 3] == thr).sum())
                    aims["alpha_thr1"] += int((c[:, 3] == thr + 1).sum())
                    aims["alpha_killed"] += int((~passed).sum())
                    aims["thr_eq"][m] = aims["thr_eq"].get(m, 0) + int((c[:, 3] == thr).sum())
                    aims["thr_plus1"][m] = aims["thr_plus1"].get(m, 0) + int((c[:, 3] == thr + 1).sum())
            sh = shade(t, cx, cy, consts)
            assert sh is not None, "a generated triangle fails its shading margins under this frame's light"
            q = np.array(sh["q"], np.int64)
            aims["q_clamped"] += int(((alb * q[None, :] + 128) >> 8 > 255).any(1)[passed].sum())
            col = np.minimum(255, (alb * q[None, :] + 128) >> 8).astype(np.uint8)
            und_px[px] |= und
            und_lab[label][px] |= und
            masks[label][px] |= passed
            p2 = px[passed]
            Zq = Zp[passed]
            other = bestZ[p2] >= 0
            if other.any():
                gap = np.abs(Zq[other] - bestZ[p2][other]).astype(np.float64) / Zq[other]
                if (gap > 0).any():
                    g = float(gap[gap > 0].min())
                    aims["min_rel_gap"] = g if aims["min_rel_gap"] is None else min(g, aims["min_rel_gap"])
                _, e = np.frexp(np.maximum(Zq[other], bestZ[p2][other]).astype(np.float64))
                ulps = np.abs(Zq[other] - bestZ[p2][other]) / np.ldexp(1.0, e - 24)       # float32 ulps of the larger 1 / W
                if (ulps > 0).any():
                    g = float(ulps[ulps > 0].min())
                    aims["min_ulp_gap"] = g if aims["min_ulp_gap"] is None else min(g, aims["min_ulp_gap"])
                close = (ulps > 0) & (ulps <= 64 * NEAR_ULPS)
                aims["near_front"] += int((close & (Zq[other] > bestZ[p2][other])).sum())
                aims["near_behind"] += int((close & (Zq[other] < bestZ[p2][other])).sum())
            tie = Zq == bestZ[p2]
            aims["ties"] += int(tie.sum())
            better = (Zq > bestZ[p2]) | (tie & (uid < bestU[p2]))
            w = p2[better]
            bestZ[w], bestU[w] = Zq[better], uid
            ids[w], depth[w], rgb[w] = label, d[passed][better], col[passed][better]
            normals[w] = np.array(sh["normal"], np.uint16)
            clip_win[w] = is_clipped(t)
            drawn.append(dict(inst=i, tri=k, shade=sh, n_won=int(better.sum())))
    d64 = depth.astype(np.float64)
    on = ids >= 0
    ax = (np.arange(npx) % Wd + 0.5 - cx)
    ay = (np.arange(npx) // Wd + 0.5 - cy)
    points = np.full((npx, 3), np.nan, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        points[on, 0] = (ax * d64).astype(np.float32)[on] / np.float32(256.0)
        points[on, 1] = -((ay * d64).astype(np.float32)[on] / np.float32(256.0))
        points[on, 2] = -depth[on]
    shp = (Hd, Wd)
    ids2 = ids.reshape(shp)
    out = dict(ids=ids2, depth=depth.reshape(shp), rgb=rgb.reshape(Hd, Wd, 3), normals=normals.reshape(Hd, Wd, 3),
               points=points.reshape(Hd, Wd, 3), undecided=und_px.reshape(shp), bestZ=bestZ.reshape(shp),
               uid=bestU.reshape(shp), masks=masks.reshape(N_LABELS, Hd, Wd), und_label=und_lab.reshape(N_LABELS, Hd, Wd),
               beyond=beyond.reshape(N_LABELS, Hd, Wd), clip_win=clip_win.reshape(shp),
               inst_stats=np.array([stats_of(ids2 == l) for l in range(N_LABELS)], np.uint32),
               amodal_stats=np.array([stats_of(mk.reshape(shp)) for mk in masks], np.uint32),
               covered=masks.sum(1).astype(np.uint32), aims=aims, drawn=drawn)
    return out


def keypoints(kps, depth, Wd, Hd, cx, cy, PV=None):
    """Item 10 on float32 points [(x, y, z)] -> uv (n, 2) float32, vis (n,) int32: every operation of
    ``((P0 x + P1 y) + P2 z) + P3`` and the division rounded with ``rn32`` on rationals.  ``PV`` is the
    float32 product P V (tests/pose_exact.py); without it V = identity and P = ``projection(cx, cy)``."""
    P = projection(cx, cy) if PV is None else np.asarray(PV, np.float32).astype(np.float64)
    uv = np.zeros((len(kps), 2), np.float32)
    vis = np.zeros(len(kps), np.int32)
    for k, pt in enumerate(kps):
        x, y, z = (Fr(float(np.float32(v))) for v in pt)
        row = lambda r: rn32(rn32(rn32(rn32(Fr(r[0]) * x) + rn32(Fr(r[1]) * y)) + rn32(Fr(r[2]) * z)) + Fr(r[3]))   # noqa: E731
        X, Y, Wc = row(P[0]), row(P[1]), row(P[3])
        if not Wc >= Fr(NEAR):
            uv[k] = -1.0
            continue
        u, v = rn32(X / Wc), rn32(Y / Wc)
        uv[k] = float(u), float(v)
        if not (0 <= u < Wd and 0 <= v < Hd):
            continue
        dd = depth[int(v), int(u)]
        vis[k] = 2 if (np.isinf(dd) or Wc <= Fr(float(dd))) else 1
    return uv, vis


# -- scenes --------------------------------------------------------------------------------------------
def lights():
    """The light sets: (0, 0, 1) with the reference's constants, (0, 0, -1) dimmer and coloured,
    (3, 0, 4) / 5, and one whose q passes 256 (the min(255, ...) clamp)."""
    from constructionsceneposeestimation_amd.scene.model import Light
    return [Light(np.array([0.0, 0.0, 1.0]), 1500.0, np.ones(3), 500.0, np.array([0.75, 0.85, 1.0])),
            Light(np.array([0.0, 0.0, -1.0]), 900.0, np.array([1.0, 0.9, 0.7]), 300.0, np.array([0.5, 0.6, 0.4])),
            Light(np.array([3.0, 0.0, 4.0]), 1200.0, np.array([0.9, 1.0, 0.8]), 700.0, np.array([0.3, 0.35, 0.9])),
            Light(np.array([0.0, 0.0, 1.0]), 1500.0, np.array([1.0, 0.95, 0.9]), 1400.0, np.array([1.0, 0.8, 0.6]))]


class _Builder:
    def __init__(self, Wd, Hd):
        from constructionsceneposeestimation_amd.scene.model import Scene, SceneObject
        self.W, self.H, self.cx, self.cy = Wd, Hd, Wd // 2, Hd // 2
        self.scene = Scene()
        self.scene.objects = [SceneObject(f"/label{l}", "fence", 2, l) for l in range(N_LABELS)]
        self.lights = lights()
        self.scene.light = self.lights[0]
        self.consts = [light_fractions(l) for l in self.lights]
        self.frames = []
        self.rejected = 0
        self.undecided_clips = 0

    def texture(self, rgba):
        from constructionsceneposeestimation_amd.scene.model import Texture
        self.scene.textures.append(Texture(f"t{len(self.scene.textures)}", np.ascontiguousarray(rgba, np.uint8)))
        return len(self.scene.textures) - 1

    def material(self, base255=(255, 255, 255), texture=-1, alpha_test=False, thr=0):
        from constructionsceneposeestimation_amd.scene.model import Material
        self.scene.materials.append(Material(f"m{len(self.scene.materials)}", np.array(base255, np.float64) / 255.0,
                                             texture, alpha_test, thr))
        return len(self.scene.materials) - 1

    def ok(self, t, light):
        """The input conditions: exact planes and the shading margins, in both vertex orders."""
        good = all(planes_exact(s, self.W, self.H, self.cx, self.cy) and shade(s, self.cx, self.cy, self.consts[light])
                   is not None for s in (t, swapped(t)))
        self.rejected += not good
        return good

    def frame(self, family, light, insts):
        self.frames.append(dict(family=family, light=light, insts=insts))


def right_tri(rng, Wd, Hd, p, q, horiz, snap=16, inside=False):
    """Screen vertices: an axis-aligned edge of 2^p units (horizontal or vertical) from a random vertex on
    a multiple of ``snap`` units within the frame +- 4 px (``inside``: within it), the third vertex 2^q units across it."""
    n_al, n_ac = (Wd, Hd) if horiz else (Hd, Wd)
    L, Q, pad = 1 << p, 1 << q, 0 if inside else 4 * 256
    lo_al, hi_al = -pad, n_al * 256 + pad - L
    if hi_al < lo_al or n_ac * 256 + 2 * pad < Q:
        return None
    a0 = int(rng.integers(lo_al // snap, hi_al // snap + 1)) * snap
    sgn = int(rng.choice([-1, 1]))
    lo_b, hi_b = (-pad, n_ac * 256 + pad - Q) if sgn > 0 else (-pad + Q, n_ac * 256 + pad)
    b0 = int(rng.integers(-(-lo_b // snap), hi_b // snap + 1)) * snap
    c = int(rng.integers((a0 - L // 2) // snap, (a0 + L + L // 2) // snap + 1)) * snap
    c = min(max(c, -pad), n_al * 256 + pad)
    pts = [(a0, b0), (a0 + L, b0), (c, b0 + sgn * Q)]
    return pts if horiz else [(y, x) for x, y in pts]


def affine_uv(xy, ou, ov, ru, rv):
    """uvs (in 1/256) affine in screen position: u = ou + ru U, v = ov - rv V (U, V in units; Fractions)."""
    out = []
    for x, y in xy:
        u, v = ou + Fr(ru) * x, ov - Fr(rv) * y
        assert u.denominator == 1 and v.denominator == 1, "the uv of a vertex is no multiple of 1/256"
        out.append((int(u), int(v)))
    return out


def _pick(rng, b, light, make, tries=200):
    for _ in range(tries):
        t = make()
        if t is not None and b.ok(t, light):
            return t
    raise AssertionError("the generator found no exact triangle")


def _sizes(rng, Wd, Hd, lo=9, hi=14):
    p = int(rng.integers(lo, hi + 1))
    q = int(rng.integers(lo, hi + 1))
    return p, q


def _rgba(rng, h, w):
    return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)


def _texel(b, rng):
    """Flat layers, uvs affine in screen position, opaque and alpha-tested (threshold 127) materials on
    random RGBA textures of 16 x 8, 4 x 4, 13 x 7 and 1 x 1.  Aims: pixel centres exactly on texel centres
    (one texel per pixel, aligned) and exactly on texel boundaries (the same, half a texel off); the wrap
    row and column; negative texel coordinates; uvs three repeats away; 8 px per texel and 4 texels per px."""
    Wd, Hd = b.W, b.H
    texs = [b.texture(_rgba(rng, h, w)) for h, w in ((8, 16), (4, 4), (7, 13), (1, 1))]
    dims = [(16, 8), (4, 4), (13, 7), (1, 1)]
    pow2, rest = [], []
    for k, (tx, (tw, th)) in enumerate(zip(texs, dims)):
        for alpha in (False, True):
            m = b.material((255, 255, 255) if k % 2 == 0 else (200, 255, 31), tx, alpha, 127)
            tris = []
            for j in range(6):
                snap = (16, 32, 128, 16, 64, 64)[j]
                # per unit: one texel per pixel; 8 px per texel; 4 texels per px; arbitrary dyadic rates
                ru, rv = [(Fr(1, tw), Fr(1, th)), (Fr(1, tw), Fr(1, th)), (Fr(1, 8 * 16), Fr(1, 8 * 8)),
                          (Fr(4, 16), Fr(4, 8)), (Fr(1, 32), Fr(1, 16)), (Fr(1, 4), Fr(1, 64))][j] if tw in (16, 4, 1) else \
                         [(Fr(1, 16), Fr(1, 8)), (Fr(1, 32), Fr(1, 16)), (Fr(1, 128), Fr(1, 64)), (Fr(1, 16), Fr(1, 8)),
                          (Fr(1, 64), Fr(1, 16)), (Fr(1, 16), Fr(1, 32))][j]
                ou = (0, 128 // tw if tw > 1 else 0, 0, 0, -3 * 256 - 64, 3 * 256)[j]
                ov = (256, 256 - (128 // th if th > 1 else 0), 256, 256, 4 * 256, -3 * 256 + 32)[j]
                if tw == 1:
                    ru, rv = Fr(1, 16), Fr(1, 16)

                def make():
                    p, q = _sizes(rng, Wd, Hd, 11, 13)
                    xy = right_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)), snap)
                    return None if xy is None else tri(xy, 2.0 ** int(rng.integers(0, 5)), affine_uv(xy, ou, ov, ru, rv))
                tris.append(_pick(rng, b, 0, make))
            (pow2 if tw in (16, 4, 1) else rest).append((len(pow2 + rest) % N_LABELS, m, tris))
    b.frame("texel", 0, pow2)
    b.frame("texel_npot", 0, rest)


def _thresh_tex(rng, thr):
    """16 x 8: 4 x 4 blocks of constant alpha thr - 1, thr, thr + 1, 0 and 255 (clipped to 0..255), one
    column of blocks a ramp thr - 2 .. thr + 2, random colours."""
    vals = sorted({max(thr - 1, 0), thr, min(thr + 1, 255), 0, 255})
    a = np.kron(rng.permutation(np.resize(np.array(vals), 8)).reshape(2, 4), np.ones((4, 4), np.int64))
    a[:, 12:16] = np.clip(thr - 2 + np.arange(4), 0, 255)[None, :]
    t = _rgba(rng, 8, 16)
    t[..., 3] = a
    return t


def _thresh(b, rng):
    """Flat layers on textures whose alpha is piecewise constant at thr - 1, thr, thr + 1, 0, 255 for thr =
    0, 127, 254, with ramps, at 2 and 4 px per texel: inside a block the filtered alpha is the block's value,
    so there are fragments at exactly thr (dropped) and thr + 1 (kept).  Each texture is also used by a second
    material with another threshold."""
    Wd, Hd = b.W, b.H
    insts = []
    for k, thr in enumerate((0, 127, 254)):
        tx = b.texture(_thresh_tex(rng, thr))
        for m in (b.material((255, 255, 255), tx, True, thr), b.material((255, 128, 64), tx, True, (126, 254, 0)[k])):
            tris = []
            for j in range(6):                       # (each starts at another block of the texture)
                ru, rv = ((Fr(1, 2 * 16), Fr(1, 2 * 8)), (Fr(1, 4 * 16), Fr(1, 4 * 8)))[j % 2]

                def make():
                    p, q = _sizes(rng, Wd, Hd, 12, 14)
                    xy = right_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)), 64)
                    return None if xy is None else tri(xy, 2.0 ** int(rng.integers(0, 4)),
                                                       affine_uv(xy, 64 * j + 16, 256 + 128 * (j % 2) + 16 * j, ru, rv))
                tris.append(_pick(rng, b, 0, make))
            insts.append((len(insts) % N_LABELS, m, tris))
    b.frame("thresh", 0, insts)


def _tilted(rng, b, light, ws, uv_range=4, lo=11, hi=14, tex=True):
    def make():
        p, q = _sizes(rng, b.W, b.H, lo, hi)
        xy = right_tri(rng, b.W, b.H, p, q, bool(rng.integers(2)))
        if xy is None:
            return None
        w = [float(v) for v in rng.permutation(np.array(ws))]
        uv = [(int(rng.integers(-uv_range * 16, uv_range * 16 + 1)) * 16, int(rng.integers(-uv_range * 16, uv_range * 16 + 1)) * 16)
              for _ in range(3)] if tex else None
        return tri(xy, w, uv)
    return _pick(rng, b, light, make, 2000)


def _persp(b, rng):
    """Tilted triangles with W ratios of 2 to 32 inside one triangle and random uvs on multiples of 1/16 in
    [-2, 2], opaque and alpha-tested on a random 16 x 8 texture: affine interpolation would pick another
    texel on at least a quarter of the fragments."""
    tx = b.texture(_rgba(rng, 8, 16))
    insts = []
    for k, ws in enumerate(((1, 32, 4), (2, 64, 64), (1, 1, 8), (4, 16, 128), (2, 4, 8), (1, 32, 32))):
        m = b.material((255, 255, 255), tx, bool(k % 2), 100)
        insts.append((k % N_LABELS, m, [_tilted(rng, b, 0, ws, 2, 12, 14) for _ in range(3)]))
    b.frame("persp", 0, insts)


def _cross(b, rng):
    """Pairs and triples of tilted triangles over the same screen triangle with their W exchanged, of
    different labels, alpha-tested and opaque: they intersect along a line inside the triangle and the id
    flips there.  The third of a triple is a flat layer through the same line.  A second frame, cross_near,
    holds nearly parallel pairs: a tilted triangle and the same with its axis-aligned edge moved by 1/16 or
    1/8 px along itself and its third vertex by another such step, found by a seeded search for pairs that
    cross inside the frame (at least 50 common centres on either side) with a smallest nonzero difference
    of at most NEAR_ULPS float32 ulps of 1 / W; one pair is alpha-tested, one has a flat layer through it."""
    tx = b.texture(_rgba(rng, 8, 16))
    insts = []
    for k, (wa, wb, wflat) in enumerate((((2, 2, 8), (8, 8, 2), 4), ((1, 4, 4), (4, 1, 1), None), ((4, 4, 16), (16, 16, 4), 8),
                                         ((2, 8, 2), (8, 2, 8), None), ((16, 64, 64), (64, 16, 16), 32))):
        for _ in range(4000):
            p, q = _sizes(rng, b.W, b.H, 12, 14)
            xy = right_tri(rng, b.W, b.H, p, q, bool(rng.integers(2)))
            if xy is None:
                continue
            uv = [(int(rng.integers(-32, 33)) * 16, int(rng.integers(-32, 33)) * 16) for _ in range(3)]
            t, o = tri(xy, wa, uv), tri(xy, wb, uv)
            fl = None if wflat is None else tri(xy, float(wflat), uv)
            if all(b.ok(s, 0) for s in (t, o) + (() if fl is None else (fl,))):
                break
        else:
            raise AssertionError("no exact crossing pair")
        insts.append(((3 * k) % N_LABELS, b.material((255, 200, 150), tx, True, 90), [t]))
        insts.append(((3 * k + 1) % N_LABELS, b.material((100, 255, 255), tx, False, 0), [o]))
        if fl is not None:
            insts.append(((3 * k + 2) % N_LABELS, b.material((40, 80, 255)), [fl]))
    b.frame("cross", 0, insts)
    # nearly parallel pairs, in a frame of their own (nothing in front of a pair's common pixels but the pair)
    insts = []
    for k in range(3):
        for _ in range(40000):
            p, q = _sizes(rng, b.W, b.H, 13, 14)
            xy = right_tri(rng, b.W, b.H, p, q, bool(rng.integers(2)))
            if xy is None:
                continue
            ws = [float(v) for v in rng.choice([1, 2, 4, 8, 16, 32], 3)]
            ax = 0 if xy[0][1] == xy[1][1] else 1
            s0, s2 = int(rng.choice([-32, -16, 16, 32])), int(rng.choice([-32, -16, 0, 16, 32]))
            if len(set(ws)) == 1 or s0 == s2:
                continue
            move = lambda pt, d: tuple(c + d * (j == ax) for j, c in enumerate(pt))       # noqa: E731
            uv = [(int(rng.integers(-32, 33)) * 16, int(rng.integers(-32, 33)) * 16) for _ in range(3)]
            t, o = tri(xy, ws, uv), tri([move(xy[0], s0), move(xy[1], s0), move(xy[2], s2)], ws, uv)
            g = pair_gap(t, o, b.W, b.H)
            if g is not None and g[0] <= NEAR_ULPS and min(g[1], g[2]) >= 50 and b.ok(t, 0) and b.ok(o, 0):
                break
        else:
            raise AssertionError("no exact nearly parallel pair")
        if g[3]:                                     # the nearer one at the smallest difference gets the larger uid,
            t, o = o, t                              # so that a key that lost its low bits would tie to the wrong one
        insts.append(((2 * k) % N_LABELS, b.material((255, 200, 150), tx, k == 1, 60), [t]))
        insts.append(((2 * k + 1) % N_LABELS, b.material((100, 255, 255), tx, False, 0), [o]))
        if k == 2:                                   # a flat layer through the pair, at the W of its middle
            fl = tri(xy, sorted(ws)[1])
            if b.ok(fl, 0):
                insts.append((4, b.material((40, 80, 255)), [fl]))
    b.frame("cross_near", 0, insts)


def plane_z(t, Wd, Hd):
    """(Z, in range, covered) (H, W) of one triangle: 1 / W = Z / 2^ZS on the covered centres."""
    N, _, _, pq = _grid_ints(t, Wd, Hd)
    cov = cover_of(t, Wd, Hd)
    Z = np.where(cov, N, 0) << (PQ - pq)
    return Z, cov & (Z >= Z_FAR) & (Z <= Z_NEAR), cov


def pair_gap(a, b, Wd, Hd):
    """Two triangles on their common in-range centres -> (smallest nonzero |1/W_a - 1/W_b| in float32 ulps of
    the larger, centres where a is nearer, centres where b is nearer, whether a is nearer at that smallest
    difference), or None without a common centre."""
    (Za, ia, _), (Zb, ib, _) = plane_z(a, Wd, Hd), plane_z(b, Wd, Hd)
    both = ia & ib & (Za != Zb)
    if not both.any():
        return None
    _, e = np.frexp(np.maximum(Za[both], Zb[both]).astype(np.float64))
    ulps = np.abs(Za[both] - Zb[both]) / np.ldexp(1.0, e - 24)
    k = int(np.argmin(ulps))
    return (float(ulps.min()), int((Za[both] > Zb[both]).sum()), int((Za[both] < Zb[both]).sum()),
            bool(Za[both][k] > Zb[both][k]))


def _tie(b, rng):
    """Exact depth ties, the two fragments differing in material or uv so that rgb shows the winner:
    (a) the same flat triangles in two instances of different labels, and overlapping ones in one layer;
    (b) a triangle twice in one mesh with other uvs; (c) two tilted triangles in one plane (W constant
    along their common axis-aligned edge, the third vertices apart along it); (d) a duplicate whose first
    instance is alpha-tested with holes, so that the second must show through them."""
    Wd, Hd = b.W, b.H
    tx = b.texture(_rgba(rng, 8, 16))
    holes = _rgba(rng, 8, 16)
    holes[..., 3] = np.kron(np.array([[0, 255, 0, 255], [255, 0, 255, 0]]), np.ones((4, 4), np.int64))
    th = b.texture(holes)

    def flat(w, snap=32, lo=12):
        def make():
            p, q = _sizes(rng, Wd, Hd, lo, 14)
            xy = right_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)), snap, inside=True)
            return None if xy is None else tri(xy, w, affine_uv(xy, 16, 300, Fr(1, 32), Fr(1, 16)))
        return _pick(rng, b, 0, make)

    insts = []
    a = [flat(2.0), flat(2.0), flat(2.0)]                                                   # (a)
    insts.append((0, b.material((255, 40, 40), tx), a))
    insts.append((1, b.material((40, 255, 40)), [dict(t) for t in a]))
    t = flat(4.0)                                                                           # (b)
    insts.append((2, b.material((255, 255, 255), tx), [t, dict(t, uv=[(u + 77, v - 130) for u, v in t["uv"]])]))
    for _ in range(4000):                                                                   # (c)
        p, q = _sizes(rng, Wd, Hd, 12, 14)
        xy = right_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)), inside=True)
        if xy is None:
            continue
        ax = 0 if xy[0][1] == xy[1][1] else 1
        sh = int(rng.choice([-1, 1])) * int(rng.integers(48, 200)) * 16
        c2 = list(xy[2])
        c2[ax] += sh
        t1 = tri(xy, (2.0, 2.0, 8.0), [(0, 0), (256, 16), (48, 512)])
        t2 = tri([xy[0], xy[1], tuple(c2)], (2.0, 2.0, 8.0), [(512, 0), (16, 256), (0, 48)])
        if b.ok(t1, 0) and b.ok(t2, 0):
            break
    else:
        raise AssertionError("no exact coplanar pair")
    insts.append((3, b.material((255, 255, 255), tx), [t1]))
    insts.append((4, b.material((255, 255, 0), tx), [t2]))
    d = flat(1.0, 64)                                                                       # (d)
    insts.append((5, b.material((255, 255, 255), th, True, 128), [d]))
    insts.append((3, b.material((0, 90, 255)), [dict(d)]))
    b.frame("tie", 0, insts)


def _range(b, rng):
    """Tilted triangles across W = far = 256 (W of 64 .. 1024 at their vertices), some with a vertex of W =
    256 on a pixel centre, where 1 / W = 2^-8 exactly (kept), and with that vertex 1/16 px further along
    the falling 1 / W, so that the centre is just beyond (dropped); a triangle from a seeded search with a
    dropped centre at most FAR_ULPS float32 ulps below 2^-8; a vertex of W = 1/2 = near on a pixel
    centre (1 / W = 2, kept); a flat layer at W = 256 (kept) and one at 512 (nothing)."""
    Wd, Hd = b.W, b.H
    insts = []
    tris = []
    for off in (0, 16, 0, -16, 0, 16):
        def make():
            horiz = bool(rng.integers(2))
            p, q = _sizes(rng, Wd, Hd, 12, 14)
            xy = right_tri(rng, Wd, Hd, p, q, horiz, 256, inside=True)
            if xy is None:
                return None
            dx, dy = 128 - xy[0][0] % 256 + off, 128 - xy[0][1] % 256
            xy = [(x + dx, y + dy) for x, y in xy]                       # vertex 0 on a pixel centre (+ off in x)
            return tri(xy, (256.0, float(rng.choice([64.0, 128.0])), float(rng.choice([512.0, 1024.0]))))
        tris.append(_pick(rng, b, 0, make, 2000))
    insts.append((0, b.material((255, 255, 255)), tris))
    insts.append((1, b.material((255, 128, 0)), [_tilted(rng, b, 0, ws, tex=False) for ws in ((128, 512, 512), (64, 1024, 256), (128, 128, 512))]))
    near = []
    for _ in range(3):
        def make():
            p, q = _sizes(rng, Wd, Hd, 11, 13)
            xy = right_tri(rng, Wd, Hd, p, q, True, 256, inside=True)
            if xy is None or xy[2][1] < xy[0][1]:
                return None
            xy = [(x + 128, y + 128) for x, y in xy]
            xy[2] = (xy[0][0] + int(rng.integers(0, 8)) * 256, xy[2][1])   # vertex 0 is the top-left corner: its centre is covered
            return tri(xy, (0.5, float(rng.choice([1.0, 2.0])), float(rng.choice([1.0, 4.0]))))
        near.append(_pick(rng, b, 0, make, 2000))
    insts.append((2, b.material((0, 255, 128)), near))

    def layer(w):
        def make():
            xy = right_tri(rng, Wd, Hd, 13, 13, True, 16, inside=True)
            return None if xy is None else tri(xy, w)
        return _pick(rng, b, 0, make)
    insts.append((3, b.material((90, 90, 90)), [layer(256.0)]))
    insts.append((4, b.material((255, 0, 255)), [layer(512.0), layer(0.25)]))
    insts.append((5, b.material((9, 9, 200)), [layer(128.0)]))
    for _ in range(200000):                          # a dropped centre at most FAR_ULPS below 2^-8
        p, q = _sizes(rng, Wd, Hd, 12, 14)
        xy = right_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)))
        ws = [float(v) for v in rng.choice([64, 128, 256, 512, 1024], 3)]
        if xy is None or max(ws) <= 256 or min(ws) >= 256:
            continue
        t = tri(xy, ws)
        Z, _, cov = plane_z(t, Wd, Hd)
        out = cov & (Z < Z_FAR)
        if out.any() and int((Z_FAR - Z[out]).min()) <= FAR_ULPS << (ZS - 32) and b.ok(t, 0):
            break
    else:
        raise AssertionError("no exact triangle with a centre just beyond far")
    insts.append((1, b.material((200, 30, 90)), [t]))
    b.frame("range", 0, insts)


def _light(b, rng):
    """Every light set on flat and tilted triangles, untextured with base colours 0, k/255 and 1 and
    textured: one frame per light set."""
    tx = b.texture(_rgba(rng, 8, 16))
    for li in range(len(b.lights)):
        insts = []
        for k, base in enumerate(((0, 0, 0), (1, 2, 254), (255, 255, 255), (37, 128, 201))):
            m = b.material(base, tx if k == 3 else -1)
            tris = []
            for j, ws in enumerate(((1,), (4,), (2, 4, 4), (1, 2, 8), (8, 8, 2))):
                if len(ws) == 1:
                    def make():
                        p, q = _sizes(rng, b.W, b.H, 11, 13)
                        xy = right_tri(rng, b.W, b.H, p, q, bool(rng.integers(2)))
                        return None if xy is None else tri(xy, float(ws[0]), affine_uv(xy, 0, 256, Fr(1, 16), Fr(1, 8)))
                    tris.append(_pick(rng, b, li, make))
                else:
                    tris.append(_tilted(rng, b, li, ws, 2, 11, 13))
            insts.append(((k + li) % N_LABELS, m, tris))
        b.frame(f"light{li}", li, insts)


def _trim(b, rng):
    """Alpha-tested cards (two triangles) whose 16 x 16 texture has one opaque 2 x 2 block and whose uvs span
    10/16 of a repeat around it, like the engaging cases of tests/test_gpu_alpha_trim.py: flat cards and
    tilted ones (W constant along one axis), partly in front of an opaque flat backdrop."""
    Wd, Hd = b.W, b.H
    insts = []
    back = tri([(0, 0), (1 << 14, 0), (0, 1 << 13)], 64.0)
    assert b.ok(back, 0)
    insts.append((0, b.material((120, 110, 100)), [back, tri([(1 << 14, 0), (1 << 14, 1 << 13), (0, 1 << 13)], 64.0)]))
    assert b.ok(insts[0][2][1], 0)
    for k, (bx, by) in enumerate(((3, 4), (9, 9), (12, 2), (6, 11))):
        t = _rgba(rng, 16, 16)
        t[..., 3] = 0
        t[by:by + 2, bx:bx + 2, 3] = 255
        m = b.material((255, 255, 255), b.texture(t), True, 100)
        for _ in range(2000):
            p = 13
            x0 = int(rng.integers(0, max(1, (Wd * 256 - (1 << p)) // 256 + 1))) * 256
            y0 = int(rng.integers(0, max(1, (Hd * 256 - (1 << p)) // 256 + 1))) * 256
            L = 1 << p
            A, B, C, D = (x0, y0), (x0 + L, y0), (x0, y0 + L), (x0 + L, y0 + L)
            wl, wr = (2.0, 2.0) if k % 2 == 0 else ((2.0, 8.0) if k == 1 else (4.0, 1.0))
            u0, v0 = (bx - 4) * 16, 256 - (by - 4) * 16                # the card shows texels bx - 4 .. bx + 6
            uv = {A: (u0, v0), B: (u0 + 160, v0), C: (u0, v0 - 160), D: (u0 + 160, v0 - 160)}
            w = {A: wl, C: wl, B: wr, D: wr}
            t1 = tri([A, B, C], [w[A], w[B], w[C]], [uv[A], uv[B], uv[C]])
            t2 = tri([B, D, C], [w[B], w[D], w[C]], [uv[B], uv[D], uv[C]])
            if b.ok(t1, 0) and b.ok(t2, 0):
                break
        else:
            raise AssertionError("no exact card")
        insts.append((1 + k, m, [t1, t2]))
    b.frame("trim", 0, insts)


def _virt_tri(rng, Wd, Hd, p, q, horiz, pad_px, snap=16):
    """As ``right_tri`` with the vertices up to ``pad_px`` outside the frame: the virtual screen position of
    a vertex in front of the near plane may lie anywhere."""
    n_al, n_ac = (Wd, Hd) if horiz else (Hd, Wd)
    L, Q, pad = 1 << p, 1 << q, pad_px * 256
    if n_al * 256 + 2 * pad < L:
        return None
    a0 = int(rng.integers(-pad // snap, (n_al * 256 + pad - L) // snap + 1)) * snap
    b0 = int(rng.integers(-pad // snap, (n_ac * 256 + pad) // snap + 1)) * snap
    sgn = int(rng.choice([-1, 1]))
    c = int(rng.integers((a0 - L // 2) // snap, (a0 + L + L // 2) // snap + 1)) * snap
    pts = [(a0, b0), (a0 + L, b0), (c, b0 + sgn * Q)]
    return pts if horiz else [(y, x) for x, y in pts]


def pair_need(Hd):
    """clip_pair: each triangle of a pair is the nearer one on this many of their common centres."""
    return 30 if Hd >= 64 else 12


def texels_of(t, tex, Wd, Hd):
    """The in-range fragments of one textured triangle on ``tex`` -> (texel column floor(t_x), texel row, filtered
    alpha), unwrapped, as ``render`` computes them."""
    N, NU, NV, pq = _grid_ints(t, Wd, Hd)
    Z = np.where(cover_of(t, Wd, Hd), N, 0).ravel() << (PQ - pq)
    px = np.nonzero((Z >= Z_FAR) & (Z <= Z_NEAR))[0]
    d64 = rn32_recip(Z[px]).astype(np.float64)
    u32 = (np.ldexp(NU.ravel()[px].astype(np.float64), -(20 + pq)) * d64).astype(np.float32)
    v32 = (np.ldexp(NV.ravel()[px].astype(np.float64), -(20 + pq)) * d64).astype(np.float32)
    c, _, _, flags = sample(tex, u32, v32)
    tx = (flags["texel"] + 2048) // 4096
    return tx, flags["texel"] - tx * 4096, c[:, 3]


def _orient(t):
    """The sign of det: that of 2 area W0 W1 W2 (positive W keep the screen orientation)."""
    return 1 if area2(t["xy"]) * t["w"][0] * t["w"][1] * t["w"][2] > 0 else -1


def _clip_search(rng, b, make, min_px, max_px, pred=None, tries=20000, must=True, cheap=None):
    """A triangle from ``make`` that satisfies ``cheap``, whose clip vertices are decided in both vertex
    orders, that shows min_px .. max_px in-range centres, satisfies ``pred`` (given the triangle and its
    ``plane_z``) and passes the input conditions (``_Builder.ok``); the tests run cheapest first."""
    for _ in range(tries):
        t = make()
        if t is None or abs(area2(t["xy"])).bit_length() - 1 > PQ or (cheap is not None and not cheap(t)):
            continue
        if clip_exact(t) is None:
            b.undecided_clips += 1
            continue
        if min_px > 0:                               # no more centres than the polygon's box holds inside the frame,
            x0, y0, x1, y1, need = getattr(pred, "within", (0, 0, b.W, b.H, min_px))      # or inside the pixel box ``pred`` needs
            xs, ys = [v[0] for v in clip_exact(t)["poly"]] or [0], [v[1] for v in clip_exact(t)["poly"]] or [0]
            bw = (min(max(xs), x1 * 256) - max(min(xs), x0 * 256)) // 256 + 1
            bh = (min(max(ys), y1 * 256) - max(min(ys), y0 * 256)) // 256 + 1
            if bw <= 0 or bh <= 0 or bw * bh < need:
                continue
        pz = plane_z(t, b.W, b.H)
        if not min_px <= int(pz[1].sum()) <= max_px or (pred is not None and not pred(t, pz)):
            continue
        if clip_exact(swapped(t)) is None:
            b.undecided_clips += 1
            continue
        if b.ok(t, 0):
            return t
    assert not must, "the generator found no exact clipped triangle"
    return None


PALETTE = ((255, 60, 60), (60, 255, 60), (60, 60, 255), (255, 255, 60), (255, 60, 255), (60, 255, 255), (255, 255, 255),
           (128, 64, 200), (200, 128, 64), (64, 200, 128))
W_IN, W_FRONT, W_BEHIND = (1.0, 2.0, 4.0, 16.0), (0.125, 0.25), (-4.0, -1.0, -0.5, -0.25)


def _clip(b, rng):
    """Triangles with one or two vertices in front of the near plane W = 1/2 (W of 1/8, 1/4, or negative:
    behind the camera), in four frames, all in front of nothing or of a far backdrop.
    clip: every inside mask (code 1, 2, 4: one sub-triangle; 3, 5, 6: two) with the outside vertices at small
    positive W and behind the camera, in both orientations, W ratios up to 128; a vertex at exactly W = near
    (inside; tt = 0 or 1 on its edges, a zero-area sub-triangle first or second in the fan) at each index, one
    with both others outside (nothing left), and a flat triangle at W = near (all inside: drawn, 1 / W = 2); a
    triangle of W = -1, -1, -2 alone in label 5 (nothing).
    clip_edge: W varying along x or y only, 1, 1, -1, so that the clip edge is a column or row of pixel
    centres with 1 / W = 2 exactly, as a left / top edge (centres kept) and a right / bottom one (not); a
    visible strip whose virtual vertices lie left of, right of and above the frame (one behind the camera),
    and one whose three virtual vertices all lie above it.
    clip_tex: alpha-tested cards across the near plane (W constant along one axis, 16 x 8 texture, an opaque
    2 x 2 block on the visible side and one on the cut side) and opaque textured clipped triangles.
    clip_pair: pairs of different labels, clipped with clipped and clipped with unclipped, that cross inside
    the clipped region (each is the nearer one on ``pair_need`` common centres or more)."""
    Wd, Hd = b.W, b.H
    big = Hd >= 64
    lim = (60, 420) if big else (24, 150)
    pal = iter(PALETTE * 8)

    def coded(code, outs, ins, orient, uv=False, tag=None, lo=12, hi=15, lim=lim, pred=None):
        def make():
            p, q = _sizes(rng, Wd, Hd, lo, hi)
            xy = _virt_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)), 48)
            if xy is None:
                return None
            w = [float(rng.choice(ins if code >> k & 1 else outs)) for k in range(3)]
            uvs = [(int(rng.integers(-16, 17)) * 16, int(rng.integers(-16, 17)) * 16) for _ in range(3)] if uv else None
            return tri(xy, w, uvs, tag)
        return _clip_search(rng, b, make, lim[0], lim[1], pred, cheap=None if orient is None else lambda t: _orient(t) == orient)

    insts = []
    for code in (1, 2, 4, 3, 5, 6):
        tris = [coded(code, W_FRONT, (16.0,) if code == 1 else W_IN, 1), coded(code, W_BEHIND, W_IN, -1),
                coded(code, W_FRONT + W_BEHIND, W_IN, None)]
        insts.append((len(insts) % 5, b.material(next(pal)), tris))
    near = []
    for idx in range(3):                             # W = near at vertex idx, the others (in, out) and (out, in)
        for flip in (0, 1):
            def make():
                p, q = _sizes(rng, Wd, Hd, 12, 14)
                xy = _virt_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)), 16)
                w = [0.0, 0.0, 0.0]
                w[idx] = NEAR
                w[(idx + 1 + flip) % 3] = float(rng.choice((1.0, 2.0, 4.0)))
                w[(idx + 2 - flip) % 3] = float(rng.choice(W_FRONT + W_BEHIND))
                return None if xy is None else tri(xy, w, None, "near_vertex")
            near.append(_clip_search(rng, b, make, lim[0] // 2, lim[1]))

    def make():
        p, q = _sizes(rng, Wd, Hd, 12, 14)
        xy = _virt_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)), 16)
        return None if xy is None else tri(xy, (NEAR, float(rng.choice(W_FRONT)), float(rng.choice(W_BEHIND))), None, "near_alone")
    near.append(_clip_search(rng, b, make, 0, 0))
    insts.append((0, b.material(next(pal)), near[:4]))
    insts.append((1, b.material(next(pal)), near[4:]))

    def make():
        p, q = _sizes(rng, Wd, Hd, 11, 12)
        xy = right_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)), inside=True)
        return None if xy is None else tri(xy, NEAR, None, "near_flat")
    insts.append((2, b.material(next(pal)), [_pick(rng, b, 0, make)]))

    def make():
        p, q = _sizes(rng, Wd, Hd, 12, 14)
        xy = right_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)), inside=True)
        return None if xy is None else tri(xy, (-1.0, -1.0, -2.0), None, "invisible")
    insts.append((5, b.material(next(pal)), [_clip_search(rng, b, make, 0, 0)]))
    b.frame("clip", 0, insts)

    # clip edges through pixel centres, and the homogeneous reject
    insts = []
    p, q = (12, 13) if big else (11, 12)
    L, Q = 1 << p, 1 << q
    edge = []
    for axis in (0, 1):
        for sg in (1, -1):                           # sg > 0: the clip edge is the region's left / top edge
            for _ in range(2):
                def make():
                    n_ac, n_al = (Wd, Hd) if axis == 0 else (Hd, Wd)
                    lo, hi = (0, n_ac - Q // 512 - 1) if sg > 0 else (Q // 512, n_ac - 1)
                    line = int(rng.integers(lo, hi + 1)) * 256 + 128            # 1 / W = 2 on this column / row of centres
                    a = line + sg * (Q // 2)
                    y0 = int(rng.integers(0, (n_al * 256 - L) // 16 + 1)) * 16
                    yb = y0 + int(rng.integers(0, L // 16 + 1)) * 16
                    pts = [(a, y0), (a, y0 + L), (a + sg * Q, yb)]
                    return tri(pts if axis == 0 else [(y, x) for x, y in pts], (1.0, 1.0, -1.0), None,
                               f"edge_{'xy'[axis]}_{'incl' if sg > 0 else 'excl'}")
                edge.append(_clip_search(rng, b, make, 20, 1 << 20))
    for k in range(0, 8, 2):
        insts.append((k // 2, b.material(next(pal)), edge[k:k + 2]))
    ya = (Hd - 8) * 256                              # a strip along the bottom: A left of, B right of, C above the frame
    qs = 14 if big else 13
    xa = -((1 << 15) - Wd * 256) // 2 // 16 * 16
    strip = tri([(xa, ya), (xa + (1 << 15), ya), (Wd * 128, ya - (1 << qs))], (1.0, 1.0, -1.0), None, "hom_sides")
    assert clip_exact(strip) is not None and b.ok(strip, 0), "the strip under the homogeneous reject is not exact"
    xs = (Wd // 2 - 16) * 256                        # all three above the frame: A, B 8 px, C (behind the camera) 40 px
    above = tri([(xs, -8 * 256), (xs + (1 << 13), -8 * 256), (xs + (1 << 12), -40 * 256)], (1.0, 1.0, -1.0), None, "hom_above")
    assert clip_exact(above) is not None and b.ok(above, 0), "the triangle above the frame is not exact"
    # a vertex in the camera's plane, W = 0: clip (+-2^a, 0, 0) or (0, +-2^a, 0); the two others differ by 2^j units
    # across that axis, so that det = X0 W1 W2 (y1 - y2) is a power of two.  A seeded search of at most 10,000.
    w0 = []
    for n_try in range(10000):
        a, axis, k, j = int(rng.integers(0, 7)), int(rng.integers(2)), int(rng.integers(3)), int(rng.integers(10, 14))
        n_al, n_ac = (Wd, Hd) if axis == 0 else (Hd, Wd)
        x1, y1 = int(rng.integers(0, n_al * 16 + 1)) * 16, int(rng.integers(0, n_ac * 16 + 1)) * 16
        x2, y2 = x1 + int(rng.integers(-64, 65)) * 16, y1 + int(rng.choice([-1, 1])) * (1 << j)
        c0 = (int(rng.choice([-1, 1])) << a, 0)
        pts = [(x1, y1), (x2, y2)]
        if axis:
            pts, c0 = [(y, x) for x, y in pts], (0, c0[0])
        t = tri_w0(k, c0, pts, [float(v) for v in rng.choice((0.5, 1.0, 2.0, 4.0), 2)], "w0")
        if any(clip_exact(s) is None for s in (t, swapped(t))):
            continue
        if planes_exact(t, Wd, Hd, b.cx, b.cy) and int(plane_z(t, Wd, Hd)[1].sum()) >= 20 and b.ok(t, 0):
            w0.append(t)
            if len(w0) == 2:
                break
    b.w0_searched = n_try + 1
    insts.append((4, b.material(next(pal)), [strip, above] + w0))
    b.frame("clip_edge", 0, insts)

    # textured: cards (their texture reads columns up to 7 of the window with W 1 -> 1/4 and up to 3 with 1 -> -1: the clip
    # line lies at 2/3 and at 1/4 of the u range, so the second block, at columns 8, 9 and 5, 6, is never read) and opaque triangles
    insts = []
    back = [tri([(0, 0), (1 << 14, 0), (0, 1 << 13)], 64.0), tri([(1 << 14, 0), (1 << 14, 1 << 13), (0, 1 << 13)], 64.0)]
    assert all(b.ok(t, 0) for t in back)
    insts.append((0, b.material((120, 110, 100)), back))
    Lc = 1 << 13
    for k, (win, wout, vis, cut) in enumerate(((1.0, 0.25, 2, 8), (1.0, -1.0, 0, 5))):
        t = _rgba(rng, 8, 16)
        t[..., 3] = 0
        bx, by = 4, 2
        for off in (vis, cut):                       # window offsets of the two opaque blocks along the card's W axis
            t[by:by + 2, (bx - 4 + off) % 16:(bx - 4 + off) % 16 + 2, 3] = 255
        m = b.material((255, 255, 255), b.texture(t), True, 100)
        for _ in range(4000):
            x0 = int(rng.integers(2, max(3, Wd - 34))) * 256
            y0 = int(rng.integers(0, max(1, Hd - 32 + 1))) * 256
            if k == 1:                               # the visible part lies beyond the inside edge, away from the other
                x0 = int(rng.integers(18, max(19, Wd - 2))) * 256
            A, B, C, D = (x0, y0), (x0 + Lc, y0), (x0, y0 + Lc), (x0 + Lc, y0 + Lc)
            u0, v0 = (bx - 4) * 16, 256 - (by - 2) * 32
            uv = {A: (u0, v0), B: (u0 + 160, v0), C: (u0, v0 - 160), D: (u0 + 160, v0 - 160)}
            w = {A: win, C: win, B: wout, D: wout}
            t1 = tri([A, B, C], [w[A], w[B], w[C]], [uv[A], uv[B], uv[C]], "card")
            t2 = tri([B, D, C], [w[B], w[D], w[C]], [uv[B], uv[D], uv[C]], "card")
            if all(clip_exact(s) is not None for s in (t1, t2, swapped(t1), swapped(t2))) and b.ok(t1, 0) and b.ok(t2, 0):
                break
        else:
            raise AssertionError("no exact clipped card")
        insts.append((1 + k, m, [t1, t2]))
    mo = b.material((255, 255, 255), b.texture(_rgba(rng, 8, 16)))
    insts.append((3, mo, [coded(5, W_FRONT, (1.0, 2.0), None, uv=True), coded(2, W_BEHIND, (1.0, 2.0), None, uv=True)]))
    def crossing(o, others=()):
        """Whether a triangle and ``o`` are each the nearer one on enough common centres that ``others`` leave alone."""
        need = pair_need(Hd)
        Zo, io, _ = plane_z(o, Wd, Hd)
        for x in others:
            io = io & ~plane_z(x, Wd, Hd)[1]

        def pred(t, pz):
            Zt, it, _ = pz
            return min(int((Zo > Zt)[io & it].sum()), int((Zo < Zt)[io & it].sum())) >= need
        ys, xs = np.nonzero(io)                      # the partner's polygon has to reach 2 need centres of this box
        pred.within = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1, 2 * need) if ys.size else (0, 0, 0, 0, 1)
        return pred
    a1 = coded(3, W_FRONT, (4.0, 16.0), None, tag="pair_cc")
    a2 = coded(6, W_BEHIND + W_FRONT, W_IN, None, tag="pair_cc", pred=crossing(a1))

    def make():
        p, q = _sizes(rng, Wd, Hd, 12, 14)
        xy = right_tri(rng, Wd, Hd, p, q, bool(rng.integers(2)))
        return None if xy is None else tri(xy, [float(v) for v in rng.choice((1.0, 2.0, 4.0), 3)], None, "pair_cu")
    for _ in range(20):                              # (not every clipped triangle has room for a partner beside the first pair)
        c1 = coded(5, W_BEHIND, (4.0, 16.0), None, tag="pair_cu")
        c2 = _clip_search(rng, b, make, 12, 1 << 20, crossing(c1, (a1, a2)), 2000, False)
        if c2 is not None:
            break
    assert c2 is not None, "no crossing pair of a clipped and an unclipped triangle"
    b.frame("clip_tex", 0, insts)
    insts = [(0, b.material((120, 110, 100)), [dict(t) for t in back])]
    for lab, t in ((1, a1), (2, a2), (3, c1), (4, c2)):
        insts.append((lab, b.material(next(pal)), [t]))
    b.frame("clip_pair", 0, insts)


def _swap(b, rng):
    """Texture tables (``csg_set_dr_textures``): one set of instances -- an opaque backdrop, two flat and two
    tilted alpha-tested cards on one material (authored: 16 x 8, one opaque 2 x 2 block, as ``_trim``; the cards show
    10 x 3 texels around it) and two
    opaque textured triangles -- drawn by seven frames that differ in their table alone: the authored
    indices spelt out; KEEP_TEXTURE; the same alpha with other RGB; the block in the opposite corner of the
    card's window; a random 4 x 4; a random 13 x 7 (swap_npot); and -1 on the opaque material."""
    Wd, Hd = b.W, b.H

    def block(bx, by):
        t = _rgba(rng, 8, 16)
        t[..., 3] = 0
        t[by:by + 2, bx:bx + 2, 3] = 255
        return t
    auth = block(2, 2)
    rgb2 = _rgba(rng, 8, 16)
    rgb2[..., 3] = auth[..., 3]
    T = [b.texture(t) for t in (auth, rgb2, block(9, 3), _rgba(rng, 4, 4), _rgba(rng, 7, 13))]
    O = [b.texture(_rgba(rng, 8, 16)) for _ in range(2)]
    ma = b.material((255, 255, 255), T[0], True, 100)
    mo = b.material((200, 255, 120), O[0])
    insts = []
    back = [tri([(0, 0), (1 << 14, 0), (0, 1 << 13)], 64.0), tri([(1 << 14, 0), (1 << 14, 1 << 13), (0, 1 << 13)], 64.0)]
    assert all(b.ok(t, 0) for t in back)
    insts.append((0, b.material((120, 110, 100)), back))
    L = 1 << 13
    for k in range(4):
        for _ in range(2000):
            x0 = int(rng.integers(0, max(1, Wd - 32 + 1))) * 256
            y0 = int(rng.integers(0, max(1, Hd - 32 + 1))) * 256
            A, B, C, D = (x0, y0), (x0 + L, y0), (x0, y0 + L), (x0 + L, y0 + L)
            wl, wr = (2.0, 2.0) if k % 2 == 0 else ((2.0, 8.0) if k == 1 else (4.0, 1.0))
            u0, v0 = 16, 256 - 48                    # the card shows texel columns 1 .. 11 and rows 1.5 .. 4.5: with the trim's
            uv = {A: (u0, v0), B: (u0 + 160, v0), C: (u0, v0 - 96), D: (u0 + 160, v0 - 96)}   # guard band less than a repeat
            w = {A: wl, C: wl, B: wr, D: wr}
            t1 = tri([A, B, C], [w[A], w[B], w[C]], [uv[A], uv[B], uv[C]])
            t2 = tri([B, D, C], [w[B], w[D], w[C]], [uv[B], uv[D], uv[C]])
            if b.ok(t1, 0) and b.ok(t2, 0):
                break
        else:
            raise AssertionError("no exact card")
        insts.append((1 + k, ma, [t1, t2]))
    insts.append((5, mo, [_tilted(rng, b, 0, ws, 2, 12, 13) for ws in ((1, 2, 2), (2, 2, 4))]))
    for name, table in (("swap_id", {ma: T[0], mo: O[0]}), ("swap_keep", {}), ("swap_rgb", {ma: T[1], mo: O[1]}),
                        ("swap_alpha", {ma: T[2]}), ("swap_4x4", {ma: T[3], mo: T[3]}), ("swap_npot", {ma: T[4]}),
                        ("swap_none", {mo: -1})):
        b.frames.append(dict(family=name, light=0, insts=insts, table=table, share="swap"))


_GENERATORS = (_texel, _thresh, _persp, _cross, _tie, _range, _light, _trim, _clip, _swap)


def _place_keypoints(exp, rng, Wd, Hd, cx, cy, prefer=None):
    """N_KP float32 camera-space points for a frame: on centres of drawn, decided pixels (of ``prefer``, a
    mask, where it has any) with W exactly the drawn depth (vis 2) and one float32 step behind it (vis 1);
    on the last column and row; at u = W (outside); behind the near plane."""
    ok = (exp["ids"] >= 0) & ~exp["undecided"]
    if prefer is not None and (ok & prefer).any():
        ok &= prefer
    ys, xs = np.nonzero(ok)
    pts = []
    f = np.float32

    def at(u, v, w):
        w = f(w)
        return [f(f(u - cx) * w / f(256.0)), f(-(f(v - cy) * w / f(256.0))), -w]
    for j in range(4):
        if ys.size == 0:
            pts.append(at(1.5, 1.5, 3.0))
            continue
        k = int(rng.integers(ys.size))
        d = exp["depth"][ys[k], xs[k]]
        w = d if j % 2 == 0 else np.nextafter(d, f(np.inf))
        pts.append(at(xs[k] + 0.5, ys[k] + 0.5, w))
    pts.append(at(Wd - 0.5, Hd - 0.5, 2.0))
    pts.append(at(Wd - 0.25, 0.5, 1.0))
    pts.append(at(float(Wd), 3.5, 4.0))
    pts.append(at(5.5, 5.5, 0.25))
    return np.array(pts, np.float32)


@functools.lru_cache(maxsize=None)
def batch(Wd, Hd):
    """All frames of one size (every family in both vertex orders, every light set): the scene, the per-frame
    transform sets, lights and keypoints, and the expected outputs (``render``) with keypoint uv and vis.
    Computed once, read-only."""
    from constructionsceneposeestimation_amd.scene.model import Instance, Mesh
    b = _Builder(Wd, Hd)
    for k, gen in enumerate(_GENERATORS):
        gen(b, np.random.default_rng(7000 * Wd + k))
    cx, cy = b.cx, b.cy
    scene = b.scene
    frames = []
    rng = np.random.default_rng(Wd)
    shared = {}
    for spec in b.frames:
        for order in (0, 1):
            insts = [(l, m, [t if order == 0 else swapped(t) for t in tris]) for l, m, tris in spec["insts"]]
            key = (spec.get("share"), order)         # frames of one ``share`` draw the same instances
            first = shared.get(key, len(scene.instances))
            if key[0] is not None:
                shared[key] = first
            for l, m, tris in insts if first == len(scene.instances) else ():
                assert_planes_exact(tris, Wd, Hd, cx, cy)
                pos = np.concatenate([vertices(t, cx, cy) for t in tris]).astype(np.float32)
                idx = np.arange(pos.shape[0], dtype=np.uint32).reshape(-1, 3)
                if all(t["uv"] is not None for t in tris):
                    uvs = np.array([c for t in tris for c in t["uv"]], np.float64).astype(np.float32) / np.float32(UVQ)
                    uvi = idx.copy()
                else:
                    assert scene.materials[m].texture < 0
                    uvs, uvi = np.zeros((0, 2), np.float32), np.zeros((0, 3), np.uint32)
                scene.meshes.append(Mesh(f"{spec['family']}{order}_{len(scene.meshes)}", pos, idx, uvs, uvi, m))
                scene.instances.append(Instance(len(scene.meshes) - 1, np.eye(4), l, l, np.eye(4)))
            table = None
            if spec.get("table") is not None:
                table = np.array([spec["table"].get(m, KEEP_TEXTURE) for m in range(len(scene.materials))], np.int32)
            exp = render(insts, scene, b.lights[spec["light"]], Wd, Hd, cx, cy, first, table)
            kp = _place_keypoints(exp, rng, Wd, Hd, cx, cy, exp["clip_win"] if spec["family"].startswith("clip") else None)
            kuv, kvis = keypoints(kp, exp["depth"], Wd, Hd, cx, cy)
            fr = dict(exp, family=spec["family"], order=order, light=spec["light"], insts=insts, first=first,
                      count=len(insts), kp=kp, kp_uv=kuv, kp_vis=kvis, table=table)
            for a in fr.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            frames.append(fr)
    n, I = len(frames), len(scene.instances)
    assert I < 1 << 12
    models = np.zeros((n, I, 16), np.float32)
    for f, fr in enumerate(frames):
        models[f, fr["first"]:fr["first"] + fr["count"]] = np.eye(4, dtype=np.float32).reshape(16)
    models.setflags(write=False)
    V = np.broadcast_to(np.eye(4), (n, 4, 4)).copy()
    P = np.broadcast_to(projection(cx, cy), (n, 4, 4)).copy()
    return dict(scene=scene, V=V, P=P, models=models, frames=frames, W=Wd, H=Hd, lights=b.lights, rejected=b.rejected,
                undecided_clips=b.undecided_clips, w0_searched=b.w0_searched)


@functools.lru_cache(maxsize=None)
def oracle_frames(Wd, Hd):
    """The CPU oracle's outputs for every frame of ``batch`` (rendered once, shared by the tests)."""
    from constructionsceneposeestimation_amd.packing import pack_scene
    from oracle.oracle import Oracle
    b = batch(Wd, Hd)
    o = Oracle(pack_scene(b["scene"]), Wd, Hd, near=NEAR, far=FAR)
    out = []
    for f, fr in enumerate(b["frames"]):
        st = o.frame_state(models16=b["models"][f], light=b["lights"][fr["light"]], texture_per_material=fr["table"])
        r = st.render(b["V"][f], b["P"][f], extra=True, covered=True)
        r["keypoints_uv"], r["keypoints_vis"] = st.keypoints(b["V"][f], b["P"][f], fr["kp"], r["depth"])
        out.append(r)
    return out


def compare(fr, got, what):
    """``got`` (instance, depth, rgb, normals, points, inst_stats, label_covered of one frame) against the
    frame's expected outputs on decided pixels -> list of failure messages (empty: equal)."""
    bad = []
    ok = ~fr["undecided"]

    def px(name, a, e):
        d = (a != e) if a.ndim == 2 else (a != e).any(-1)
        d &= ok
        if d.any():
            bad.append(f"{what}: {int(d.sum())} pixels of {name} differ, first at (y, x) {np.argwhere(d)[:5].tolist()}")
    px("ids", got["instance"], fr["ids"])
    px("depth", got["depth"].view(np.uint32), fr["depth"].view(np.uint32))
    px("rgb", got["rgb"], fr["rgb"])
    px("normals", got["normals"].view(np.uint16), fr["normals"])
    gp, ep = got["points"], fr["points"]
    px("points", np.where(np.isnan(gp), np.float32(7e37), gp), np.where(np.isnan(ep), np.float32(7e37), ep))
    if not fr["undecided"].any():
        if not np.array_equal(got["inst_stats"], fr["inst_stats"]):
            bad.append(f"{what}: label stats {got['inst_stats'].tolist()} != {fr['inst_stats'].tolist()}")
    else:                                            # the counts can differ by the undecided pixels at the most
        off = np.abs(got["inst_stats"][:, 0].astype(np.int64) - fr["inst_stats"][:, 0].astype(np.int64))
        if off.sum() > 2 * int(fr["undecided"].sum()):
            bad.append(f"{what}: label counts {got['inst_stats'][:, 0].tolist()} != {fr['inst_stats'][:, 0].tolist()}")
    lo = (fr["masks"] & ~fr["und_label"]).reshape(N_LABELS, -1).sum(1)
    hi = (fr["masks"] | fr["und_label"]).reshape(N_LABELS, -1).sum(1)
    cov = got["label_covered"].astype(np.int64)
    if not ((lo <= cov) & (cov <= hi)).all():
        bad.append(f"{what}: label coverage {cov.tolist()} not in {lo.tolist()} .. {hi.tolist()}")
    return bad
