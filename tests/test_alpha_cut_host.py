"""CPU test of csg_alpha_cut.h, the cut of the alpha trim:
a stand-alone driver (tests/alpha_cut_host.cpp, built with AddressSanitizer and
UBSan) cuts the pixel boxes of seeded records, and every box is checked by brute
force over every centre of the input box:

* safe: every centre inside the (closed) snapped triangle whose four float
  half-plane values, evaluated as the header evaluates them
  (``(h0 * x + h1 * y) + h2`` with ``h = sg * (P - bound * D)``, one float32
  rounding per operation), are all >= -m lies in the returned box;
* not loose (coordinates below 2^12 px): the box is within one pixel per side of
  the exact box of the clipped polygon.  The polygon is the snapped triangle
  clipped in rational arithmetic, per half-plane, at g >= -12 m (kCutOuter: the
  outermost level at which the header, by its proof, may still take a vertex
  for "in"; 12 m is below 0.2 px of distance at these coordinates), the four
  boxes and the input box intersected.  An empty polygon means "none left";
* a NaN or an infinity in the planes leaves the box unchanged.

``m`` is the guard's: 2^-20 (S + B S_D) in float32.  The kinds of case the seeded
set must hold are counted from the exact reference alone (the facts of ``_reference``)."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
OUTER = 12


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("alpha_cut") / "alpha_cut_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "alpha_cut_host.cpp"), "-o", out], check=True)
    return out


def _bits(x):
    return f"{np.array(x, F).view(np.uint32):08x}"


def _run(exe, cases):
    text = [str(len(cases))]
    for c in cases:
        text.append(" ".join(str(int(v)) for v in c["xy"]) + " " +
                    " ".join(_bits(v) for v in list(c["U"]) + list(c["V"]) + list(c["D"]) + list(c["bx"]) + [c["m"]]) +
                    " " + " ".join(str(int(v)) for v in c["box"]))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True)
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def _guard_m(xy, U, V, D, bx):
    """The guard's m in float32 (X, Y: the largest vertex coordinate in pixels, plus one)."""
    X = F(np.abs(np.array(xy[:3], np.float64)).max() / 256.0 + 1.0)
    Y = F(np.abs(np.array(xy[3:], np.float64)).max() / 256.0 + 1.0)
    with np.errstate(all="ignore"):
        s = [F(F(F(abs(P[0]) * X) + F(abs(P[1]) * Y)) + abs(P[2])) for P in (U, V, D)]
        B = F(np.abs(np.array(bx, F)).max())
        return F(F(2.0 ** -20) * F(max(s[0], s[1]) + F(B * s[2])))


def _make(xy, U, V, D, bx, box=None, m=None, tag=""):
    xy = [int(v) for v in xy]
    U, V, D, bx = (np.array(a, F) for a in (U, V, D, bx))
    if box is None:     # as make_rec: the centres inside the vertices' extent, at most 40 x 40, not below 0
        x, y = xy[:3], xy[3:]
        box = [max((min(x) - 128 + 255) >> 8, 0), max((min(y) - 128 + 255) >> 8, 0), (max(x) - 128) >> 8, (max(y) - 128) >> 8]
        box[2], box[3] = min(box[2], box[0] + 39), min(box[3], box[1] + 39)
    assert 0 <= box[0] <= box[2] < 65536 and 0 <= box[1] <= box[3] < 65536 and box[2] - box[0] < 40 and box[3] - box[1] < 40
    area = (xy[1] - xy[0]) * (xy[5] - xy[3]) - (xy[2] - xy[0]) * (xy[4] - xy[3])
    assert area != 0
    return dict(xy=xy, U=U, V=V, D=D, bx=bx, box=box, m=_guard_m(xy, U, V, D, bx) if m is None else F(m), tag=tag)


def _coeffs(c):
    """The four half-planes' float32 coefficients, as the header forms them."""
    out = []
    with np.errstate(all="ignore"):
        for k in range(4):
            P, sg = (c["U"] if k < 2 else c["V"]), F(-1.0 if k & 1 else 1.0)
            out.append([F(sg * F(P[i] - F(c["bx"][k] * c["D"][i]))) for i in range(3)])
    return out


def _frame(angle, scale, centre, uv0=(0.5, 0.5), persp=(0.0, 0.0)):
    """Planes of a uv frame rotated by `angle` on screen: `scale` uv per pixel, uv0 at `centre`, D = 1 there."""
    c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    cx, cy = centre
    D = np.array([persp[0], persp[1], 1.0 - persp[0] * cx - persp[1] * cy])
    Ua = np.array([scale * c, scale * s, uv0[0] - scale * (c * cx + s * cy)])
    Va = np.array([-scale * s, scale * c, uv0[1] - scale * (-s * cx + c * cy)])
    # u = U / D with U = Ua * D at first order: keep it simple, U = Ua + uv0 * (D - 1)
    U = Ua + uv0[0] * (D - [0.0, 0.0, 1.0])
    V = Va + uv0[1] * (D - [0.0, 0.0, 1.0])
    return U, V, D


def _cases():
    rng = np.random.default_rng(20240607)
    cases = []

    def tri(ox, oy, size=40.0):
        while True:
            p = rng.uniform(0.0, size, (3, 2)) + [ox, oy]
            xy = np.rint(p * 256.0).astype(np.int64)
            if (xy[1, 0] - xy[0, 0]) * (xy[2, 1] - xy[0, 1]) - (xy[2, 0] - xy[0, 0]) * (xy[1, 1] - xy[0, 1]) != 0:
                return [xy[0, 0], xy[1, 0], xy[2, 0], xy[0, 1], xy[1, 1], xy[2, 1]]

    def uvbox(scale, spread=25.0):
        lo = 0.5 + scale * rng.uniform(-spread, spread * 0.6, 2)
        hi = lo + scale * rng.uniform(0.3, spread, 2)
        return [lo[0], hi[0], lo[1], hi[1]]

    # random triangles and frames, near the origin and at a few thousand pixels; some with perspective
    for n in range(220):
        ox, oy = (rng.integers(0, 30, 2) if n % 3 else rng.integers(1000, 4000, 2))
        xy = tri(ox, oy)
        angle = (30.0, 45.0, 60.0)[n % 3] + 90.0 * (n % 4) if n % 2 else rng.uniform(0.0, 360.0)
        scale = 2.0 ** rng.uniform(-8.0, -4.0)
        persp = rng.uniform(-2e-3, 2e-3, 2) if n % 5 == 0 else (0.0, 0.0)
        U, V, D = _frame(angle, scale, (ox + 20.0, oy + 20.0), persp=persp)
        cases.append(_make(xy, U, V, D, uvbox(scale), tag="random"))
    # u = x, v = y (exact coefficients): a vertex exactly on a line, lines parallel to edges
    for n in range(24):
        ox, oy = rng.integers(0, 50, 2)
        xy = tri(ox, oy)
        k = n % 3
        vx, vy = xy[k] / 256.0, xy[3 + k] / 256.0
        bx = [vx, vx + 7.0, oy - 1.0, oy + 50.0] if n % 2 else [ox - 1.0, ox + 50.0, vy - 6.0, vy]
        cases.append(_make(xy, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], bx, tag="on the line"))
    for n in range(24):
        ox, oy = (int(v) for v in rng.integers(0, 50, 2))
        a, b, h = (int(v) for v in rng.integers(256, 40 * 256, 3))
        if n % 2:      # a vertical edge x = ox, and u = x: the lines u = bound are parallel to it
            xy = [ox * 256, ox * 256, ox * 256 + h, oy * 256, oy * 256 + a, oy * 256 + b]
            off = (0.0, 1.0 / 256.0, -1.0 / 256.0, 3.0)[n // 2 % 4]
            bx = [ox + off, ox + off + 9.0, oy - 1.0, oy + 50.0]
            U, V = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
        else:          # an edge along (1, 1), and u = x - y
            xy = [ox * 256, ox * 256 + a, ox * 256 + h, oy * 256, oy * 256 + a, oy * 256 + (h - 256) // 2]
            off = (0.0, 1.0 / 256.0, -1.0 / 256.0, 2.5)[n // 2 % 4]
            bx = [float(ox - oy) + off, float(ox - oy) + off + 11.0, -100.0, 100.0]
            U, V = [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]
        area = (xy[1] - xy[0]) * (xy[5] - xy[3]) - (xy[2] - xy[0]) * (xy[4] - xy[3])
        if area != 0:
            cases.append(_make(xy, U, V, [0.0, 0.0, 1.0], bx, tag="parallel"))
    # slivers 1/256 px wide, along x, y and slanted, at small and at large coordinates
    for n in range(36):
        ox, oy = (int(v) for v in (rng.integers(0, 40, 2) if n % 2 else rng.integers(3000, 4000, 2)))
        L = int(rng.integers(5 * 256, 38 * 256))
        x0, y0 = ox * 256 + int(rng.integers(0, 256)), oy * 256 + int(rng.integers(0, 256))
        if n % 3 == 0:
            y0 = oy * 256 + 128      # (the sliver lies on a row, or a column, of centres)
        elif n % 3 == 1:
            x0 = ox * 256 + 128
        t = int(rng.integers(1, L))
        if n % 3 == 0:
            xy = [x0, x0 + L, x0 + t, y0, y0, y0 + 1]
        elif n % 3 == 1:
            xy = [x0, x0, x0 + 1, y0, y0 + L, y0 + t]
        else:
            xy = [x0, x0 + L, x0 + t, y0, y0 + L, y0 + t + 1]
        scale = 2.0 ** -6
        U, V, D = _frame(rng.uniform(0.0, 360.0), scale, (ox + 15.0, oy + 10.0))
        cases.append(_make(xy, U, V, D, uvbox(scale, 12.0), tag="sliver"))
    # a vertex at 2^19 px; the record's box is the part of it on a small screen
    for n in range(12):
        far = 2 ** 19 * 256
        xy = [int(rng.integers(0, 30 * 256)), far if n % 2 else int(rng.integers(0, 30 * 256)), int(rng.integers(0, 30 * 256)),
              int(rng.integers(0, 30 * 256)), int(rng.integers(0, 60 * 256)), int(rng.integers(0, 30 * 256)) if n % 2 else -far]
        if (xy[1] - xy[0]) * (xy[5] - xy[3]) - (xy[2] - xy[0]) * (xy[4] - xy[3]) == 0:
            continue
        scale = 2.0 ** -5
        U, V, D = _frame(rng.uniform(0.0, 360.0), scale, (15.0, 15.0))
        cases.append(_make(xy, U, V, D, uvbox(scale, 10.0), box=[0, 0, 39, 39], tag="far"))
    # strips in u and in v that each cross the triangle, and meet outside it
    for n in range(8):
        ox, oy = (int(v) for v in rng.integers(0, 40, 2))
        xy = [ox * 256, (ox + 30) * 256, ox * 256, oy * 256, oy * 256, (oy + 30) * 256]
        a, b = rng.uniform(19.0, 23.0, 2)
        bx = [ox + a, ox + a + 4.0, oy + b, oy + b + 4.0]
        cases.append(_make(xy, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], bx, tag="meet outside"))
    # NaN and infinite planes
    xy = tri(3, 4)
    U, V, D = _frame(30.0, 2.0 ** -5, (20.0, 20.0))
    for n, bad in enumerate((np.nan, np.inf, -np.inf)):
        for which in range(3):
            P = [np.array(U), np.array(V), np.array(D)]
            P[which][(n + which) % 3] = bad
            cases.append(_make(xy, P[0], P[1], P[2], [0.4, 0.6, 0.4, 0.6], m=2.0 ** -18, tag="not finite"))
    cases.append(_make(xy, U * 3e38, V, D * 3e38, [0.4, 1e30, 0.4, 0.6], m=2.0 ** 100, tag="not finite"))
    return cases


def _frac(v):
    return Fraction(float(v))


def _clip(poly, h, level):
    """Sutherland-Hodgman in rationals: the part of `poly` with h0 x + h1 y + h2 >= level."""
    out = []
    g = [h[0] * p[0] + h[1] * p[1] + h[2] - level for p in poly]
    for i, p in enumerate(poly):
        q, gp, gq = poly[(i + 1) % len(poly)], g[i], g[(i + 1) % len(poly)]
        if gp >= 0:
            out.append(p)
        if (gp >= 0) != (gq >= 0):
            t = gp / (gp - gq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def _reference(c):
    """Exact quantities of one finite case: the kept centres (bool image over the input box), the reference
    pixel box (or None: some polygon is empty), and the facts `_kinds` counts."""
    xy, box = c["xy"], c["box"]
    hf = _coeffs(c)
    m = c["m"]
    # the closed snapped triangle, in integers
    x, y = xy[:3], xy[3:]
    area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    o = 1 if area > 0 else -1
    px = np.arange(box[0], box[2] + 1, dtype=np.int64)[None, :]
    py = np.arange(box[1], box[3] + 1, dtype=np.int64)[:, None]
    cx, cy = px * 256 + 128, py * 256 + 128
    keep = np.ones((py.size, px.size), bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        keep &= o * ((x[b] - x[a]) * (cy - y[a]) - (y[b] - y[a]) * (cx - x[a])) >= 0
    fx, fy = (px + 0.5).astype(F), (py + 0.5).astype(F)
    for h in hf:
        keep &= ((h[0] * fx + h[1] * fy) + h[2]) >= -m          # float32, one rounding per operation
    # exact polygons
    T = [(Fraction(x[k], 256), Fraction(y[k], 256)) for k in range(3)]
    H = [[_frac(v) for v in h] for h in hf]
    mf = _frac(m)
    ref = [Fraction(box[0]) + Fraction(1, 2), Fraction(box[2]) + Fraction(1, 2), Fraction(box[1]) + Fraction(1, 2),
           Fraction(box[3]) + Fraction(1, 2)]
    empty = False
    for h in H:
        poly = _clip(T, h, -OUTER * mf)
        if not poly:
            empty = True
            break
        ref[0], ref[1] = max(ref[0], min(p[0] for p in poly)), min(ref[1], max(p[0] for p in poly))
        ref[2], ref[3] = max(ref[2], min(p[1] for p in poly)), min(ref[3], max(p[1] for p in poly))
    half = Fraction(1, 2)
    refpx = None if empty else [math.ceil(ref[0] - half), math.ceil(ref[2] - half), math.floor(ref[1] - half),
                                math.floor(ref[3] - half)]
    # facts for the sanity counts (exact, at the level -m)
    facts = dict(nin=set(), on_line=False, parallel=False, small_diff=False, rotated=set(), meet_outside=False)
    alone, allp = True, list(T)
    for h in H:
        g = [h[0] * p[0] + h[1] * p[1] + h[2] for p in T]
        facts["nin"].add(sum(v >= -mf for v in g))
        facts["on_line"] |= any(v == 0 for v in g) and (h[0] != 0 or h[1] != 0)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ex, ey = T[b][0] - T[a][0], T[b][1] - T[a][1]
            facts["parallel"] |= (h[0] * ex + h[1] * ey == 0) and (h[0] != 0 or h[1] != 0)
            facts["small_diff"] |= abs(g[a] - g[b]) < mf
        if h[0] != 0 or h[1] != 0:
            ang = math.degrees(math.atan2(float(h[1]), float(h[0]))) % 90.0
            for t in (30.0, 45.0, 60.0):
                if abs(ang - t) < 0.5:
                    facts["rotated"].add(t)
        alone &= bool(_clip(T, h, -mf))
        if allp:
            allp = _clip(allp, h, -mf)
    facts["meet_outside"] = alone and not allp
    w = max(max(abs(v) for v in x), max(abs(v) for v in y))
    facts["far"] = w >= 2 ** 19 * 256
    edges = [math.hypot(x[b] - x[a], y[b] - y[a]) for a, b in ((0, 1), (1, 2), (2, 0))]
    facts["sliver"] = abs(area) / max(edges) <= 1.0 + 1e-9        # width in 1/256 px
    return keep, refpx, facts


def test_boxes_against_brute_force(exe):
    cases = _cases()
    got = _run(exe, cases)
    kinds = dict(in0=0, in1=0, in2=0, in3=0, on_line=0, parallel=0, small_diff=0, sliver=0, far=0, rot30=0, rot45=0,
                 rot60=0, meet_outside=0, not_finite=0, none_left=0, cut=0, loose_checked=0)
    for c, (left, px0, py0, px1, py1) in zip(cases, got):
        box = c["box"]
        what = (f"{c['tag']}: xy {c['xy']} U {c['U'].tolist()} V {c['V'].tolist()} D {c['D'].tolist()} bx {c['bx'].tolist()} "
                f"m {float(c['m'])} box {box} -> {left} {[px0, py0, px1, py1]}")
        if c["tag"] == "not finite":
            assert left == 1 and [px0, py0, px1, py1] == box, f"changed: {what}"
            kinds["not_finite"] += 1
            continue
        keep, refpx, facts = _reference(c)
        # safe
        if keep.any():
            assert left == 1, f"unsafe (dropped): {what}"
            ys, xs = np.nonzero(keep)
            assert (px0 <= box[0] + xs.min() and box[0] + xs.max() <= px1 and
                    py0 <= box[1] + ys.min() and box[1] + ys.max() <= py1), f"unsafe: {what}"
        if left:
            assert box[0] <= px0 <= px1 <= box[2] and box[1] <= py0 <= py1 <= box[3], f"outside its box: {what}"
            kinds["cut"] += [px0, py0, px1, py1] != box
        else:
            kinds["none_left"] += 1
        # not loose
        if max(abs(v) for v in c["xy"]) < 2 ** 12 * 256:
            kinds["loose_checked"] += 1
            if refpx is None:
                assert left == 0, f"loose (an empty polygon): {what}"
            elif left:
                assert (px0 >= refpx[0] - 1 and py0 >= refpx[1] - 1 and px1 <= refpx[2] + 1 and
                        py1 <= refpx[3] + 1), f"loose: reference {refpx}: {what}"
        for n in facts["nin"]:
            kinds[f"in{n}"] += 1
        for key in ("on_line", "parallel", "small_diff", "sliver", "far", "meet_outside"):
            kinds[key] += bool(facts[key])
        for t in facts["rotated"]:
            kinds[f"rot{int(t)}"] += 1
    print(kinds)
    for key, least in dict(in0=20, in1=20, in2=20, in3=20, on_line=10, parallel=10, small_diff=10, sliver=20, far=8,
                           rot30=10, rot45=10, rot60=10, meet_outside=4, not_finite=10, none_left=10, cut=100,
                           loose_checked=250).items():
        assert kinds[key] >= least, (key, kinds)
