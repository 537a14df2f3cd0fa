"""The CPU oracle against the exact integer coverage reference of
tests/raster_exact.py (no GPU): ids, label stats and label coverage on every
frame of every family, and the conditions the reference rests on -- exact float32
inputs (asserted while the scenes are built), the condition cap, the fill of every
frame, the depth ratio that keeps layers from swapping, and that each family
really holds the case it is named after.  tests/test_gpu_raster_exact.py runs
the same frames through the kernels."""
import numpy as np
import pytest

from tests import raster_exact as rx

SIZES = [pytest.param(s, id=f"{s[0]}x{s[1]}") for s in rx.SIZES]


def test_edge_rule_by_hand():
    """The reference itself on cases small enough to decide by hand (y grows downwards)."""
    c = lambda px, py: (px * 256 + 128, py * 256 + 128)      # noqa: E731  the centre of a pixel
    # a right triangle with its legs through centres: the top and the left edge cover them, the
    # hypotenuse (a right / bottom edge) does not; both vertex orders
    for t in ([c(0, 0), c(2, 0), c(0, 2)], [c(0, 0), c(0, 2), c(2, 0)]):
        assert np.argwhere(rx.edge_cover(t, 4, 4)).tolist() == [[0, 0], [0, 1], [1, 0]]
    # an axis-aligned box from centre (1, 1) to centre (3, 2), as two triangles: the left column and the top
    # row of centres are in, the right column and the bottom row are out, the diagonal is covered once
    a, b, cc, d = c(1, 1), c(3, 1), c(3, 2), c(1, 2)
    m0, m1 = rx.edge_cover([a, b, cc], 5, 4), rx.edge_cover([a, cc, d], 5, 4)
    assert not (m0 & m1).any() and np.argwhere(m0 | m1).tolist() == [[1, 1], [1, 2]]
    # one unit makes the difference
    assert rx.edge_cover([(128, 128), (129, 128), (128, 129)], 2, 2).sum() == 1
    assert rx.edge_cover([(129, 128), (130, 128), (129, 129)], 2, 2).sum() == 0
    # the guard: exactly 2^20 px drops the triangle, 32 units less keeps it; zero area drops it
    far = [(100, 100), (100, 5000), (rx.GUARD, 2000)]
    near = [(100, 100), (100, 5000), (rx.GUARD - 32, 2000)]
    assert rx.dropped(far) and not rx.cover(far, 8, 8).any() and rx.edge_cover(far, 8, 8).any()
    assert not rx.dropped(near) and np.array_equal(rx.cover(near, 8, 8), rx.edge_cover(near, 8, 8))
    assert rx.cover([(-rx.GUARD, 0), (100, 100), (100, 5000)], 8, 8).sum() == 0
    assert rx.dropped([(0, 0), (512, 512), (1024, 1024)])
    # the cap: max(|U|, |V|)^2 <= 2^16 |2 area|
    assert rx.within_cap([(0, 0), (65536, 0), (0, 65536)])
    assert rx.within_cap([(0, 0), (1 << 20, 0), (0, 16)]) and not rx.within_cap([(0, 0), (1 << 20, 0), (1, 15)])


def _small_record(t, W, H):
    """Whether make_rec's exact cover test applies (csg_raster_math.h: a box of at most 4 x 4 centres,
    clamped to the frame, and a vertex extent below 8192 units) -> (box is small, extent, box size)."""
    xs, ys = [p[0] for p in t], [p[1] for p in t]
    px0, px1 = max((min(xs) - 128 + 255) >> 8, 0), min((max(xs) - 128) >> 8, W - 1)
    py0, py1 = max((min(ys) - 128 + 255) >> 8, 0), min((max(ys) - 128) >> 8, H - 1)
    small = 0 <= px1 - px0 < 4 and 0 <= py1 - py0 < 4
    return small, max(max(xs) - min(xs), max(ys) - min(ys)), (px1 - px0 + 1, py1 - py0 + 1)


@pytest.mark.parametrize("size", SIZES)
def test_conditions_of_the_reference(size):
    W, H = size
    b = rx.batch(W, H)
    fam = {}
    assert [(f["family"], f["order"]) for f in b["frames"]] == [(n, o) for n in rx.FAMILIES for o in (0, 1)]
    for k, fr in enumerate(b["frames"]):
        what = f'{fr["family"]}/{fr["order"]}'
        fill = float((fr["ids"] >= 0).mean())
        pops = fr["masks"].reshape(rx.N_LABELS, -1).sum(1)
        print(f"{W}x{H} {what}: covered {fill:.3f}, layers {pops.tolist()}")
        assert 0.2 <= fill <= 0.8, what
        assert (pops[:len(rx.LAYERS)] > 0).all() and (pops[:len(rx.LAYERS)] < W * H).all(), what
        assert (pops[len(rx.LAYERS):] == 0).all()
        for l in range(len(rx.LAYERS), rx.N_LABELS):          # ... though their triangles lie over the frame
            assert sum(int(rx.edge_cover(t, W, H).sum()) for t in fr["layers"][l]) > W * H // 10, what
        assert all(rx.within_cap(t) for tris in fr["layers"] for t in tris)
        if fr["order"]:                                        # the other vertex order: the same images
            prev = b["frames"][k - 1]
            assert np.array_equal(fr["ids"], prev["ids"]) and np.array_equal(fr["masks"], prev["masks"])
            assert all(area2 == -prev2 for area2, prev2 in zip(
                (rx.area2(t) for tris in fr["layers"] for t in tris),
                (rx.area2(t) for tris in prev["layers"] for t in tris)))
        fam[fr["family"]] = fr
        seen = np.unique(fr["ids"]).tolist()                  # background and at least four layers are visible
        assert seen[0] == -1 and len(seen) >= 5 and seen[-1] < len(rx.LAYERS), what
    visible = [t for tris in fam["tiny"]["layers"][:len(rx.LAYERS)] for t in tris]
    small = [_small_record(t, W, H) for t in visible]
    assert sum(s and e < 8192 for s, e, _ in small) >= 50         # the exact cover test of small records ...
    assert sum(s and e == 8191 for s, e, _ in small) >= 5         # ... up to its limit
    assert sum(s and e == 8192 for s, e, _ in small) >= 5 and sum(s and e == 8193 for s, e, _ in small) >= 5
    boxes = {box for s, e, box in small if s and e < 8192}
    assert {(1, 1), (4, 4)} <= boxes and len(boxes) >= 12, sorted(boxes)
    empty = sum(s and e < 8192 and not rx.cover(t, W, H).any() for (s, e, _), t in zip(small, visible))
    assert empty >= 5                                              # small records that cover no centre are dropped
    far = [max(max(abs(x), abs(y)) for x, y in t) for tris in fam["wedge"]["layers"][:len(rx.LAYERS)] for t in tris]
    assert {e for e in range(20, 28) if any(v == (1 << e) - (1 << (e - 10)) for v in far)} == set(range(20, 28))
    ext = _tile_edge_extremes(fam["wedge"], W, H)
    assert ext["first"] >= 2 and ext["last"] >= 2, ext
    slant = [max(t, key=lambda p: abs(p[0])) for tris in fam["diag"]["layers"][:len(rx.LAYERS)] for t in tris]
    assert len(slant) >= 20 and all(min(abs(x), abs(y)) >= 1 << 22 for x, y in slant)   # far out in x and in y
    assert {(x > 0, y > 0) for x, y in slant} == {(a, b) for a in (False, True) for b in (False, True)}
    graze = [t for tris in fam["graze"]["layers"][:len(rx.LAYERS)] for t in tris]
    assert len(graze) >= 14 and sum(_grazed_centres(t, W, H) > 0 for t in graze) == len(graze)
    g = [t for tris in fam["guard"]["layers"][:len(rx.LAYERS)] for t in tris]
    assert sum(rx.dropped(t) for t in g) >= 14 and sum(not rx.dropped(t) and rx.cover(t, W, H).any() for t in g) >= 14
    assert fam["guard"]["would_cover"] >= 200                      # the dropped ones would have shown
    flat = [t for tris in fam["flat"]["layers"][:len(rx.LAYERS)] for t in tris]
    assert sum(rx.area2(t) == 0 for t in flat) >= 40
    assert sum(flat.count(t) >= 2 for t in flat if rx.area2(t) != 0) >= 14
    assert all(f["would_cover"] == 0 for n, f in fam.items() if n != "guard")
    on_centres = [t for tris in fam["centre"]["layers"][:len(rx.LAYERS)] for t in tris]
    assert all(x % 256 == 128 and y % 256 == 128 for t in on_centres for x, y in t)
    corners = [(x, y) for tris in fam["tile"]["layers"][:len(rx.LAYERS)] for t in tris for x, y in t]
    assert all((x + 128) % (rx.TILE_W * 256) in (0, 128, 256) and (y + 128) % (rx.TILE_H * 256) in (0, 128, 256)
               for x, y in corners)


def _grazed_centres(t, W, H):
    """Covered centres on the first / last column or row of a tile that lie within 42 units (40 and the rounding of the near vertex; in y for a
    column, in x for a row) of an edge to the far vertex: |edge function| <= 40 |dx| (or |dy|)."""
    m = rx.edge_cover(t, W, H)
    far = max(t, key=lambda p: abs(p[0]))
    n = 0
    for a in t:
        if a is far:
            continue
        dx, dy = far[0] - a[0], far[1] - a[1]
        for py, px in np.argwhere(m):
            e = abs(dx * (int(py) * 256 + 128 - a[1]) - dy * (int(px) * 256 + 128 - a[0]))
            on_col = px % rx.TILE_W in (0, rx.TILE_W - 1) or px == W - 1
            on_row = py % rx.TILE_H in (0, rx.TILE_H - 1) or py == H - 1
            n += int((on_col and e <= 42 * abs(dx)) or (on_row and e <= 42 * abs(dy)))
    return n


def _tile_edge_extremes(fr, W, H):
    """How many wedges of a frame have their extreme covered centre on the first (``first``) or last
    (``last``) pixel column / row of a 32 x 16 tile, at the end where their two near vertices are."""
    n = dict(first=0, last=0)
    for tris in fr["layers"][:len(rx.LAYERS)]:
        for t in tris:
            m = rx.cover(t, W, H)
            if not m.any():
                continue
            far = max(t, key=lambda p: max(abs(p[0]), abs(p[1])))
            axis = 0 if abs(far[0]) > abs(far[1]) else 1
            along = np.nonzero(m)[1 - axis]                    # columns for a wedge in x, rows for one in y
            tile = rx.TILE_W if axis == 0 else rx.TILE_H
            if far[axis] > 0:
                n["first"] += int(along.min() % tile == 0 and along.min() > 0)
            else:
                n["last"] += int(along.max() % tile == tile - 1 and along.max() < (W, H)[axis] - 1)
    return n


@pytest.mark.parametrize("size", SIZES)
def test_oracle_matches_the_integer_reference(size):
    W, H = size
    b, ora = rx.batch(W, H), rx.oracle_frames(W, H)
    for fr, o in zip(b["frames"], ora):
        what = f'{W}x{H} {fr["family"]}/{fr["order"]}'
        bad = np.argwhere(o["instance"] != fr["ids"])
        assert len(bad) == 0, f"{what}: {len(bad)} ids differ, first at (y, x) {bad[:5].tolist()}"
        assert np.array_equal(o["inst_stats"], fr["inst_stats"]), what
        assert np.array_equal(o["label_covered"], fr["covered"]), what
        assert np.isinf(o["depth"][fr["ids"] < 0]).all(), what


@pytest.mark.parametrize("size", SIZES)
def test_oracle_depth_stays_in_its_layer(size):
    """Layers are a factor 2 apart; under the condition cap the depth of a covered pixel is within a
    factor 2^(1/4) of its layer's distance, so no two layers can swap."""
    W, H = size
    b, ora = rx.batch(W, H), rx.oracle_frames(W, H)
    lay = np.array(rx.DISTANCES)
    lo, hi = 1.0, 1.0
    for fr, o in zip(b["frames"], ora):
        on = fr["ids"] >= 0
        ratio = o["depth"][on].astype(np.float64) / lay[fr["ids"][on]]
        lo, hi = min(lo, float(ratio.min())), max(hi, float(ratio.max()))
        assert 2.0 ** -0.25 < ratio.min() and ratio.max() < 2.0 ** 0.25, (fr["family"], fr["order"])
    print(f"{W}x{H}: depth / layer distance in [{lo:.6f}, {hi:.6f}]")
