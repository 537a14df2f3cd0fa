"""The area filter of csg_crop_objects_filtered (CSG_CROP_FILTER_AREA), host
side: the NumPy restatement of its spec in include/csg_api.h that the GPU tests
compare against (tests/test_gpu_crop_area.py), the properties that follow from
it, and the bookkeeping of the new entry point (no GPU)."""
import os
import re

import numpy as np
import pytest

from tests.test_object_crops import F32, INFO_DTYPE, restate_crops, restate_sample, slot_is_live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BILINEAR, AREA = 0, 1          # CSG_CROP_FILTER_*, stated here independently


def area_edges(origin, step, S):
    """EX_0 .. EX_S of one axis as Python integers (1/256 source pixel): the
    edges in float32, one rounding per operation, then floor."""
    e = F32(origin) + np.arange(S + 1, dtype=F32) * F32(step)
    assert e.dtype == F32
    scaled = e * F32(256.0)
    assert scaled.dtype == F32
    return [int(v) for v in np.floor(scaled)]


def area_weights(E, size):
    """wx_i(p) for the source columns 0 .. size-1 of the frame, (S, size) int64."""
    lo = np.array(E[:-1], np.int64)[:, None]
    hi = np.array(E[1:], np.int64)[:, None]
    p = np.arange(size, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum(hi, 256 * (p + 1)) - np.maximum(lo, 256 * p))


def slot_is_filtered(slot, S, n_labels, explicit):
    """Whether the area filter makes this slot's RGB: live, minified (a float32
    comparison), and a window within the bounds of explicit boxes."""
    if not slot_is_live(slot, n_labels, explicit):
        return False
    side, x0, y0 = F32(slot["side"]), F32(slot["x0"]), F32(slot["y0"])
    with np.errstate(invalid="ignore", over="ignore"):
        step = side / F32(S)
    return bool(step > F32(1.0) and side <= F32(32768) and abs(x0) <= F32(2 ** 20) and abs(y0) <= F32(2 ** 20))


def restate_area(slot, S, rgb):
    """The S x S x 3 box-filtered RGB of one minified slot from one frame
    (H, W, 3) uint8.  The edges are Python integers; every sum and the division
    are exact in int64 (acc + D / 2 < 2^48)."""
    H, W = rgb.shape[:2]
    step = F32(slot["side"]) / F32(S)
    EX, EY = area_edges(slot["x0"], step, S), area_edges(slot["y0"], step, S)
    assert max(map(abs, EX + EY)) < 2 ** 31
    wx, wy = area_weights(EX, W), area_weights(EY, H)                   # (S, W), (S, H)
    DX, DY = np.diff(np.array(EX, np.int64)), np.diff(np.array(EY, np.int64))
    ok = (DY[:, None] > 0) & (DX[None, :] > 0)                          # [j][i]
    D = np.where(ok, DY[:, None] * DX[None, :], 1)
    out = np.zeros((S, S, 3), np.uint8)
    for c in range(3):
        acc = wy @ rgb[..., c].astype(np.int64) @ wx.T                  # pixels outside the frame add 0
        v = np.where(ok, (acc + (D >> 1)) // D, 0)
        assert v.min() >= 0 and v.max() <= 255
        out[..., c] = v
    return out


def restate_crops_filtered(instance, S, K, n_labels, rgb_filter, rgb=None, **kw):
    """csg_crop_objects_filtered over n frames: restate_crops (restate_sample)
    for everything, and restate_area for the RGB of the filtered slots."""
    out = restate_crops(instance, S, K, n_labels, rgb=rgb, **kw)
    assert rgb_filter in (BILINEAR, AREA)
    if rgb_filter == AREA and rgb is not None:
        explicit = kw.get("info") is not None
        out["crop_rgb"] = out["crop_rgb"].copy()
        for f in range(instance.shape[0]):
            for k in range(K):
                if slot_is_filtered(out["info"][f, k], S, n_labels, explicit):
                    out["crop_rgb"][f, k] = restate_area(out["info"][f, k], S, rgb[f])
    return out


def _slot(label, x0, y0, side):
    s = np.zeros((), INFO_DTYPE)
    s[()] = (label, 0, x0, y0, side, 0, (0, 0))
    return s


def test_integer_window_at_step_2_averages_each_2x2_block():
    rng = np.random.default_rng(41)
    S, x0, y0 = 16, 3, 2
    rgb = rng.integers(0, 256, (40, 44, 3), dtype=np.uint8)
    got = restate_area(_slot(0, x0, y0, 2.0 * S), S, rgb)
    win = rgb[y0:y0 + 2 * S, x0:x0 + 2 * S].astype(np.int64)
    exp = (win[0::2, 0::2] + win[0::2, 1::2] + win[1::2, 0::2] + win[1::2, 1::2] + 2) >> 2
    assert np.array_equal(got, exp)
    # (the bilinear taps of this window sit on the blocks' centres with weights 128: the same bytes;
    # one more half pixel per sample and they no longer are)
    ids = np.zeros(rgb.shape[:2], np.int32)
    assert np.array_equal(restate_sample(_slot(0, x0, y0, 2.0 * S), S, 1, True, ids, rgb=rgb)["crop_rgb"], got)
    wide = _slot(0, x0, y0, 3.0 * S)
    assert not np.array_equal(restate_sample(wide, S, 1, True, ids, rgb=rgb)["crop_rgb"], restate_area(wide, S, rgb))


def test_constant_image_is_reproduced_exactly():
    for value, (x0, y0, side) in ((255, (3.25, 1.6, 27.3)), (1, (0.0, 0.0, 40.0)), (200, (2.7, 5.1, 16.000002)),
                                  (77, (0.5, 0.25, 39.5))):
        rgb = np.full((40, 44, 3), value, np.uint8)
        rgb[..., 1] = 255 - value
        got = restate_area(_slot(0, x0, y0, side), 16, rgb)
        assert (got[..., 0] == value).all() and (got[..., 1] == 255 - value).all() and (got[..., 2] == value).all()


def test_stripes_alias_under_bilinear_and_average_under_area():
    S, H = 16, 70
    W = 4 * S + 8
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[:, (np.arange(W) % 4) >= 2] = 255                 # vertical stripes, period 4 px
    ids = np.zeros((H, W), np.int32)
    for x0 in (1.0, 3.0, 0.5, 2.5):
        slot = _slot(0, x0, 2.0, 4.0 * S)                 # step 4, wholly inside the frame
        bil = restate_sample(slot, S, 1, True, ids, rgb=rgb)["crop_rgb"]
        assert set(np.unique(bil)) <= {0, 255} and len(np.unique(bil)) == 1, x0    # one flat colour: aliased
        area = restate_area(slot, S, rgb)
        assert set(np.unique(area)) <= {127, 128}, x0
    assert {int(np.unique(restate_sample(_slot(0, x0, 2.0, 4.0 * S), S, 1, True, ids, rgb=rgb)["crop_rgb"])[0])
            for x0 in (1.0, 3.0)} == {0, 255}             # ... and which colour depends on the window's phase


def test_pixel_outside_the_frame_counts_as_black():
    rgb = np.full((23, 37, 3), 200, np.uint8)
    got = restate_area(_slot(0, -16.0, 0.0, 32.0), 16, rgb)            # left half outside
    assert not got[:, :8].any() and (got[:11, 8:] == 200).all()
    assert (got[11, 8:] == 100).all() and not got[12:].any()           # row 11 is half below the frame (H = 23)
    whole = restate_area(_slot(0, 0.0, 0.0, 32768.0), 16, rgb)         # step 2048: the frame sits in one crop pixel
    assert whole[0, 0, 0] == (200 * 37 * 23 * 65536 + (2048 * 256) ** 2 // 2) // (2048 * 256) ** 2
    assert not whole.reshape(-1, 3)[1:].any()


@pytest.mark.parametrize("S", [16, 512])
def test_edges_stay_ordered_and_in_range(S):
    rng = np.random.default_rng(43)
    first = float(np.float32(S) * np.nextafter(F32(1), F32(2)))
    sides = [first, 32768.0, float(S) * 1.5] + list(np.exp(rng.uniform(np.log(first), np.log(32768.0), 60)))
    origins = [-2.0 ** 20, 2.0 ** 20, 0.0, -0.5, 2.0 ** 20 - 0.0625] + list(rng.uniform(-2.0 ** 20, 2.0 ** 20, 8))
    smallest = None
    for side in sides:
        side = F32(side)
        step = side / F32(S)
        assert step > F32(1.0)
        for o in origins:
            E = np.array(area_edges(o, step, S), np.int64)
            d = np.diff(E)
            # (at most step 2048, and two edges each rounded by up to 1/16 pixel at an origin of 2^20)
            assert d.min() >= 1 and d.max() <= 2 ** 19 + 64, (side, o)
            assert np.abs(E).max() < 2 ** 31 and np.abs(E).max() < 2 ** 29, (side, o)
            smallest = int(d.min()) if smallest is None else min(smallest, int(d.min()))
    print("smallest edge difference", smallest)


def test_filter_applies_to_minified_live_slots_only():
    S = 16
    assert slot_is_filtered(_slot(1, 0.0, 0.0, 32.0), S, 2, True)
    assert slot_is_filtered(_slot(1, 0.0, 0.0, float(F32(16) * np.nextafter(F32(1), F32(2)))), S, 2, True)
    assert not slot_is_filtered(_slot(1, 0.0, 0.0, 16.0), S, 2, True)          # step exactly 1
    assert not slot_is_filtered(_slot(1, 0.0, 0.0, 11.3), S, 2, True)          # magnified
    assert not slot_is_filtered(_slot(2, 0.0, 0.0, 32.0), S, 2, True)          # dead: label == n_labels
    assert not slot_is_filtered(_slot(1, 0.0, 0.0, float("nan")), S, 2, False)
    assert not slot_is_filtered(_slot(1, 0.0, 0.0, 65536.0), S, 2, False)      # a planned window past the bounds
    assert not slot_is_filtered(_slot(1, 3e6, 0.0, 32.0), S, 2, False)
    assert slot_is_filtered(_slot(1, -7.5, 3.0, 32.0), S, 2, False)


def test_entry_point_is_declared_bound_and_exported():
    from constructionsceneposeestimation_amd import _lib
    assert "csg_crop_objects_filtered" in _lib.EXPORTED
    header = open(os.path.join(ROOT, "include", "csg_api.h")).read()
    assert re.search(r"\bint\s+csg_crop_objects_filtered\s*\(\s*csg_ctx\s*\*\s*ctx,\s*const\s+csg_crop_job\s*\*\s*job,"
                     r"\s*uint32_t\s+rgb_filter,\s*uint32_t\s+n_frames,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"#define\s+CSG_CROP_FILTER_BILINEAR\s+0u", header)
    assert re.search(r"#define\s+CSG_CROP_FILTER_AREA\s+1u", header)
    assert _lib.CROP_FILTERS == {"bilinear": BILINEAR, "area": AREA}
    assert hasattr(_lib.load(), "csg_crop_objects_filtered")
    assert _lib.ABI_VERSION == 14 and re.search(r"#define\s+CSG_ABI_VERSION\s+14\b", header)


def test_unknown_filter_name_is_refused_before_the_library_is_called():
    from constructionsceneposeestimation_amd.renderer import Renderer
    with pytest.raises(ValueError, match="rgb_filter"):
        Renderer.crop_objects(None, 1, size=16, per_frame=1, instance=0, info=0, rgb_filter="lanczos")
    with pytest.raises(ValueError, match="rgb_filter"):
        Renderer.render_crops(None, np.zeros(0), rgb_filter="box")
