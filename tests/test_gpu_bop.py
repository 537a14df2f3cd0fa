"""``generate --outputs bop`` end to end on the GPU: the small world of the amodal
span tests (480 x 272), six frames that straddle an epoch, then ``bop merge``.
Every listed object's ``mask_visib`` decodes to ``instance == inst_idx``, its
``mask`` contains it, and the counts and boxes of ``scene_gt_info.json`` are
those of the PNGs; the depth PNG holds ``writers.depth_to_u16``.  The ids and
the float depth come from a second run with other outputs."""
import json
import os

import numpy as np
import pytest

from constructionsceneposeestimation_amd import bop, masks, writers
from tests.test_compact_files import decode_png16
from tests.test_crop_amodal import H3, W3
from tests.test_mask_png import decode_grey_png

pytestmark = pytest.mark.gpu
FRAMES = [7, 8, 9, 10, 11, 12]


def _box(m):
    ys, xs = np.nonzero(m)
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from constructionsceneposeestimation_amd.generate import generate
    d = tmp_path_factory.mktemp("bop")
    kw = dict(workload="C3", seed=2, batch=4, width=W3, height=H3, writers=2)
    generate(str(d / "bop"), FRAMES, outputs=("bop",), **kw)
    generate(str(d / "ref"), FRAMES, outputs=("rgb", "mask", "mask_rle", "amodal_rle", "depth_npy", "depth16_png"), **kw)
    bop.merge(str(d / "bop"))
    return str(d / "bop"), str(d / "ref")


def test_masks_counts_and_boxes(runs):
    out, ref = runs
    sdir = bop.scene_dir(out, 0)
    cam, gt, info = (json.load(open(os.path.join(sdir, n))) for n in
                     ("scene_camera.json", "scene_gt.json", "scene_gt_info.json"))
    want_ids = [str(f) for f in FRAMES]
    assert list(cam) == want_ids and list(gt) == want_ids and list(info) == want_ids
    objects = json.load(open(os.path.join(out, "models", "objects.json")))
    n_listed = n_hidden_part = 0
    for f in FRAMES:
        ids = np.load(os.path.join(ref, "labels", f"instance_mask_{f:06d}.npy"))
        g, gi = gt[str(f)], info[str(f)]
        assert len(g) == len(gi)
        assert [o["obj_id"] for o in g] == sorted(o["obj_id"] for o in g)          # ascending inst_idx
        n_masks = len([p for p in os.listdir(os.path.join(sdir, "mask")) if p.startswith(f"{f:06d}_")])
        assert n_masks == len(g) == len([p for p in os.listdir(os.path.join(sdir, "mask_visib"))
                                         if p.startswith(f"{f:06d}_")])
        for k, (o, i) in enumerate(zip(g, gi)):
            inst = o["obj_id"] - 1
            assert objects[str(o["obj_id"])]["inst_idx"] == inst
            vis_png = open(bop.mask_path(out, "mask_visib", f, k), "rb").read()
            amo_png = open(bop.mask_path(out, "mask", f, k), "rb").read()
            vis, amo = decode_grey_png(vis_png)[0] != 0, decode_grey_png(amo_png)[0] != 0
            assert vis.shape == (H3, W3) and np.array_equal(vis, ids == inst), (f, k)
            assert not (vis & ~amo).any() and amo.any(), (f, k)
            assert vis_png == writers.mask_png_bytes(vis) and amo_png == writers.mask_png_bytes(amo)
            assert i["px_count_visib"] == int(vis.sum()) and i["px_count_all"] == int(amo.sum()) == i["px_count_valid"]
            assert i["bbox_obj"] == _box(amo)
            assert i["bbox_visib"] == (_box(vis) if vis.any() else [-1, -1, -1, -1])
            assert i["visib_fract"] == i["px_count_visib"] / i["px_count_all"]
            R = np.array(o["cam_R_m2c"]).reshape(3, 3)
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-9) and abs(np.linalg.det(R) - 1) < 1e-9
            n_listed += 1
            n_hidden_part += i["px_count_visib"] < i["px_count_all"]
    print("listed objects", n_listed, "partly hidden", n_hidden_part)
    assert n_listed >= 6 and n_hidden_part >= 1


def test_amodal_masks_equal_the_coco_run(runs):
    """The ``mask`` files hold the amodal masks the ``amodal_rle`` output describes."""
    out, ref = runs
    gt = json.load(open(os.path.join(bop.scene_dir(out, 0), "scene_gt.json")))
    n = 0
    for f in FRAMES:
        frag = json.load(open(masks.fragment_path(ref, f)))
        by_inst = {a["inst_idx"]: a for a in frag["annotations"] if "amodal_segmentation" in a}
        for k, o in enumerate(gt[str(f)]):
            a = by_inst.get(o["obj_id"] - 1)
            if a is None:          # wholly hidden: COCO lists only objects with visible pixels
                continue
            amo = decode_grey_png(open(bop.mask_path(out, "mask", f, k), "rb").read())[0] != 0
            seg = a["amodal_segmentation"]
            assert np.array_equal(amo, masks.decode(seg["size"], seg["counts"])), (f, k)
            n += 1
    assert n >= 6


def test_depth_and_rgb_files(runs):
    out, ref = runs
    cam = json.load(open(os.path.join(bop.scene_dir(out, 0), "scene_camera.json")))
    for f in FRAMES:
        depth = np.load(os.path.join(ref, "depth", f"depth_{f:06d}.npy"))
        png = open(bop.image_path(out, "depth", f), "rb").read()
        u16 = decode_png16(png)
        assert np.array_equal(u16, writers.depth_to_u16(depth))
        assert cam[str(f)]["depth_scale"] == 4.0
        mm, ok = u16.astype(np.float64) * cam[str(f)]["depth_scale"], (u16 > 0) & (u16 < 65535)
        assert np.abs(mm[ok] - depth[ok].astype(np.float64) * 1000.0).max() <= 2.0 + 1e-3     # half a 4 mm step
        # the same encoders as the outputs under their own names: the same bytes
        assert png == open(os.path.join(ref, "depth", f"depth16_{f:06d}.png"), "rb").read()
        assert open(bop.image_path(out, "rgb", f), "rb").read() == open(
            os.path.join(ref, "rgb", f"rgb_{f:06d}.png"), "rb").read()
    assert json.load(open(os.path.join(out, "camera.json")))["depth_scale"] == 4.0
    assert os.path.exists(os.path.join(out, "labels", f"label_{FRAMES[0]:06d}.json"))              # the resume marker


def test_refused_combinations(tmp_path):
    from constructionsceneposeestimation_amd.generate import generate
    kw = dict(workload="C3", seed=2, batch=2, width=W3, height=H3, writers=2)
    with pytest.raises(ValueError):
        generate(str(tmp_path / "a"), [0], outputs=("bop", "mask_rle"), **kw)
    with pytest.raises(ValueError):
        generate(str(tmp_path / "b"), [0], outputs=("bop",), depth16_counts_per_metre=0.5, **kw)   # near reads 0 counts
    with pytest.raises(ValueError):
        generate(str(tmp_path / "c"), [0], outputs=("bop",), writer_mode="process", **kw)
