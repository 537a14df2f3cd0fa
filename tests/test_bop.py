"""CPU tests of the BOP writer (bop.py): the pose conversion against the
schedule's own float64 projection, the fragment schema, scene and image
numbering across the 1,000-frame boundary, merging shards, and the output sets
``parse_outputs`` accepts."""
import json
import os

import numpy as np
import pytest

from constructionsceneposeestimation_amd import bop
from constructionsceneposeestimation_amd.crops import DYNAMIC_KINDS, eligible_labels
from constructionsceneposeestimation_amd.generate import parse_outputs
from constructionsceneposeestimation_amd.labels import object_box
from constructionsceneposeestimation_amd.workload import Workload

W, H = 480, 272
EMPTY = (0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0)


@pytest.fixture(scope="module")
def wl():
    return Workload("C3", seed=2, width=W, height=H)


def _stats(wl, seed):
    """Made-up label statistics: every other label has amodal pixels, a third of those no visible ones."""
    from constructionsceneposeestimation_amd.renderer import scene_labels
    L = scene_labels(wl.scene)
    rng = np.random.default_rng(seed)
    amo, vis = np.tile(np.array(EMPTY, np.uint32), (L, 1)), np.tile(np.array(EMPTY, np.uint32), (L, 1))
    for l in range(0, L, 2):
        x0, y0 = int(rng.integers(0, W - 40)), int(rng.integers(0, H - 40))
        amo[l] = (900, x0, y0, x0 + 29, y0 + 29)
        if l % 3:
            vis[l] = (400, x0 + 5, y0 + 5, x0 + 24, y0 + 24)
    return vis, amo


def test_pose_projects_the_box_centre(wl):
    """For every object with a box, over two epochs: R is a rotation, and K (R c_model + t) is the float64
    projection of the box centre through the schedule's own P V T_obj, to 1e-6 px (both float64)."""
    n = 0
    for f in (3, 14):
        V, P = wl.camera(f)[:2]
        frames = wl.epoch(f // 10).object_frames
        em = bop.epoch_models(frames)
        K = bop.cam_K(P)
        for j, o in enumerate(wl.scene.objects):
            box = object_box(o)
            if box is None:
                continue
            R, t = bop.object_pose(V, em, j)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
            c_local = (box[0] + box[1]) / 2.0
            c_model = c_local * em["scale"][j] * 1000.0
            q = (P @ V @ np.asarray(frames[j], np.float64).reshape(4, 4) @ np.append(c_local, 1.0))
            if abs(q[3]) < 1e-3:
                continue
            p = K @ (R @ c_model + t)
            # OpenCV's integer coordinates are pixel centres: the renderer's (u, v) reads (u - 1/2, v - 1/2)
            assert np.abs(p[:2] / p[2] - (q[:2] / q[3] - 0.5)).max() < 1e-6, (f, j)
            assert abs(p[2] / 1000.0 - q[3]) < 1e-9 * max(1.0, abs(q[3]))   # depth along the optical axis, mm -> m
            n += 1
    assert n >= 40
    rec = bop.camera_record(V, P, 250.0)
    Rw = np.array(rec["cam_R_w2c"]).reshape(3, 3)
    assert abs(np.linalg.det(Rw) - 1.0) < 1e-12 and rec["depth_scale"] == 4.0
    assert rec["cam_K"] == [wl.intr.fx, 0.0, wl.intr.cx - 0.5, 0.0, wl.intr.fy, wl.intr.cy - 0.5, 0.0, 0.0, 1.0]
    Cw = np.linalg.inv(V)[:3, 3]                                    # the camera's position maps to the origin
    assert np.abs(Rw @ Cw * 1000.0 + np.array(rec["cam_t_w2c"])).max() < 1e-6


def test_fragment_schema(wl):
    vis, amo = _stats(wl, 1)
    el = eligible_labels(wl.scene, DYNAMIC_KINDS)
    V, P = wl.camera(12)[:2]
    em = bop.epoch_models(wl.epoch(1).object_frames)
    listed = bop.listed_objects(wl.scene, el, amo)
    idx = [wl.scene.objects[j].inst_idx for j in listed]
    assert idx == sorted(idx) and len(idx) >= 2
    assert all(el[i] and amo[i][0] > 0 for i in idx)
    every = bop.listed_objects(wl.scene, None, amo)
    assert set(listed) < set(every)
    frag = bop.frame_fragment(1012, V, P, 250.0, wl.scene, em, vis, amo, listed)
    assert (frag["frame_id"], frag["scene_id"], frag["im_id"]) == (1012, 1, 12)
    assert sorted(frag["camera"]) == ["cam_K", "cam_R_w2c", "cam_t_w2c", "depth_scale"]
    assert len(frag["gt"]) == len(frag["gt_info"]) == len(listed)
    hidden = 0
    for g, i, l in zip(frag["gt"], frag["gt_info"], idx):
        assert sorted(g) == ["cam_R_m2c", "cam_t_m2c", "obj_id"] and g["obj_id"] == l + 1
        assert len(g["cam_R_m2c"]) == 9 and len(g["cam_t_m2c"]) == 3
        assert sorted(i) == ["bbox_obj", "bbox_visib", "px_count_all", "px_count_valid", "px_count_visib",
                             "visib_fract"]
        assert i["px_count_all"] == i["px_count_valid"] == 900 and i["bbox_obj"][2:] == [30, 30]
        if vis[l][0] == 0:          # inside the frame, wholly hidden
            assert i["bbox_visib"] == [-1, -1, -1, -1] and i["visib_fract"] == 0 and i["px_count_visib"] == 0
            hidden += 1
        else:
            assert i["bbox_visib"][2:] == [20, 20] and i["visib_fract"] == 400 / 900
    assert json.loads(bop.json_bytes(frag)) == frag
    models = bop.model_records(wl.scene, em)
    assert [m["obj_id"] for m in models] == sorted(m["obj_id"] for m in models)
    m = next(m for m in models if "model" in m)
    o = next(o for o in wl.scene.objects if o.inst_idx == m["inst_idx"])
    size = np.array([m["model"][k] for k in ("size_x", "size_y", "size_z")])
    box = object_box(o)
    j = wl.scene.objects.index(o)
    assert np.allclose(size, (box[1] - box[0]) * em["scale"][j] * 1000.0)
    assert m["model"]["diameter"] == pytest.approx(float(np.linalg.norm(size)))


def _write_run(wl, out_dir, frames):
    el = eligible_labels(wl.scene, DYNAMIC_KINDS)
    em0 = bop.epoch_models(wl.epoch(0).object_frames)
    bop.write_run_tables(out_dir, wl.scene, em0, wl.intr.pixel_projection(), W, H, 250.0)
    for f in frames:
        vis, amo = _stats(wl, f)
        V, P = wl.camera(f)[:2]
        em = bop.epoch_models(wl.epoch(f // 10).object_frames)
        bop.write_fragment(bop.fragment_path(out_dir, f), f, V, P, 250.0, wl.scene, em, vis, amo,
                           bop.listed_objects(wl.scene, el, amo))


def test_numbering_and_merge_of_shards(wl, tmp_path):
    """Frames 998 .. 1001 straddle the scene boundary; two shards merged give the files of one run."""
    frames = [998, 999, 1000, 1001]
    assert [bop.scene_image(f) for f in frames] == [(0, 998), (0, 999), (1, 0), (1, 1)]
    assert bop.image_path("D", "rgb", 1001) == os.path.join("D", "train_pbr", "000001", "rgb", "000001.png")
    assert bop.mask_path("D", "mask_visib", 999, 3) == os.path.join("D", "train_pbr", "000000", "mask_visib",
                                                                    "000999_000003.png")
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    _write_run(wl, one, frames)
    _write_run(wl, os.path.join(two, "shard_00"), frames[0::2])
    _write_run(wl, os.path.join(two, "shard_01"), frames[1::2])
    a, b = bop.merge(one), bop.merge(two)
    assert [os.path.relpath(p, one) for p in a] == [os.path.relpath(p, two) for p in b] and len(a) == 9
    for pa, pb in zip(a, b):
        assert open(pa, "rb").read() == open(pb, "rb").read(), pa
    for s, ims in ((0, ["998", "999"]), (1, ["0", "1"])):
        docs = [json.load(open(os.path.join(bop.scene_dir(one, s), n)))
                for n in ("scene_camera.json", "scene_gt.json", "scene_gt_info.json")]
        assert all(list(d) == ims for d in docs)
        assert all(len(docs[1][i]) == len(docs[2][i]) >= 1 for i in ims)
    cam = json.load(open(os.path.join(one, "camera.json")))
    assert (cam["width"], cam["height"], cam["depth_scale"]) == (W, H, 4.0) and cam["fx"] == wl.intr.fx
    objects = json.load(open(os.path.join(one, "models", "objects.json")))
    info = json.load(open(os.path.join(one, "models", "models_info.json")))
    assert set(info) <= set(objects) and all(objects[k]["inst_idx"] == int(k) - 1 for k in objects)
    assert sorted(objects["1"]) == ["class_id", "class_name", "inst_idx", "prim_path"]
    _write_run(wl, os.path.join(two, "shard_01"), [998])            # the same frame in two shards
    with pytest.raises(ValueError):
        bop.merge(two)
    assert bop.main(["merge"]) == 2


def test_parse_outputs():
    assert parse_outputs("bop") == ("bop",)
    assert parse_outputs("rgb,bop,depth16_png") == ("rgb", "bop", "depth16_png")
    for bad in ("bop,mask", "mask_rle,bop", "bop,mask_rle,amodal_rle"):
        with pytest.raises(ValueError):
            parse_outputs(bad)
    assert "bop" not in parse_outputs("all") and "bop" not in parse_outputs("reference")
    with pytest.raises(ValueError):
        bop.check_depth_scale(0.5, 0.9)
    bop.check_depth_scale(0.5, 250.0)
