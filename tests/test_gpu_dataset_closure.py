"""Labels against pixels on the files of real generator runs.  Two runs of frames 7 … 12 of C3,
seed 2, 480 x 272 with ``batch=4, writers=2, prep_workers=2`` (the default starts worker processes only from 20
batches on), so frames 9 and 10, of two epochs, share a batch that worker processes prepared: run A writes the
reference-shaped and the per-pixel outputs, run B the BOP layout (then ``bop merge``).  The reader of
tests/dataset_closure.py gets the two directories and nothing else; every check passes with the bounds the CPU
test uses and gives the figures the CPU oracle's arrays give, and mutants 1, 2, 4 and 6 fail on the files as they
do there.  A third case runs check H on what ``render_crops`` returns for the crops' test frames."""
import pytest

from tests import dataset_closure as dc
from tests.test_dataset_closure import (FRAMES, H, SEED, W, assert_box_records, assert_mutant_fails, crop_labels,
                                        oracle_dataset, report, run_checks)

pytestmark = pytest.mark.gpu

RUN_A = ("rgb", "mask", "depth_npy", "obj_coords", "pointcloud_ply", "mask_rle", "amodal_rle",
         "pointcloud_voxel_ply", "depth16_png")
RUN_B = ("bop", "obj_coords")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from constructionsceneposeestimation_amd import bop
    from constructionsceneposeestimation_amd.generate import generate
    d = tmp_path_factory.mktemp("closure")
    kw = dict(workload="C3", seed=SEED, batch=4, width=W, height=H, writers=2, prep_workers=2)
    for name, outs in (("a", RUN_A), ("b", RUN_B)):
        summary = generate(str(d / name), FRAMES, outputs=outs, **kw)
        assert summary["throughput"]["prep_workers"] == 2 and summary["throughput"]["writers"] == 2
    bop.merge(str(d / "b"))
    return str(d / "a"), str(d / "b")


@pytest.fixture(scope="module")
def read(runs):
    """The two directories as the reader's dicts: tables, and per frame (run A's dict, the BOP dict)."""
    a_dir, b_dir = runs
    objects, voxel = dc.load_run_tables(a_dir)
    return dict(objects=objects, voxel=voxel, boxes=dc.boxes_of(objects), rigid=dc.rigid_objects(objects),
                frames={f: (dc.load_frame(a_dir, f), dc.load_bop_frame(b_dir, f)) for f in FRAMES})


def test_every_check_passes_on_the_files(read):
    """... and every figure is the one the CPU oracle's arrays give (DESIGN.md §9 records one table for both)."""
    ds = oracle_dataset()
    for f in FRAMES:
        a, b = read["frames"][f]
        assert a["label"]["camera_pose"] == b["label"]["camera_pose"]       # the two runs drew the same frame
        res = run_checks(a, b, read["boxes"], read["rigid"], read["voxel"])
        report(f, res)
        for k, r in res.items():
            assert r.ok, (f, k, dict(r))
        B = res["B"]
        assert B["partition"] and B["unlisted"] == 0 and B["two_sided"] >= 0.85 * B["labelled"], (f, dict(B))
        assert res["E"]["worst_px_bound"] < 0.1 and res["E"]["pixels"] > 0 and res["D"]["vis2"] > 0
        assert_box_records(res["G"])
        cpu = run_checks(ds["a"][f], ds["b"][f], read["boxes"], read["rigid"], read["voxel"])
        for k, r in res.items():
            assert dict(r) == dict(cpu[k]), (f, k, dict(r), dict(cpu[k]))


@pytest.mark.parametrize("number", [1, 2, 4, 6])
def test_mutants_fail_on_the_files(read, number):
    assert_mutant_fails(number, *read["frames"][7], [read["frames"][f][0]["label"] for f in (10, 11, 12)],
                        read["boxes"], read["rigid"], read["voxel"])


def test_crops_and_point_samples_close_on_the_gpu():
    """render_crops on frames 4, 17, 23 of the crops' fixtures: check H on its arrays, ``intrinsics`` and ``info``."""
    from constructionsceneposeestimation_amd.labels import object_box
    from constructionsceneposeestimation_amd.renderer import Renderer
    from tests.test_crop_amodal import FIDS3, H3, K3, MINPX3, PAD3, S3, W3, c3_reference
    ref = c3_reference(None)
    wl = ref["wl"]
    with Renderer(wl.scene, W3, H3, max_frames=2) as r:
        for k, e in enumerate(ref["epochs"]):
            r.set_instance_transforms(k, wl.epoch(e).models)
            r.set_object_frames(k, wl.epoch(e).object_frames)
        got = r.render_crops(ref["fr"], size=S3, per_frame=K3, min_pixels=MINPX3, pad=PAD3, samples=256,
                             want=("mask", "coords", "depth", "amodal", "amodal_depth", "amodal_coords", "points"))
    objs = [{"inst_idx": int(o.inst_idx), "class_name": o.class_name,
             "lo": object_box(o)[0].tolist() if object_box(o) else None,
             "hi": object_box(o)[1].tolist() if object_box(o) else None} for o in wl.scene.objects]
    kw = dict(labels=crop_labels(wl, FIDS3), boxes=dc.boxes_of(objs), info=got["info"], S=S3,
              intrinsics=got["intrinsics"], arrays=got)
    res = dc.check_crops(**kw)
    report("4,17,23", {"H": res})
    assert res.ok, dict(res)
    assert res["hidden"] >= 500 and res["samples"] >= 10000 and res["points"] >= 256 * 15
    assert dc.check_crops(other_slot=True, **kw)["failures"] > 0
