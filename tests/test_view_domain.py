"""The cases of tests/view_domain.py really occur (no GPU): each assertion is
made on the CPU oracle's output alone, so that bit-exact parity of the kernels
(tests/test_gpu_view_domain.py asserts these again, then compares) cannot be
vacuous -- the clip ranges cut the quad on both sides, every projection changes
the picture and its world points fall back onto their pixels, the odd views see
what they are named after, the mirrored cone is visible and the flattened one is
not, and every frustum sweep goes from nothing to something."""
import numpy as np
import pytest

from tests import view_domain as vd


def check_clip(case, others):
    """``others``: the oracle outputs of the other clip ranges (frame 0's keypoints must differ)."""
    n = vd.clip_preconditions(case)
    print(case["name"], n)
    assert n["outside"] == 0 and 0 < n["kept"] < n["whole"], n       # a strict, non-empty subset
    assert n["lost_far"] >= 50 and n["lost_near"] >= 50, n
    assert n["visible"] >= 50, n
    ora = vd.oracle_case(case)
    assert ora[0]["stats"]["n_clipped"] >= 1
    w = [0.02, 0.04, 0.1, 0.3, 0.6, 1.0, 2.0, 2.9, 3.5, 5.0, 7.0, 9.0, 50.0, 300.0, 2.0e4]
    vis = ora[0]["project_vis"][:len(w)]
    assert [bool(v) for v in vis] == [x >= case["near"] for x in w], vis.tolist()   # the far plane does not hide them
    assert sorted(set(ora[0]["keypoints_vis"].tolist())) == [0, 1, 2]
    for o in others:
        assert not np.array_equal(o[0]["keypoints_vis"], ora[0]["keypoints_vis"])
        assert not np.array_equal(o[0]["instance"], ora[0]["instance"])
    lo, hi = ora[0]["depth_range"]
    assert case["near"] * 0.999 <= lo < hi <= case["far"] * 1.001


def check_intrinsics(case):
    ora = vd.oracle_case(case)
    plain = vd._case("plain", case["scene"], case["V"], [vd.default_pinhole()] * 5)
    base = vd.oracle_case(plain)
    for f, out in enumerate(ora):
        hit = np.isfinite(out["depth"])
        px, w = vd.reprojection_error(case, f, out)
        print(f"intrinsics {f}: {int(hit.sum())} pixels hit, {len(np.unique(out['instance']))} ids, reprojection "
              f"{px:.2e} px, W / depth - 1 {w:.2e}")
        assert hit.sum() >= 2000 and len(np.unique(out["instance"])) >= 3, f
        assert not np.array_equal(out["instance"], base[f]["instance"]), f
        assert px <= 0.02 and w <= 1e-4, (f, px, w)                 # points were made with this frame's fx, fy, cx, cy
        inside = ((out["obj_coords"] > 0) & (out["obj_coords"] < 65535)).all(-1)[out["instance"] >= 0]
        assert inside.size >= 500 and inside.mean() >= 0.9, f
        assert (out["keypoints_vis"] > 0).sum() >= 2, f
    assert len({tuple(np.round(o["keypoints_uv"], 3).reshape(-1).tolist()) for o in ora}) == 5


def check_odd_views(case):
    ora = vd.oracle_case(case)
    level = ora[-1]                                                 # the same pose without roll
    for f, roll in enumerate(vd.ROLLS):
        assert len(np.unique(ora[f]["instance"])) >= 5 and not np.array_equal(ora[f]["instance"], level["instance"])
    # rolled by 180 degrees the picture is the level one turned upside down, up to pixels on silhouettes
    same = (ora[2]["instance"] == level["instance"][::-1, ::-1]).mean()
    print("odd views: rolled 180 degrees agrees with the turned level picture on", round(float(same), 4))
    assert same >= 0.9
    down, up, cut = ora[3], ora[4], ora[5]
    assert np.isfinite(down["depth"]).all() and len(np.unique(down["instance"])) >= 4   # the ground fills the view
    assert abs(float(np.median(down["depth"])) - 9.0) < 0.5
    hit = np.isfinite(up["depth"])
    assert 0.1 <= hit.mean() <= 0.95 and set(np.unique(up["instance"][hit]).tolist()) == {25}, hit.mean()
    assert cut["stats"]["n_clipped"] >= 50, cut["stats"]                # the near plane cuts many triangles of the panel
    assert (cut["instance"] == 1).sum() >= 500 and float(cut["depth"][cut["instance"] == 1].min()) < 0.51


def check_inside(case):
    ora = vd.oracle_case(case)
    for f, out in enumerate(ora):
        hit = np.isfinite(out["depth"])
        print(f"inside the cone {f}: {hit.mean():.3f} of the frame hit")
        assert hit.mean() >= 0.95 and (out["instance"][hit] == 0).all(), f
        assert (out["normals"][hit].astype(np.float32) != 0).any(-1).all(), f


def check_models(case):
    ora = vd.oracle_case(case)
    kinds = case["kinds"]
    for s in (0, 1):
        M = case["models"][s].reshape(5, 4, 4)
        dets = [float(np.linalg.det(M[k][:3, :3])) for k in range(5)]
        assert dets[kinds[s].index("mirrored")] < 0 and dets[kinds[s].index("flattened")] == 0.0
        assert all(d > 0 for k, d in enumerate(dets) if kinds[s][k] not in ("mirrored", "flattened"))
    for f, out in enumerate(ora):
        s = case["sets"][f]
        px = out["inst_stats"][:, 0]
        print(f"model matrices frame {f} (set {s}): pixels per cone {px.tolist()}")
        hit = np.isfinite(out["depth"])
        assert (out["normals"][hit].astype(np.float32) != 0).any(-1).all(), f
        for k in range(5):
            if kinds[s][k] == "flattened":
                assert px[k] == 0 and out["label_covered"][k] == 0, (f, k)   # every triangle is flat: nothing is drawn
            else:
                assert px[k] >= 20, (f, k, kinds[s][k])
    # the cone that is flattened in set 0 is drawn in set 2, from a like distance
    assert ora[2]["inst_stats"][kinds[0].index("flattened"), 0] >= 100


def check_sweeps(case):
    ora = vd.oracle_case(case)
    for p, plane in enumerate(vd.PLANES):
        px = [int((ora[p * vd.STEPS + k]["instance"] == 0).sum()) for k in range(vd.STEPS)]
        print(f"sweep {plane}: pixels {px}")
        assert px[0] == 0 and px[-1] > 0, (plane, px)
        if plane in ("near", "far"):
            assert all(v == 0 for v in px[:8]), (plane, px)         # W outside the plane by 1 ulp or more
        else:
            assert px == sorted(px), (plane, px)


def test_clip_ranges(world2):
    cases = [vd.clip_case(world2, *r) for r in vd.CLIP_RANGES]
    outs = [vd.oracle_case(c) for c in cases]
    for k, c in enumerate(cases):
        check_clip(c, outs[:k] + outs[k + 1:])


def test_intrinsics(world2):
    check_intrinsics(vd.intrinsics_case(world2))


def test_odd_views(world2, cone):
    check_odd_views(vd.odd_views_case(world2))
    check_inside(vd.inside_case(cone))


def test_model_matrices(cone):
    check_models(vd.models_case(cone))


def test_frustum_sweeps():
    case = vd.sweep_case()
    assert case["V"].shape[0] == 96 and len(case["scene"].meshes[0].tris) >= 1024
    check_sweeps(case)
