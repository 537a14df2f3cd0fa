"""The CPU oracle against the posed exact frames of tests/pose_exact.py (no GPU): the model, view and
projection chain.  ``pose_exact`` holds for every triangle of every frame under every pose, the oracle
equals the carried reference on every decided pixel (ids, depth bits, rgb, normals, points, label
statistics, coverage, keypoints), ``restate_obj_coords`` on its points equals the rounded chain of §12,
and the expected object coordinates lie within the derived bound of the exact surface.
tests/test_gpu_pose_exact.py runs the same frames through the kernels.

Mutants.  Each of these changes to oracle/csg_oracle.c (applied one at a time to a scratch copy) fails
``test_oracle_matches_the_posed_reference``; DESIGN.md §9 has the table of poses and outputs that catch
each: ``R_cw`` transposed in the camera constants; ``c`` taken as V's translation column; the normal from
object-space positions; the sun direction used as if in camera space; keypoints through ``P (V M)`` of
instance 0; ``M p`` with M transposed.  ``(P V) M`` for ``P (V M)`` is the same function on these exact
matrices and is not caught.
"""
import hashlib

import numpy as np
import pytest

from tests import pose_exact as px
from tests import shade_exact as sx
from tests.test_obj_coords import restate_obj_coords

SIZES = [pytest.param(s, id=f"{s[0]}x{s[1]}") for s in sx.SIZES]
IDENTITY_DIGEST = {(96, 64): "b9daf958d0cb2fc7394a7240044f15522afc7306762a878cb4679a44121f065f",
                   (67, 35): "4feb36fcc3888dec7cd733ec07f6d0badf10355db9602e561f1f88498d43c7ba"}
DIGEST_KEYS = ("ids", "depth", "rgb", "normals", "points", "undecided", "masks", "und_label", "inst_stats", "amodal_stats",
               "covered", "uid", "bestZ", "kp", "kp_uv", "kp_vis")


def test_pieces_by_hand():
    f = np.float32
    q = px.Q((1, 0, 2), (1, -1, 1))
    assert q.tolist() == [[0, 1, 0], [-1, 0, 0], [0, 0, 1]] and np.linalg.det(q) == 1.0
    V = px.affine(q, (2, -1, 0.5))
    Vi = px.inv_affine(V)                                           # [Q^T | -Q^T t]
    assert Vi[:3, :3].tolist() == q.T.tolist() and Vi[:3, 3].tolist() == [-1.0, -2.0, -0.5]
    assert [p["proper"] for p in px.POSES.values()] == [True] * 7 + [False]
    assert np.linalg.det(px.POSES["B2"]["M"][:3, :3]) < 0           # the mirrored model
    # a signed permutation on f16 bits: -0 never appears, a sign flips
    n = np.array([[0x3C00, 0x0000, 0xB800]], np.uint16)             # (1, 0, -1/2)
    assert px.rotate_normals(n, q.T).tolist() == [[0x0000, 0x3C00, 0xB800]]          # Q^T n = (-0 -> 0, 1, -1/2)
    assert px.rotate_normals(n, q).tolist() == [[0x0000, 0xBC00, 0xB800]]
    assert px.rotate_normals(n, q, negate=True).tolist() == [[0x0000, 0x3C00, 0x3800]]
    # one rounding: 3 + 3 2^-23 lies halfway between 3 + 2^-22 and 3 + 2^-21 and goes to the even one
    p = np.array([[f(1.0) + f(3 * 2.0 ** -23), np.nan, 3.0]], f)
    got = px.move_points(p, px.affine(np.eye(3), (2, 0, 0)))
    assert got[0, 0] == f(3.0) + f(2.0 ** -21) and np.isnan(got[0, 1]) and got[0, 2] == 3.0
    assert px.move_points_fr(p[:, [0, 2, 2]], px.affine(np.eye(3), (2, 0, 0)))[0][0] == float(got[0, 0])
    # §12: (int)(c 65535 + 1/2), clamps and zero rows
    t = np.zeros((2, 3, 4), f)
    t[0] = [[0.5, 0, 0, 0.25], [0, 1, 0, 0], [0, 0, 1, 0]]
    u, _ = px.obj_chain(np.array([[0, 1, -1]]), np.array([[[1.0, -3.0, 7.0]] * 3], f), t)
    assert u.tolist() == [[[49151, 0, 65535], [0, 0, 0], [0, 0, 0]]]
    assert px.obj_chain_fr(0, [1.0, -3.0, 7.0], t) == [49151, 0, 65535]
    assert np.array_equal(u, restate_obj_coords(np.array([[0, 1, -1]]), np.array([[[1.0, -3.0, 7.0]] * 3], f), t))


@pytest.mark.parametrize("size", SIZES)
def test_the_identity_batch_is_unchanged(size):
    """tests/shade_exact.py changed by addition only: its frames are, byte for byte, what they were, and
    the generalised ``keypoints`` with P V = P gives the identity frames' keypoints."""
    b = sx.batch(*size)
    h = hashlib.sha256()
    for fr in b["frames"]:
        for k in DIGEST_KEYS:
            h.update(np.ascontiguousarray(fr[k]).tobytes())
    h.update(np.ascontiguousarray(b["models"]).tobytes())
    h.update(b["V"].tobytes())
    h.update(b["P"].tobytes())
    for m in b["scene"].meshes:
        h.update(np.ascontiguousarray(m.positions).tobytes())
    assert h.hexdigest() == IDENTITY_DIGEST[size]
    W, H = size
    PV = px.mat4_mul32(b["P"][0], b["V"][0])
    for fr in b["frames"]:
        uv, vis = sx.keypoints(fr["kp"], fr["depth"], W, H, W // 2, H // 2, PV)
        assert uv.tobytes() == fr["kp_uv"].tobytes() and vis.tobytes() == fr["kp_vis"].tobytes()


@pytest.mark.parametrize("size", SIZES)
def test_pose_exact_holds_everywhere(size):
    W, H = size
    pb = px.batch(W, H)
    assert len(pb["frames"]) == len(px.NAMES) * pb["n_base"] == 8 * 48
    counts = {}
    for k, pf in enumerate(pb["frames"]):
        counts[pf["pose"]] = counts.get(pf["pose"], 0) + px.pose_exact(pb, k)[0]
    print(f"{W}x{H}: triangles that pass pose_exact per pose {counts}")
    assert counts == {name: 756 for name in px.NAMES}
    # the posed frames add no undecided pixel: the masks are the identity frames' own
    und = cov = 0
    for k, pf in enumerate(pb["frames"]):
        fr = pb["base"]["frames"][k % pb["n_base"]]
        assert pf["fr"] is fr and pf["base"] == k % pb["n_base"] and px.expected(pf)["undecided"] is fr["undecided"]
        if k < pb["n_base"]:
            und, cov = und + int(fr["undecided"].sum()), cov + int((fr["masks"].any(0) | fr["undecided"]).sum())
    assert und <= 0.00054 * cov, (und, cov)
    # the blocks: carried worlds draw the identity meshes, every pre-imaged pose has meshes of its own
    assert [pb["block_of"][n] for n in px.NAMES] == [0, 0, 0, 1, 2, 3, 4, 0]
    for k in (px.frame_index(pb, "B1", 0), px.frame_index(pb, "A3", 5)):
        pf = pb["frames"][k]
        m = pb["models"][k].reshape(-1, 4, 4)
        own = np.zeros(len(m), bool)
        own[pf["first"]:pf["first"] + pf["count"]] = True
        assert not m[~own].any() and (m[own] == pb["poses"][pf["pose"]]["M"].astype(np.float32)).all()


@pytest.mark.parametrize("size", SIZES)
def test_conditions_of_the_posed_reference(size):
    W, H = size
    pb = px.batch(W, H)
    rng = np.random.default_rng(W)
    for name in px.NAMES:
        pose = pb["poses"][name]
        fs = [pf for pf in pb["frames"] if pf["pose"] == name]
        kv = np.concatenate([pf["kp_vis"] for pf in fs])
        assert (kv == 1).sum() >= 10 and (kv == 2).sum() >= 10 and (kv == 0).sum() >= 10, name
        same = [pf["kp_uv"].tobytes() == pf["fr"]["kp_uv"].tobytes() and pf["kp_vis"].tobytes() == pf["fr"]["kp_vis"].tobytes()
                for pf in fs]
        exact = [pf["kp_exact"] for pf in fs]
        print(f"{W}x{H} {name}: keypoints carried exactly in {sum(exact)} frames, uv and vis the identity frame's in {sum(same)}")
        if all(exact):                                              # a pose whose carried keypoints are float32s
            assert all(same), name
        assert all(exact) == (name in ("P", "improper")), name
        # the world really differs: points and (off class P) normals are not the identity frame's
        moved = sum(not np.array_equal(pf["points"], pf["fr"]["points"], equal_nan=True) for pf in fs)
        turned = sum(not np.array_equal(pf["normals"], pf["fr"]["normals"]) for pf in fs)
        # (A1 turns about z: frames of flat triangles keep their normals)
        assert moved == len(fs) and (turned >= len(fs) // 2 or name == "P"), (name, moved, turned)
        assert all(pf["shaded"].all() for pf in fs) == (name != "P")
        if name == "P":                                             # flat triangles win a good part of the stretched world
            share = (sum(int((pf["shaded"] & (pf["fr"]["ids"] >= 0)).sum()) for pf in fs)
                     / sum(int((pf["fr"]["ids"] >= 0).sum()) for pf in fs))
            print(f"{W}x{H} P: rgb and normals compared on {100 * share:.1f}% of the drawn pixels")
            assert share >= 0.3
        # the boxes: label 0 wholly inside, label 1 clamped at both ends, label 5 without rows
        table, boxes = fs[0]["obj_table"], fs[0]["boxes"]
        assert boxes[5] is None and not table[5].any() and all(boxes[l] is not None for l in range(5))
        for l in range(5):
            e = boxes[l][1] - boxes[l][0]
            assert (np.log2(e) == np.rint(np.log2(e))).all() and (boxes[l][0] * 2.0 ** 12 == np.rint(boxes[l][0] * 2.0 ** 12)).all()
        of = lambda key, l: np.concatenate([pf[key][(pf["fr"]["ids"] == l) & ~pf["fr"]["undecided"]] for pf in fs])    # noqa: E731
        at, u_of = (lambda l: of("obj_q", l)), (lambda l: of("obj_coords", l))
        assert len(at(0)) >= 1000 and (at(0) >= 0).all() and (at(0) <= 1).all(), name
        q1, u1 = at(1), u_of(1)
        assert (q1 < 0).any(0).all() and (q1 > 1).any(0).all() and (u1 == 0).sum() >= 50 and (u1 == 65535).sum() >= 50, name
        assert ((u1 > 0) & (u1 < 65535)).sum() >= 50 and len(u_of(5)) >= 50 and not u_of(5).any(), name
        # the rounded chains against rationals on a sample of pixels, and the bound against the exact surface
        worst = 0.0
        n_free = 0
        for pf in fs:
            fr = pf["fr"]
            ys, xs = np.nonzero(fr["ids"] >= 0)
            pick = rng.choice(ys.size, min(4, ys.size), replace=False)
            C = px.carry(pose)
            for y, x in zip(ys[pick], xs[pick]):
                assert px.move_points_fr(fr["points"][y:y + 1, x], C)[0] == pf["points"][y, x].astype(np.float64).tolist()
                assert px.obj_chain_fr(int(fr["ids"][y, x]), pf["points"][y, x], table) == pf["obj_coords"][y, x].tolist()
            t, E, free = px.surface_bound(pf, pb)
            off = np.abs(pf["obj_coords"].astype(np.float64) - 65535.0 * t)
            assert (off[free] <= 0.5 + 65535.0 * E[free]).all(), (name, fr["family"])
            if free.any():
                worst = max(worst, float((off[free] - 0.5).max()))
                n_free += int(free.sum())
        print(f"{W}x{H} {name}: {n_free} unclamped components within 1/2 + 65535 E of the exact surface, "
              f"worst |u - 65535 t| - 1/2 = {worst:.4f}")
        assert n_free >= 10000


@pytest.mark.parametrize("size", SIZES)
def test_oracle_matches_the_posed_reference(size):
    W, H = size
    pb, ora = px.batch(W, H), px.oracle_frames(W, H)
    bad = []
    for pf, o in zip(pb["frames"], ora):
        what = f'{W}x{H} {pf["pose"]} {pf["fr"]["family"]}/{pf["fr"]["order"]}'
        bad += px.compare(pf, o, what)
        bad += px.compare_keypoints(pf, o["keypoints_uv"], o["keypoints_vis"], what, W, H)
        ok = ~pf["fr"]["undecided"]
        if not np.array_equal(restate_obj_coords(o["instance"], o["points"], pf["obj_table"])[ok], pf["obj_coords"][ok]):
            bad.append(f"{what}: restate_obj_coords on the oracle's points is not the chain of §12")
        if pf["pose"] == "improper":                                # the finding: the normals face away from the camera
            drawn = ok & (pf["fr"]["ids"] >= 0)
            assert not np.array_equal(o["normals"].view(np.uint16)[drawn], pf["normals_proper"][drawn]), what
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("size", SIZES)
def test_amodal_geometry_of_one_label_alone(size):
    """The reference of §13.3: a label drawn alone has the frame's exact amodal mask, and where it wins
    the frame its depth and coordinates are the frame's."""
    W, H = size
    pb = px.batch(W, H)
    n = 0
    for name in ("A2", "B1", "B3"):
        for f, fr in enumerate(pb["base"]["frames"]):
            if fr["family"] not in ("clip", "clip_edge", "cross", "tie"):
                continue
            k = px.frame_index(pb, name, f)
            pf = pb["frames"][k]
            for l in range(sx.N_LABELS):
                a = px.amodal_geometry(pb, k, l)
                assert np.array_equal(a["mask"] | a["undecided"], fr["masks"][l] | a["undecided"])
                won = (fr["ids"] == l) & ~a["undecided"] & ~fr["undecided"]
                assert np.array_equal(a["depth"].view(np.uint32)[won], fr["depth"].view(np.uint32)[won])
                assert np.array_equal(a["coords"][won], pf["obj_coords"][won])
                hidden = a["mask"] & (fr["ids"] != l) & ~a["undecided"]
                assert (a["depth"][hidden] >= fr["depth"][hidden]).all()
                n += int(hidden.sum())
    assert n >= 500                                                 # some of it is hidden behind another label
