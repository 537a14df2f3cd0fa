"""The CPU oracle against the exact depth / alpha / texture / shading reference of
tests/shade_exact.py (no GPU): every output on every decided pixel of every
frame, the undecided share, and that each family really holds the cases it is
named after.  tests/test_gpu_shade_exact.py runs the same frames through the
kernels.

Mutants.  Each of these changes to oracle/csg_oracle.c (applied one at a time
to a scratch copy) fails ``test_oracle_matches_the_exact_reference``; DESIGN.md
§9 has the table of families that catch each: drop ``1 - v``; drop the texel
centre's ``- 0.5``; ``(int)`` for ``floorf``; ``>=`` for ``>`` in the alpha test;
drop ``+ 32768``; affine uv; ties to the larger uid; ``<`` for ``<=`` at 1/far;
the normal's sign inverted; drop ``+ 127``; drop ``+ 0.5`` in q; and, beyond that
list, a depth key without its low 5 bits (caught by cross_near alone).
"""
from fractions import Fraction as Fr

import numpy as np
import pytest

from tests import shade_exact as sx

SIZES = [pytest.param(s, id=f"{s[0]}x{s[1]}") for s in sx.SIZES]


def test_reference_by_hand():
    """The reference's own pieces on cases small enough to decide by hand."""
    f = np.float32
    # rn32: ties to even, and the keypoint division
    assert sx.rn32(Fr(1) + Fr(1, 1 << 24)) == 1 and sx.rn32(Fr(1) + Fr(3, 1 << 24)) == Fr(1) + Fr(1, 1 << 22)
    assert sx.rn32(Fr(1, 3)) == Fr(float(f(1.0) / f(3.0))) and sx.rn32(Fr(-7, 5)) == Fr(float(f(-1.4)))
    # rn32_recip against float32 division (correctly rounded in NumPy)
    Z = np.array([1 << 40, 3 << 33, (1 << 41) - 1, (1 << 34) + 1, 12345678901], np.int64)
    want = (np.float64(2.0 ** sx.ZS) / Z.astype(np.float64))
    assert np.array_equal(sx.rn32_recip(Z), np.array([f(Fr(1 << sx.ZS, int(z))) for z in Z]))
    assert np.allclose(sx.rn32_recip(Z), want, rtol=1e-7)
    # a 2 x 2 texture: texel centres, a boundary, the wrap, floor on negative coordinates
    tex = np.zeros((2, 2, 4), np.uint8)
    tex[0, 0], tex[0, 1], tex[1, 0], tex[1, 1] = (10, 0, 0, 0), (20, 0, 0, 100), (30, 0, 0, 200), (40, 0, 0, 255)
    s = lambda u, v: sx.sample(tex, np.array([u], f), np.array([v], f))      # noqa: E731
    assert s(0.25, 0.75)[0][0].tolist() == [10, 0, 0, 0]                     # the centre of texel (0, 0): v = 1 is the top
    assert s(0.75, 0.25)[0][0].tolist() == [40, 0, 0, 255]
    assert s(0.5, 0.75)[0][0, 0] == 15 and s(0.5, 0.75)[3]["edge_x"][0]      # halfway between (0, 0) and (1, 0)
    assert s(0.0, 0.75)[0][0, 0] == 15 and s(0.0, 0.75)[3]["neg_x"][0]       # t = -1/2: floor -1 wraps to texel 1, weight 128
    assert s(-0.25, 0.75)[0][0, 0] == 20 and s(-0.75, 0.75)[0][0, 0] == 10   # (trunc would read texel 0 at -0.25)
    assert s(3.25, -1.25)[0][0].tolist() == [10, 0, 0, 0]                    # repeats away
    assert not s(0.25, 0.75)[1][0] and s(0.25, 0.75)[2][0]                   # decided, and exact in float32
    # (top (256 - wy) + bot wy + 32768) >> 16 rounds to nearest: weights 128, 128 of 10, 20, 30, 40 -> 25
    assert s(0.5, 0.5)[0][0, 0] == 25
    # a weight of 1/256: 10 (255/256) + 20 (1/256) = 10.04 -> 10;  without + 32768 it would still be 10, so also 19.96 -> 20
    assert s(0.25 + 1 / 512, 0.75)[0][0, 0] == 10 and s(0.75 - 1 / 512, 0.75)[0][0, 0] == 20


def _frames(size):
    W, H = size
    return W, H, sx.batch(W, H), sx.oracle_frames(W, H)


@pytest.mark.parametrize("size", SIZES)
def test_oracle_matches_the_exact_reference(size):
    W, H, b, ora = _frames(size)
    bad = []
    for fr, o in zip(b["frames"], ora):
        what = f'{W}x{H} {fr["family"]}/{fr["order"]}'
        bad += sx.compare(fr, o, what)
        for k in range(sx.N_KP):
            u, v = fr["kp_uv"][k]
            inside = 0 <= u < W and 0 <= v < H
            if inside and fr["undecided"][int(v), int(u)]:
                continue
            if not (np.array_equal(o["keypoints_uv"][k], fr["kp_uv"][k]) and o["keypoints_vis"][k] == fr["kp_vis"][k]):
                bad.append(f'{what}: keypoint {k}: uv {o["keypoints_uv"][k].tolist()} vis {o["keypoints_vis"][k]}, expected '
                           f'{fr["kp_uv"][k].tolist()} {fr["kp_vis"][k]}')
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("size", SIZES)
def test_conditions_of_the_reference(size):
    W, H, b, _ = _frames(size)
    fam = {}
    names = [f["family"] for f in b["frames"]]
    assert all(any(n.startswith(f) for n in names) for f in sx.FAMILIES)
    und_total = frag_total = 0
    for k, fr in enumerate(b["frames"]):
        what = f'{W}x{H} {fr["family"]}/{fr["order"]}'
        a = fr["aims"]
        drawn = int((fr["ids"] >= 0).sum())
        und = int(fr["undecided"].sum())
        covered = int((fr["masks"].any(0) | fr["undecided"]).sum())
        und_total, frag_total = und_total + und, frag_total + covered
        print(f'{what}: drawn {drawn} of {W * H}, fragments {a["frags"]}, undecided pixels {und}, ties {a["ties"]}')
        assert 0.15 <= drawn / (W * H) <= 0.98, what                # some of everything, and some sky
        assert und <= 0.01 * covered, what                         # the undecided condition
        if fr["family"] in ("texel", "thresh"):                    # flat, power-of-two textures: float32 texel_coords is exact
            assert und == 0 and a["inexact_chain"] == 0 and a["textured"] > 1000, what
        if fr["order"]:                                            # the other vertex order: the same images
            prev = b["frames"][k - 1]
            for key in ("ids", "rgb", "normals", "masks", "undecided"):
                assert np.array_equal(fr[key], prev[key]), (what, key)
            assert np.array_equal(fr["depth"].view(np.uint32), prev["depth"].view(np.uint32))
            assert all(sx.area2(t["xy"]) == -sx.area2(p["xy"]) for (_, _, ts), (_, _, ps) in zip(fr["insts"], prev["insts"])
                       for t, p in zip(ts, ps))
        # the normal's sign: facing the camera is "flipped iff det > 0", in both orders, and both occur
        flips = [d["shade"]["flipped"] for d in fr["drawn"]]
        assert all(d["shade"]["flipped"] == d["shade"]["det_positive"] for d in fr["drawn"]), what
        assert fr["order"] == 0 or (any(flips) or any(d["shade"]["flipped"] for d in b["frames"][k - 1]["drawn"])), what
        fam.setdefault(fr["family"], fr)
    print(f"{W}x{H}: {und_total} undecided of {frag_total} covered pixels ({100.0 * und_total / frag_total:.3f}%), "
          f'{b["rejected"]} generated triangles rejected')
    both = [d["shade"]["flipped"] for fr in b["frames"] for d in fr["drawn"] if d["n_won"]]
    assert any(both) and not all(both)

    a = fam["texel"]["aims"]
    assert a["centre"] >= 100 and a["edge_x"] >= 100 and a["edge_y"] >= 100           # centres and boundaries, exactly
    assert a["seam_x"] >= 100 and a["seam_y"] >= 100 and a["neg_x"] >= 100 and a["neg_y"] >= 100
    assert a["far_x"] >= 100 and a["far_y"] >= 100 and a["alpha_killed"] >= 100
    sizes = {fam["texel"]["insts"][i][1] for i in range(len(fam["texel"]["insts"]))}
    tex = {b["scene"].textures[b["scene"].materials[m].texture].rgba.shape[:2] for m in sizes}
    assert tex == {(8, 16), (4, 4), (1, 1)}
    rates = set()                                                  # texels per pixel along u, from the vertices
    for _, m, tris in fam["texel"]["insts"]:
        tw = b["scene"].textures[b["scene"].materials[m].texture].rgba.shape[1]
        for t in tris:
            A = np.array([[x, y, 1.0] for x, y in t["xy"]])
            gu = np.linalg.solve(A, np.array([u for u, _ in t["uv"]], np.float64))
            rates.add(round(float(np.hypot(gu[0], gu[1])) * tw, 6))
    assert {0.125, 1.0, 4.0} <= rates, rates                      # 8 px per texel, one to one, 4 texels per px
    n = fam["texel_npot"]["aims"]
    assert n["textured"] >= 500 and n["seam_x"] >= 50 and n["neg_x"] >= 50 and n["far_x"] >= 50
    a = fam["thresh"]["aims"]
    assert a["alpha_eq_thr"] >= 200 and a["alpha_thr1"] >= 200 and a["alpha_killed"] >= 500
    thr = {}
    for _, m, _ in fam["thresh"]["insts"]:
        mt = b["scene"].materials[m]
        thr.setdefault(mt.texture, set()).add(mt.alpha_threshold)
    assert all(len(v) == 2 for v in thr.values()) and {0, 127, 254} <= set().union(*thr.values())
    for want in (0, 127, 254):                                     # per threshold: exactly thr (dropped), thr + 1 (kept)
        ms = [m for _, m, _ in fam["thresh"]["insts"] if b["scene"].materials[m].alpha_threshold == want]
        eq, plus = sum(a["thr_eq"].get(m, 0) for m in ms), sum(a["thr_plus1"].get(m, 0) for m in ms)
        print(f"{W}x{H} thresh {want}: {eq} fragments at thr, {plus} at thr + 1")
        assert eq >= 50 and plus >= 50, (want, eq, plus)
    a = fam["persp"]["aims"]
    assert a["w_ratio"] == 32.0 and a["affine_differs"] >= 0.25 * a["textured"] and a["textured"] >= 2000
    a = fam["cross"]["aims"]
    assert a["min_rel_gap"] is not None and a["min_rel_gap"] < 2.0 ** -9
    ids = fam["cross"]["ids"]
    assert len(np.unique(ids[ids >= 0])) >= 5
    a = fam["cross_near"]["aims"]                                  # two surfaces a few float32 ulps of 1 / W apart
    print(f'{W}x{H} cross_near: smallest gap {a["min_ulp_gap"]} ulps, {a["near_front"]} / {a["near_behind"]} fragments '
          f'within {64 * sx.NEAR_ULPS} ulps in front of / behind the other')
    assert a["min_ulp_gap"] is not None and a["min_ulp_gap"] <= sx.NEAR_ULPS
    assert a["near_front"] >= 50 and a["near_behind"] >= 50       # the id flips along the line
    a = fam["tie"]["aims"]
    assert a["ties"] >= 500 and a["alpha_killed"] >= 20
    a = fam["range"]["aims"]
    assert a["z_far_exact"] >= 1 and a["z_near_exact"] >= 1 and a["out_far"] >= 200
    # a dropped centre within FAR_ULPS float32 ulps (2^-32 each) below 2^-8
    assert a["z_far_gap"] is not None and a["z_far_gap"] <= sx.FAR_ULPS << (sx.ZS - 32)
    r = fam["range"]
    assert (r["beyond"].any(0) & ~r["masks"].any(0)).sum() >= 100                # the far side is in no mask
    assert (r["covered"] < (r["masks"] | r["beyond"]).reshape(sx.N_LABELS, -1).sum(1)).any()
    lights = {fr["light"] for fr in b["frames"]}
    assert lights == set(range(len(b["lights"])))
    assert fam["light3"]["aims"]["q_clamped"] >= 50 and fam["light0"]["aims"]["textured"] >= 100
    flat = [d["shade"]["flat"] for n_, fr in fam.items() if n_.startswith("light") for d in fr["drawn"]]
    assert any(flat) and not all(flat)
    a = fam["trim"]["aims"]
    assert a["alpha_killed"] >= 0.8 * a["alpha_tested"] > 1000 and a["alpha_killed"] < a["alpha_tested"]
    kv = np.concatenate([fr["kp_vis"] for fr in b["frames"]])
    assert (kv == 0).sum() >= 10 and (kv == 1).sum() >= 10 and (kv == 2).sum() >= 10


@pytest.mark.parametrize("size", SIZES)
def test_ties_and_alpha_decide_the_winner(size):
    """The tie family by construction: the duplicate of smaller uid wins where it passes its alpha test."""
    W, H, b, _ = _frames(size)
    for fr in b["frames"]:
        if fr["family"] != "tie":
            continue
        first = fr["first"]
        win = fr["uid"] >> 20
        # (a): instances 0 and 1 hold the same triangles: 1 is never seen
        assert (win == first).sum() > 100 and (win == first + 1).sum() == 0
        # (b): triangle 1 of instance 2 repeats triangle 0
        assert ((fr["uid"] >> 20 == first + 2) & (fr["uid"] & 0xFFFFF == 0)).sum() > 50
        assert ((fr["uid"] >> 20 == first + 2) & (fr["uid"] & 0xFFFFF == 1)).sum() == 0
        # (c): instances 3 and 4 share a plane: on their common pixels 4 is never seen, elsewhere it is
        (_, i3, _), (_, i4, _) = (sx.plane_z(fr["insts"][j][2][0], W, H) for j in (3, 4))
        common = i3 & i4
        assert common.sum() > 50 and (win[common] == first + 3).sum() > 20 and (win[common] == first + 4).sum() == 0
        assert (win[i4 & ~i3] == first + 4).sum() > 5
        # (d): instance 5 (alpha-tested, holes) in front of its duplicate 6, which shows through the holes
        assert (win == first + 5).sum() > 10 and (win == first + 6).sum() > 10
