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
list, a depth key without its low 5 bits (caught by cross_near alone).  In the
clip family: the intersection interpolated from the wrong end; the fan's second
sub-triangle not drawn; the fan started at the last emitted vertex; ``<`` for
``<=`` at 1/near; ``>`` for ``>=`` at W = near (with ``all_in``); the trivial
reject in screen space; the normal's flip from the first sub-triangle's
orientation.  In the swap family: the texture table ignored by the alpha test.
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
    # the near plane: W = 1, 1, -1 with the third vertex virtually 16 px to the right.  1 / W falls from 1 at x = 16 px
    # to -1 at 32 px, so it is 2 = 1 / near 8 px to the left of the edge, where the two slanted edges, produced
    # backwards by half their length, arrive: code 3, polygon v0, v1, I12, I20, tt = 1/4 on both crossings
    c = sx.clip_exact(sx.tri([(4096, 1024), (4096, 3072), (8192, 2048)], (1.0, 1.0, -1.0)))
    assert c["code"] == 3 and c["poly"] == [(4096, 1024), (4096, 3072), (2048, 3584), (2048, 512)]
    assert c["tt"] == [0.25, 0.75] and all(c["tt_exact"]) and len(c["subs"]) == 2
    cov = sx.cover_of(sx.tri([(4096, 1024), (4096, 3072), (8192, 2048)], (1.0, 1.0, -1.0)), 32, 16)
    assert cov[7, 8:16].all() and not cov[7, :8].any() and not cov[7, 16:].any() and cov[2, 8] and not cov[1, 8] and cov[13, 8]
    c = sx.clip_exact(sx.tri([(4096, 1024), (4096, 3072), (8192, 2048)], (0.5, 1.0, 0.25)))     # W = near is inside: tt = 1 into it
    assert c["code"] == 3 and c["tt"][1] == 1.0 and c["poly"][3] == c["poly"][0] and sx.area2(c["subs"][1]) == 0


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
                       for t, p in zip(ts, ps) if "clip0" not in t)       # (a vertex of W = 0 has no screen position:)
            assert all(sx.det_exact(t) == -sx.det_exact(p) != 0 for (_, _, ts), (_, _, ps) in zip(fr["insts"], prev["insts"])
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


def _tagged(fr, tag):
    """[(instance index in the frame, triangle index, label, triangle)] of the triangles built for ``tag``."""
    return [(i, k, l, t) for i, (l, _, tris) in enumerate(fr["insts"]) for k, t in enumerate(tris) if t.get("tag") == tag]


def _wins(fr, i, k):
    return fr["uid"] == (((fr["first"] + i) << 20) | k)


@pytest.mark.parametrize("size", SIZES)
def test_the_clip_family_holds_its_cases(size):
    """Near-clipped triangles: every case the family is built for occurs in the generated frames."""
    W, H, b, _ = _frames(size)
    frames = [fr for fr in b["frames"] if fr["family"].startswith("clip")]
    assert [(fr["family"], fr["order"]) for fr in frames] == [(n, o) for n in ("clip", "clip_edge", "clip_tex", "clip_pair")
                                                                      for o in (0, 1)]
    near = Fr(sx.NEAR)
    owed = 0
    seen = {}                                       # (code, det > 0) -> kinds of outside vertices seen
    for fr in frames:
        what = f'{W}x{H} {fr["family"]}/{fr["order"]}'
        if fr["family"] != "clip_tex":
            assert not fr["undecided"].any(), what                  # untextured: nothing is left out
        owed += int(fr["clip_win"].sum()) if fr["order"] == 0 else 0
        flips = [d["shade"]["flipped"] for d in fr["drawn"] if d["n_won"]]
        assert any(flips) and not all(flips), what
        on_clipped = sum(bool(fr["clip_win"][int(v), int(u)]) for (u, v), vis in zip(fr["kp_uv"][:4], fr["kp_vis"][:4]) if vis)
        assert on_clipped >= 2, what                                # keypoints at and just behind a clipped surface
        per_code = {}
        for i, (_, _, tris) in enumerate(fr["insts"]):
            for k, t in enumerate(tris):
                if not sx.is_clipped(t):
                    continue
                c = sx.clip_exact(t)
                assert c is not None, what
                code = c["code"]
                assert len(c["subs"]) == {0: 0, 1: 1, 2: 1, 4: 1, 3: 2, 5: 2, 6: 2}[code], what
                assert all(abs(x) < sx.CLIP_GUARD and abs(y) < sx.CLIP_GUARD for x, y in c["poly"]), what
                if not _wins(fr, i, k).any():
                    continue
                per_code[code] = per_code.get(code, 0) + 1
                out = [w for w in t["w"] if w < sx.NEAR]
                kind = "front" if all(w > 0 for w in out) else "behind" if all(w < 0 for w in out) else "mixed"
                seen.setdefault((code, sx.det_exact(t) > 0), set()).add(kind)
        if fr["family"] == "clip":
            assert all(per_code.get(c, 0) >= 2 for c in (1, 2, 4, 3, 5, 6)), (what, per_code)
            assert fr["aims"]["w_ratio"] >= 32.0, what
    print(f"{W}x{H}: {owed} pixels won by clipped triangles; inside masks and orientations {sorted(seen)}; "
          f'{b["undecided_clips"]} candidates with an undecided clip vertex, W = 0 found after {b["w0_searched"]}')
    assert owed >= (1500 if (W, H) == (96, 64) else 600)
    for code in (1, 2, 4, 3, 5, 6):                                 # each mask in both orientations, outside in front and behind
        assert (code, True) in seen and (code, False) in seen, (code, seen)
        assert {"front", "behind"} <= seen[code, True] | seen[code, False], (code, seen)

    fr = frames[0]                                                  # clip / 0
    first_deg = second_deg = 0
    for i, k, _, t in _tagged(fr, "near_vertex"):                   # a vertex at exactly W = near, one other outside
        c = sx.clip_exact(t)
        assert sx.NEAR in t["w"] and len(c["subs"]) == 2 and (0.0 in c["tt"] or 1.0 in c["tt"])
        deg = [sx.area2(s) == 0 for s in c["subs"]]
        assert sum(deg) == 1 and sx.plane_z(t, W, H)[1].sum() >= 10     # one is dropped, the other drawn
        first_deg, second_deg = first_deg + deg[0], second_deg + deg[1]
    assert first_deg >= 2 and second_deg >= 2 and any(1.0 in sx.clip_exact(t)["tt"] for _, _, _, t in _tagged(fr, "near_vertex"))
    (_, _, _, t), = _tagged(fr, "near_alone")                       # both others outside: three times the same vertex
    assert len(set(sx.clip_exact(t)["poly"])) == 1 and not sx.cover_of(t, W, H).any()
    (i, k, _, t), = _tagged(fr, "near_flat")                        # all three at W = near: inside, drawn, 1 / W = 2 kept
    assert set(t["w"]) == {sx.NEAR} and _wins(fr, i, k).sum() >= 20 and fr["aims"]["z_near_exact"] >= 20
    (_, _, l, t), = _tagged(fr, "invisible")
    assert sorted(t["w"]) == [-2.0, -1.0, -1.0] and l == 5
    assert fr["covered"][5] == 0 and not fr["masks"][5].any() and not fr["beyond"][5].any() and not (fr["ids"] == 5).any()

    fr = frames[2]                                                  # clip_edge / 0
    assert fr["aims"]["z_near_exact"] >= 20
    for axis in "xy":
        for kind in ("incl", "excl"):
            hit = 0
            for i, k, _, t in _tagged(fr, f"edge_{axis}_{kind}"):
                N, _, _, pq = sx._grid_ints(t, W, H)
                line = (N << (sx.PQ - pq)) == sx.Z_NEAR             # the centres with 1 / W = 2 exactly: one column or row
                cov = sx.cover_of(t, W, H)
                ax = 0 if axis == "x" else 1                        # (the axis of the image the line runs along)
                assert line.any() and (line.all(ax) | ~line.any(ax)).all() and line.any(ax).sum() == 1
                assert all(sx.clip_exact(t)["tt_exact"])
                if kind == "incl":                                  # a left / top edge: its centres are covered, and kept by <=
                    assert (cov & line).sum() >= 5 and (_wins(fr, i, k) & line).any()
                else:                                               # a right / bottom edge: they are not, their neighbours are
                    assert not (cov & line).any() and (cov & np.roll(line, -1, 1 - ax)).sum() >= 5
                hit += 1
            assert hit >= 2, (axis, kind)
    fx = lambda t: [v[0] for v in t["xy"]]                          # noqa: E731
    (i, k, _, t), = _tagged(fr, "hom_sides")                        # virtual vertices left of, right of and above the frame
    assert min(fx(t)) < 0 and max(fx(t)) > W * 256 and min(v[1] for v in t["xy"]) < 0 and min(t["w"]) < 0
    assert all(not (0 <= x <= W * 256 and 0 <= y <= H * 256) for x, y in t["xy"]) and _wins(fr, i, k).sum() >= 100
    (i, k, _, t), = _tagged(fr, "hom_above")                        # all three above it: a reject in screen space would take it
    assert all(y < 0 for _, y in t["xy"]) and min(t["w"]) < 0 and _wins(fr, i, k).sum() >= 20
    for tag in ("hom_sides", "hom_above"):                          # item 2's reject, in rationals, keeps both
        v = sx._clip_space(_tagged(fr, tag)[0][3])
        assert not any(all(f(p) for p in v) for f in (lambda p: p[2] < near, lambda p: p[2] > Fr(sx.FAR), lambda p: p[0] < 0,
                                                      lambda p: p[0] > W * p[2], lambda p: p[1] < 0, lambda p: p[1] > H * p[2]))
    w0 = _tagged(fr, "w0")                                          # a vertex with W = 0 (the seeded search finds them)
    assert len(w0) >= 1 and all(0.0 in t["w"] and "clip0" in t for _, _, _, t in w0)
    assert sum(int(_wins(fr, i, k).sum()) for i, k, _, _ in w0) >= 10

    fr = frames[4]                                                  # clip_tex / 0
    a = fr["aims"]
    assert a["alpha_tested"] >= 100 and 0 < a["alpha_killed"] < a["alpha_tested"] and a["textured"] > a["alpha_tested"]
    cards = _tagged(fr, "card")
    assert len(cards) == 4 and all(sx.is_clipped(t) and t["uv"] is not None for _, _, _, t in cards)
    for i in sorted({i for i, _, _, _ in cards}):                   # per card: two triangles, one texture
        l, m, tris = fr["insts"][i]
        mt = b["scene"].materials[m]
        tex = b["scene"].textures[mt.texture].rgba
        cols = np.nonzero((tex[..., 3] == 255).any(0))[0].tolist()
        assert mt.alpha_test and (tex[..., 3] == 255).sum() == 8 and len(cols) == 4 and cols[1] == cols[0] + 1 and cols[3] == cols[2] + 1
        vis, cut = cols[0], cols[2]                                 # two 2 x 2 blocks: columns vis, vis + 1 and cut, cut + 1
        tx, _, alpha = (np.concatenate(x) for x in zip(*(sx.texels_of(t, tex, W, H) for t in tris)))
        drawn = alpha > mt.alpha_threshold
        print(f"{W}x{H} card {i}: texel columns {int(tx.min())} .. {int(tx.max())} read, {sorted(set(tx[drawn].tolist()))} drawn, "
              f"blocks at {vis} and {cut}")
        assert drawn.sum() >= 10 and set(tx[drawn].tolist()) <= {vis - 1, vis, vis + 1}      # the visible side's block is drawn,
        assert tx.max() + 1 < cut < 10 and tx.min() >= -1           # the other, on the card but beyond the clip line, is never read
        assert fr["masks"][l].any()
    assert all(sx.is_clipped(t) for _, m, ts in fr["insts"] for t in ts if b["scene"].materials[m].alpha_test)   # none to trim
    fr = frames[6]                                                  # clip_pair / 0
    for tag, both_clipped in (("pair_cc", True), ("pair_cu", False)):
        (ia, ka, la, ta), (ib, kb, lb, tb) = _tagged(fr, tag)
        assert la != lb and sx.is_clipped(ta) and sx.is_clipped(tb) == both_clipped
        (_, ra, _), (_, rb, _) = sx.plane_z(ta, W, H), sx.plane_z(tb, W, H)
        common = ra & rb                                            # in range under both: inside the clipped region of ta
        wa, wb = int((_wins(fr, ia, ka) & common).sum()), int((_wins(fr, ib, kb) & common).sum())
        print(f"{W}x{H} {tag}: {int(common.sum())} common pixels, won {wa} / {wb}")
        assert wa >= sx.pair_need(H) and wb >= sx.pair_need(H), (tag, wa, wb)
        assert (fr["ids"][common] == la).any() and (fr["ids"][common] == lb).any()


@pytest.mark.parametrize("size", SIZES)
def test_the_swap_family_holds_its_cases(size):
    """Texture tables: the frames share their instances and differ in the table alone, and each table does
    to the expected image what it is there for."""
    W, H, b, _ = _frames(size)
    sc = b["scene"]
    for order in (0, 1):
        fam = {fr["family"]: fr for fr in b["frames"] if fr["family"].startswith("swap") and fr["order"] == order}
        assert set(fam) == {"swap_id", "swap_keep", "swap_rgb", "swap_alpha", "swap_4x4", "swap_npot", "swap_none"}
        one = fam["swap_id"]
        assert all((fr["first"], fr["count"], fr["light"]) == (one["first"], one["count"], one["light"]) and
                   fr["insts"] is not None and [t for _, _, ts in fr["insts"] for t in ts] == [t for _, _, ts in one["insts"] for t in ts]
                   for fr in fam.values())
        tables = [tuple(fr["table"].tolist()) for fr in fam.values()]
        assert len(set(tables)) == len(tables) == 7 and all(len(t) == len(sc.materials) for t in tables)
        assert set(fam["swap_keep"]["table"].tolist()) == {sx.KEEP_TEXTURE}
        base = sx.render(one["insts"], sc, b["lights"][0], W, H, W // 2, H // 2, one["first"])     # no table at all

        def same(a, c, keys=("ids", "rgb", "normals", "masks", "undecided", "covered")):
            return all(np.array_equal(a[k], c[k]) for k in keys) and np.array_equal(a["depth"].view(np.uint32), c["depth"].view(np.uint32))
        assert same(one, base) and same(fam["swap_keep"], base)
        ma = [m for m, mt in enumerate(sc.materials) if mt.alpha_test and one["table"][m] >= 0]
        mo = [m for m, mt in enumerate(sc.materials) if not mt.alpha_test and one["table"][m] >= 0]
        assert len(ma) == 1 and len(mo) == 1
        ma, mo = ma[0], mo[0]
        tex = lambda name, m: sc.textures[fam[name]["table"][m]].rgba      # noqa: E731
        decided = lambda a, c: ~a["undecided"] & ~c["undecided"]           # noqa: E731
        # other RGB, the same alpha: the same pixels are drawn, in other colours
        r = fam["swap_rgb"]
        assert np.array_equal(tex("swap_rgb", ma)[..., 3], tex("swap_id", ma)[..., 3]) and tex("swap_rgb", ma).shape == (8, 16, 4)
        assert same(r, base, ("ids", "masks", "covered", "normals")) and ((r["rgb"] != base["rgb"]).any(-1) & decided(r, base)).sum() >= 20
        # the opaque block elsewhere: other pixels are drawn
        r = fam["swap_alpha"]
        assert tex("swap_alpha", ma).shape == (8, 16, 4) and not np.array_equal(tex("swap_alpha", ma)[..., 3], tex("swap_id", ma)[..., 3])
        moved = int(((r["ids"] != base["ids"]) & decided(r, base)).sum())
        print(f"{W}x{H} swap_alpha/{order}: {moved} decided pixels change their id")
        assert moved >= 20 and not np.array_equal(r["covered"], base["covered"])
        # other sizes
        assert tex("swap_4x4", ma).shape == (4, 4, 4) and tex("swap_npot", ma).shape == (7, 13, 4) and tex("swap_id", ma).shape == (8, 16, 4)
        for name in ("swap_4x4", "swap_npot"):
            r = fam[name]
            assert r["aims"]["alpha_tested"] >= 200 and 0 < r["aims"]["alpha_killed"] < r["aims"]["alpha_tested"]
            assert ((r["ids"] != base["ids"]) & decided(r, base)).sum() >= 20
        # no texture on the opaque material: its pixels show the base colour alone, everything else stays
        r = fam["swap_none"]
        assert r["table"][mo] == -1 and same(r, base, ("ids", "masks", "covered", "normals"))
        own = np.zeros((H, W), bool)
        for i, (_, m, ts) in enumerate(r["insts"]):
            for k in range(len(ts)):
                own |= _wins(r, i, k) if m == mo else False
        assert own.sum() >= 50 and np.array_equal(r["rgb"][~own], base["rgb"][~own]) and (r["rgb"][own] != base["rgb"][own]).any()
        assert len({tuple(c) for c in r["rgb"][own].tolist()}) <= 2      # two triangles, one colour each
        assert r["aims"]["textured"] < base["aims"]["textured"]
