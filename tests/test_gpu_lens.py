"""csg_lens_remap and csg_lens_points on the GPU: the bits of every output against the NumPy restatement of
tests/lens_ref.py on adversarial sources -- the five test lenses' maps and hand-made maps (clamped taps,
fractions 0 and 255, tagged entries of every and of unknown causes, untagged entries far outside and negative),
frame sizes from 1 x 1 to 240 x 320 with sources of other sizes -- the identity lens, subsets of outputs, both
filters, a stream, unaligned leads, repeatability, every argument check, the keypoints against
lens.distort_points, and a rendered frame against the restatement on the CPU oracle's render.  Outputs are
prefilled with 7 and followed by a guard that must stay untouched."""
import ctypes as C

import numpy as np
import pytest

from tests import lens_ref as R

pytestmark = pytest.mark.gpu
FILL = 0x07
GUARD = 4096         # bytes behind every output that must stay untouched
DTYPE = {"lens_rgb": np.uint8, "lens_instance": np.int32, "lens_depth": np.float32, "lens_coords": np.uint16,
         "lens_valid": np.uint8, "lens_stats": np.uint32, "lens_count": np.uint32}
NAMES = tuple(DTYPE)
SOURCE_OF = {"lens_rgb": "rgb", "lens_instance": "instance", "lens_depth": "depth", "lens_coords": "obj_coords",
             "lens_stats": "instance"}
L = 5                # labels of the adversarial sources


def _shape(name, n, H, W, n_labels):
    return {"lens_rgb": (n, H, W, 3), "lens_coords": (n, H, W, 3), "lens_stats": (n, n_labels, 5),
            "lens_count": (n, 3)}.get(name, (n, H, W))


@pytest.fixture(scope="module")
def ctx(cone):
    """One context for every shape of the module (its own size is irrelevant)."""
    from constructionsceneposeestimation_amd.renderer import Renderer
    with Renderer(cone, 64, 64, max_frames=1) as r:
        yield r


def _dev(a, lead=0):
    """The bytes of ``a`` on the device behind ``lead`` spare bytes -> (tensor, pointer to the data)."""
    import torch
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.zeros(lead + raw.size + 16, dtype=torch.uint8, device=torch.device("cuda", 0))
    t[lead:lead + raw.size] = torch.from_numpy(raw.copy()).to(t.device)
    return t, t.data_ptr() + lead


def _run(r, mp, src, SW, SH, names=NAMES, n_labels=L, rgb_filter="bilinear", stream=None, lead=None, what=""):
    """The pass on the sources ``src`` (name -> array of n frames) -> the outputs in ``names`` on the host."""
    import torch
    H, W = mp.shape[:2]
    n = len(next(iter(src.values())))
    lead = lead or {}
    keep = {k: _dev(v, lead.get(k, 0)) for k, v in src.items()}
    keep["map"] = _dev(mp, lead.get("map", 0))
    size = {k: int(np.prod(_shape(k, n, H, W, n_labels))) * np.dtype(DTYPE[k]).itemsize for k in names}
    bufs = {k: torch.full((size[k] + GUARD,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0)) for k in names}
    torch.cuda.synchronize()
    r.lens_remap(n, map=keep["map"][1], width=W, height=H, src_width=SW, src_height=SH, n_labels=n_labels,
                 rgb_filter=rgb_filter, stream=stream.cuda_stream if stream is not None else 0,
                 **{k: keep[k][1] for k in src}, **{k: t.data_ptr() for k, t in bufs.items()})
    if stream is not None:
        stream.synchronize()
    r.synchronize()
    out = {}
    for k, t in bufs.items():
        raw = t.cpu().numpy()
        assert (raw[-GUARD:] == FILL).all(), f"{what}: the guard behind {k} was written"
        out[k] = raw[:-GUARD].view(DTYPE[k]).reshape(_shape(k, n, H, W, n_labels))
    return out


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(got, exp, what):
    for k in got:
        g, x = _bits(got[k]), _bits(exp[k])
        assert g.dtype == x.dtype and g.shape == x.shape, f"{what}: {k}"
        bad = np.argwhere(g != x)
        assert len(bad) == 0, (f"{what}: {k}: {len(bad)} values differ, first at {bad[:4].tolist()}: "
                               f"{g[tuple(bad[0])]} != {x[tuple(bad[0])]}")


def _sources(n, SH, SW, seed):
    rgb, inst, depth, coords = R.sources(n, SH, SW, L, seed)
    return {"rgb": rgb, "instance": inst, "depth": depth, "obj_coords": coords}


def _both(r, mp, src, SW, SH, what, **kw):
    n = len(src["rgb"])
    got = _run(r, mp, src, SW, SH, what=what, **kw)
    exp = R.remap(mp, SW, SH, n, n_labels=kw.get("n_labels", L), nearest=kw.get("rgb_filter") == "nearest", **src)
    _check(got, exp, what)
    return got, exp


@pytest.mark.parametrize("H,W", R.SIZES)
def test_the_five_lenses_on_adversarial_sources(ctx, H, W):
    f = 200.0 * max(W, H) / 320.0
    SW, SH = W + 13, H + 7
    src = _sources(2, SH, SW, 100 * H + W)
    seen = np.zeros(3, np.int64)
    for name, c in R.LENSES.items():
        mp, counts = R.lens_map(R.model(c, W=W, H=H, fx=f, src=(SW, SH), sf=(0.8 * f, 0.8 * f)))
        seen += counts
        for flt in ("bilinear", "nearest"):
            got, exp = _both(ctx, mp, src, SW, SH, f"{name} {H}x{W} {flt}", rgb_filter=flt)
        assert exp["lens_count"][0].tolist() == counts.tolist()
    if H * W > 1000:
        assert (seen > 0).all(), seen


@pytest.mark.parametrize("H,W,SH,SW", [(1, 1, 1, 1), (3, 5, 2, 9), (1, 130, 7, 3), (67, 131, 50, 77), (240, 320, 131, 517),
                                       (17, 64, 1, 300), (16, 65, 300, 1)])
def test_hand_made_maps(ctx, H, W, SH, SW):
    src = _sources(3, SH, SW, H + W)
    mp = R.hand_map(H, W, SH, SW, 7 * H + W)
    for flt in ("bilinear", "nearest"):
        got, exp = _both(ctx, mp, src, SW, SH, f"hand-made {H}x{W} from {SH}x{SW} {flt}", rgb_filter=flt)
    if H * W > 100:
        assert (exp["lens_count"][0] > 0).all()


def test_identity_lens_copies_every_source(ctx):
    for H, W in R.SIZES:
        src = _sources(2, H, W, 3 * H + W)
        mp, _ = R.lens_map(R.identity_model(W, H))
        for flt in ("bilinear", "nearest"):
            got = _run(ctx, mp, src, W, H, rgb_filter=flt, what=f"identity {H}x{W}")
            assert np.array_equal(got["lens_rgb"], src["rgb"]) and np.array_equal(got["lens_instance"], src["instance"])
            assert np.array_equal(got["lens_depth"].view(np.uint32), src["depth"].view(np.uint32))
            assert np.array_equal(got["lens_coords"], src["obj_coords"]) and not got["lens_valid"].any()
            assert (got["lens_count"] == [H * W, 0, 0]).all()
            _check({"lens_stats": got["lens_stats"]}, R.remap(mp, W, H, 2, instance=src["instance"], n_labels=L), "stats")


def test_subsets_filters_streams_leads_and_repeats(ctx):
    import torch
    H, W, SH, SW = 67, 131, 80, 150
    src = _sources(3, SH, SW, 11)
    mp, _ = R.lens_map(R.model(R.LENSES["barrel"], W=W, H=H, fx=80.0, src=(SW, SH), sf=(60.0, 60.0)))
    full, exp = _both(ctx, mp, src, SW, SH, "full")
    again = _run(ctx, mp, src, SW, SH, what="again")
    assert all(full[k].tobytes() == again[k].tobytes() for k in NAMES)             # two runs, equal bytes
    for names in [(k,) for k in NAMES] + [("lens_rgb", "lens_count"), ("lens_instance", "lens_depth"),
                                          ("lens_coords", "lens_valid", "lens_stats")]:
        need = {SOURCE_OF[k] for k in names if k in SOURCE_OF}
        part = _run(ctx, mp, {k: v for k, v in src.items() if k in need} or {"rgb": src["rgb"]}, SW, SH, names=names,
                    what=str(names))
        _check(part, exp, str(names))
    for n_labels in (1, 3, 256):
        _both(ctx, mp, src, SW, SH, f"{n_labels} labels", n_labels=n_labels)
    st = torch.cuda.Stream(torch.device("cuda", 0))
    got = _run(ctx, mp, src, SW, SH, stream=st, what="stream")
    assert all(full[k].tobytes() == got[k].tobytes() for k in NAMES)
    # unaligned leads where the spec allows them: rgb at any byte, obj_coords at 2, ids and depth at 4, the map at 8
    for lead in (dict(rgb=1, obj_coords=2, instance=4, depth=4, map=8), dict(rgb=3, obj_coords=6, instance=12, depth=20, map=24)):
        got = _run(ctx, mp, src, SW, SH, lead=lead, what=f"leads {lead}")
        assert all(full[k].tobytes() == got[k].tobytes() for k in NAMES), lead
    from constructionsceneposeestimation_amd._lib import CsgError
    for lead in (dict(map=4), dict(obj_coords=1), dict(instance=2), dict(depth=1)):   # ... and a refusal where not
        with pytest.raises(CsgError, match="aligned"):
            _run(ctx, mp, src, SW, SH, lead=lead, what=f"leads {lead}")


def test_argument_checks(ctx):
    import torch
    from constructionsceneposeestimation_amd import _lib
    lib = ctx.lib
    dev = torch.device("cuda", 0)
    H = W = SH = SW = 8
    n_src = SH * SW
    rgb = torch.zeros((n_src * 3 + 16,), dtype=torch.uint8, device=dev)
    ids = torch.zeros((n_src + 16,), dtype=torch.int32, device=dev)
    dep = torch.ones((n_src + 16,), dtype=torch.float32, device=dev)
    crd = torch.zeros((n_src * 3 + 16,), dtype=torch.int16, device=dev)
    mp = torch.from_numpy(R.lens_map(R.identity_model(W, H))[0]).to(dev)
    outs = {k: torch.full((int(np.prod(_shape(k, 1, H, W, L))) * np.dtype(DTYPE[k]).itemsize + 16,), FILL,
                          dtype=torch.uint8, device=dev) for k in NAMES}

    def job(**kw):
        f = dict(width=W, height=H, src_width=SW, src_height=SH, n_labels=L, rgb_filter=0, map=mp.data_ptr(),
                 rgb=rgb.data_ptr(), instance=ids.data_ptr(), depth=dep.data_ptr(), obj_coords=crd.data_ptr(),
                 **{k: t.data_ptr() for k, t in outs.items()})
        f.update(kw)
        j = _lib.LensJob()
        for k, v in f.items():
            setattr(j, k, v)
        return j

    def call(j, n=1):
        return lib.csg_lens_remap(ctx.ctx, C.byref(j) if j is not None else None, n, None)

    assert lib.csg_lens_remap(None, C.byref(job()), 1, None) == -1
    assert call(None) == -1 and b"null job" in lib.csg_last_error(ctx.ctx)
    assert call(job(), n=0) == -1
    none = {k: None for k in NAMES}
    for bad in (dict(width=0), dict(height=0), dict(width=8193), dict(height=8193), dict(src_width=0), dict(src_height=0),
                dict(src_width=8193), dict(src_height=8193), dict(rgb_filter=2), dict(map=None), none,
                dict(rgb=None), dict(instance=None), dict(depth=None), dict(obj_coords=None),
                dict(none, lens_stats=outs["lens_stats"].data_ptr(), instance=None), dict(n_labels=0),
                dict(map=mp.data_ptr() + 4), dict(instance=ids.data_ptr() + 2), dict(depth=dep.data_ptr() + 1),
                dict(obj_coords=crd.data_ptr() + 1), dict(lens_rgb=outs["lens_rgb"].data_ptr() + 2),
                dict(lens_instance=outs["lens_instance"].data_ptr() + 1), dict(lens_depth=outs["lens_depth"].data_ptr() + 2),
                dict(lens_coords=outs["lens_coords"].data_ptr() + 2), dict(lens_stats=outs["lens_stats"].data_ptr() + 1),
                dict(lens_count=outs["lens_count"].data_ptr() + 2),
                dict(lens_rgb=rgb.data_ptr()), dict(lens_instance=ids.data_ptr() + 32), dict(lens_depth=dep.data_ptr()),
                dict(lens_coords=crd.data_ptr() + 8), dict(lens_valid=mp.data_ptr() + 17), dict(lens_count=mp.data_ptr()),
                dict(lens_valid=outs["lens_rgb"].data_ptr() + 5), dict(lens_depth=outs["lens_instance"].data_ptr() + 4)):
        assert call(job(**bad)) == -1, bad
        assert lib.csg_last_error(ctx.ctx).startswith(b"lens_remap:"), bad
    assert call(job(n_labels=257)) == -5                                           # CSG_ERR_LIMIT
    ctx.synchronize()
    assert all((t.cpu().numpy() == FILL).all() for t in outs.values())             # nothing enqueued or written
    assert call(job()) == 0
    assert call(job(**dict(none, lens_valid=outs["lens_valid"].data_ptr() + 1), n_labels=0, rgb=None, instance=None,
                    depth=None, obj_coords=None)) == 0                             # lens_valid needs no alignment, no labels
    ctx.synchronize()
    assert outs["lens_count"].cpu().numpy()[:12].view(np.uint32).tolist() == [H * W, 0, 0]
    # csg_lens_points
    m = _lens().LensModel.from_dict(R.identity_model(W, H)).to_c()
    uv = torch.zeros((4, 2), dtype=torch.float32, device=dev)
    vis = torch.ones((4,), dtype=torch.int32, device=dev)
    ouv, ovis = torch.zeros_like(uv), torch.zeros_like(vis)

    def pjob(**kw):
        f = dict(model=C.pointer(m), n_keypoints=4, keypoints_uv=uv.data_ptr(), keypoints_vis=vis.data_ptr(),
                 lens_uv=ouv.data_ptr(), lens_vis=ovis.data_ptr())
        f.update(kw)
        j = _lib.LensJob()
        for k, v in f.items():
            setattr(j, k, v)
        return j

    bad_model = _lens().LensModel.from_dict(dict(R.identity_model(W, H), fx=0.0)).to_c()
    assert lib.csg_lens_points(None, C.byref(pjob()), 1, None) == -1
    assert lib.csg_lens_points(ctx.ctx, None, 1, None) == -1 and lib.csg_lens_points(ctx.ctx, C.byref(pjob()), 0, None) == -1
    for bad in (dict(model=None), dict(model=C.pointer(bad_model)), dict(n_keypoints=0), dict(n_keypoints=65537),
                dict(keypoints_uv=None), dict(keypoints_vis=None), dict(lens_uv=None), dict(lens_vis=None),
                dict(keypoints_uv=uv.data_ptr() + 2), dict(lens_vis=ovis.data_ptr() + 1), dict(lens_uv=uv.data_ptr()),
                dict(lens_vis=vis.data_ptr()), dict(lens_vis=ouv.data_ptr() + 4)):
        assert lib.csg_lens_points(ctx.ctx, C.byref(pjob(**bad)), 1, None) == -1, bad
        assert lib.csg_last_error(ctx.ctx).startswith(b"lens_points:"), bad
    assert lib.csg_lens_points(ctx.ctx, C.byref(pjob()), 1, None) == 0
    ctx.synchronize()
    assert ovis.cpu().tolist() == [1, 1, 1, 1]


def _lens():
    from constructionsceneposeestimation_amd import lens
    return lens


def test_points_against_distort_points(ctx):
    import torch
    lens = _lens()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    for name in R.LENSES:
        m = lens.LensModel.from_dict(R.model(R.LENSES[name], src=(480, 360), sf=(150.0, 150.0)))
        n, K = 3, 211
        uv = rng.uniform(-60.0, 540.0, (n, K, 2)).astype(np.float32)        # outside the frame and beyond the fold too
        uv.reshape(-1, 2)[:6] = [[np.nan, 5.0], [5.0, np.inf], [-np.inf, np.nan], [3e38, -3e38], [240.0, 180.0], [1e-40, 0.0]]
        vis = rng.integers(0, 3, (n, K)).astype(np.int32)
        exp_uv, exp_vis = lens.distort_points(m, uv, vis)
        if name == "fold":
            assert ((exp_vis == 0) & (vis > 0)).sum() > 50
        keep = [_dev(uv), _dev(vis)]
        out_uv = torch.full((n * K * 8 + GUARD,), FILL, dtype=torch.uint8, device=dev)
        out_vis = torch.full((n * K * 4 + GUARD,), FILL, dtype=torch.uint8, device=dev)
        ctx.lens_points(n, m, n_keypoints=K, keypoints_uv=keep[0][1], keypoints_vis=keep[1][1], lens_uv=out_uv.data_ptr(),
                        lens_vis=out_vis.data_ptr())
        ctx.synchronize()
        g_uv, g_vis = out_uv.cpu().numpy(), out_vis.cpu().numpy()
        assert (g_uv[-GUARD:] == FILL).all() and (g_vis[-GUARD:] == FILL).all()
        _check({"uv": g_uv[:-GUARD].view(np.float32).reshape(n, K, 2), "vis": g_vis[:-GUARD].view(np.int32).reshape(n, K)},
               {"uv": exp_uv, "vis": exp_vis}, f"points {name}")


@pytest.fixture(scope="module")
def cone_lens():
    """Two frames of the cone workload C1 rendered by the CPU oracle at a source camera fitted to the tame lens
    (320 x 240 output, 400 x 300 source), with the oracle's keypoints and the restated object coordinates."""
    from constructionsceneposeestimation_amd.labels import object_unit_transforms
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import make_frames
    from constructionsceneposeestimation_amd.workload import Workload
    from oracle.oracle import Oracle
    from tests.test_obj_coords import restate_obj_coords
    lens = _lens()
    model = lens.fit_source(lens.output_camera(R.LENSES["tame"], 320, 240, 200.0), src_size=(400, 300))
    SW, SH = model.src_width, model.src_height
    fids = [2, 5]
    wl = Workload("C1", seed=0, width=SW, height=SH)
    st = wl.epoch(0)
    Vs, _ = wl.frame_params(fids)
    P = np.zeros((4, 4))
    P[0], P[1], P[3] = [model.sfx, 0.0, -model.scx, 0.0], [0.0, -model.sfy, -model.scy, 0.0], [0.0, 0.0, -1.0, 0.0]
    Ps = np.stack([P] * len(fids))
    o = Oracle(pack_scene(wl.scene), SW, SH)
    o.set_instance_models(np.asarray(st.models, np.float32).reshape(-1, 16))
    ref = [o.render(Vs[k], Ps[k], extra=True) for k in range(len(fids))]
    A = object_unit_transforms(wl.scene, st.object_frames)
    src = {"rgb": np.stack([r["rgb"] for r in ref]), "instance": np.stack([r["instance"] for r in ref]),
           "depth": np.stack([r["depth"] for r in ref]),
           "obj_coords": np.stack([restate_obj_coords(r["instance"], r["points"], A) for r in ref])}
    kp = [o.keypoints(Vs[k], Ps[k], st.keypoints, ref[k]["depth"]) for k in range(len(fids))]
    stats = np.stack([r["inst_stats"] for r in ref])
    for a in src.values():
        a.setflags(write=False)
    return dict(wl=wl, st=st, fr=make_frames(Vs, Ps, [0] * len(fids), fids), model=model, src=src, stats=stats,
                uv=np.stack([k[0] for k in kp]), vis=np.stack([k[1] for k in kp]))


def test_a_rendered_frame_through_the_tame_lens(cone_lens):
    import torch
    from constructionsceneposeestimation_amd.renderer import Renderer
    lens = _lens()
    c = cone_lens
    model, src, wl = c["model"], c["src"], c["wl"]
    n, SW, SH, H, W = 2, model.src_width, model.src_height, model.height, model.width
    mp, counts = R.lens_map(model.as_dict())
    assert counts.tolist() == [W * H, 0, 0]
    with Renderer(wl.scene, SW, SH, max_frames=n) as r:
        nl = r.n_labels
        exp = R.remap(mp, SW, SH, n, n_labels=nl, **src)
        exp_uv, exp_vis = lens.distort_points(model, c["uv"], c["vis"])
        assert (exp["lens_instance"] >= 0).sum() > 2000 and (exp_vis == 2).sum() >= 1   # before it compares
        r.set_instance_transforms(0, c["st"].models)
        r.set_keypoints(0, c["st"].keypoints)
        r.set_object_frames(0, c["st"].object_frames)
        for keep in (r.keep_rgb, r.keep_instance, r.keep_depth):
            keep(True)
        dev = torch.device("cuda", 0)
        d_oc = torch.empty((n, SH, SW, 3), dtype=torch.int16, device=dev)
        host = r.render(c["fr"], want=("keypoints", "stats"))
        assert np.array_equal(host["inst_stats"], c["stats"])
        r.render_into(c["fr"].ctypes.data, n, False, obj_coords=d_oc.data_ptr())
        r.synchronize()
        r.render(c["fr"], want=("keypoints", "stats"))
        got = r.lens_remap_host(n, model, rgb=r.last_rgb()[0], instance=r.last_instance()[0], depth=r.last_depth()[0],
                                obj_coords=d_oc.data_ptr(), keypoints_uv=host["keypoints_uv"],
                                keypoints_vis=host["keypoints_vis"])
        names = {"rgb": "lens_rgb", "instance": "lens_instance", "depth": "lens_depth", "coords": "lens_coords",
                 "valid": "lens_valid", "stats": "lens_stats", "count": "lens_count"}
        _check({v: got[k] for k, v in names.items()}, exp, "rendered frame")
        _check({"uv": got["keypoints_uv"], "vis": got["keypoints_vis"]}, {"uv": exp_uv, "vis": exp_vis}, "keypoints")
        # the identity lens at the source camera gives the render's own inst_stats
        ident = lens.LensModel.from_dict(R.identity_model(SW, SH))
        same = r.lens_remap_host(n, ident, instance=r.last_instance()[0])
        assert np.array_equal(same["stats"], host["inst_stats"]) and np.array_equal(same["instance"], src["instance"])
    # a keypoint the source frame shows on its own object lands on that object, or a pixel beside it
    label_of = [wl.scene.objects[j].inst_idx for j, _ in wl.kp_table]
    hits = 0
    for f in range(n):
        for k, lab in enumerate(label_of):
            if got["keypoints_vis"][f, k] != 2 or lab < 0:
                continue
            su, sv = int(np.floor(c["uv"][f, k, 0])), int(np.floor(c["uv"][f, k, 1]))
            if src["instance"][f, sv, su] != lab:
                continue                                            # a box corner in front of something else
            u, v = int(np.floor(got["keypoints_uv"][f, k, 0])), int(np.floor(got["keypoints_uv"][f, k, 1]))
            near = got["instance"][f, max(v - 1, 0):v + 2, max(u - 1, 0):u + 2]
            assert (near == lab).any(), (f, k, lab, near.tolist())
            hits += 1
    print("keypoints on their object:", hits)
    assert hits >= 1


def test_generator_writes_the_lens_files(tmp_path):
    """--outputs rgb,lens on two frames of the cone workload: lens/ holds the restatement of the pass on the
    arrays a second, pinhole run wrote (its RGB files are byte-identical to the first run's); the COCO masks
    decode to lens_instance; lens.json round-trips into the model whose map has the stored digest."""
    import json
    import os
    from constructionsceneposeestimation_amd import masks
    from constructionsceneposeestimation_amd.generate import generate
    from constructionsceneposeestimation_amd.writers import depth_to_u16
    from tests.pngutil import decode_png
    from tests.test_compact_files import decode_png16
    lens = _lens()
    kw = dict(workload="C1", seed=1, batch=2, width=320, height=240, writers=2)
    frames = [3, 4]
    a, b = str(tmp_path / "lens"), str(tmp_path / "plain")
    summary = generate(a, frames, outputs=("rgb", "lens"), lens_coeffs=R.LENSES["tame"][:5], lens_size=(288, 200), **kw)
    generate(b, frames, outputs=("rgb", "mask", "depth_npy"), **kw)
    meta = json.load(open(os.path.join(a, "lens", "lens.json")))
    model = lens.LensModel.from_dict(meta["model"])
    assert (model.width, model.height, model.src_width, model.src_height) == (288, 200, 320, 240)
    assert model.coeffs == R.LENSES["tame"] and meta["opencv"] == model.opencv() and summary["lens"] == meta
    mp, counts = lens.build_map(model)
    assert lens.map_digest(mp) == meta["map_sha256"] and counts[2] == 0
    wider = lens.LensModel.from_dict(dict(meta["model"], fx=model.fx - lens.FOCAL_STEP, fy=model.fy - lens.FOCAL_STEP))
    assert lens.build_map(wider)[1][2] > 0                       # the widest view the source holds
    totals = np.zeros(3, np.int64)
    for f in frames:
        png = open(os.path.join(a, "rgb", f"rgb_{f:06d}.png"), "rb").read()
        assert png == open(os.path.join(b, "rgb", f"rgb_{f:06d}.png"), "rb").read(), f   # the pinhole kinds stay as they are
        src = {"rgb": decode_png(png)[None], "instance": np.load(os.path.join(b, "labels", f"instance_mask_{f:06d}.npy"))[None].astype(np.int32),
               "depth": np.load(os.path.join(b, "depth", f"depth_{f:06d}.npy"))[None].astype(np.float32)}
        exp = R.remap(mp, 320, 240, 1, n_labels=int(src["instance"].max()) + 1, **src)
        totals += exp["lens_count"][0]
        assert np.array_equal(decode_png(open(os.path.join(a, "lens", f"rgb_{f:06d}.png"), "rb").read()), exp["lens_rgb"][0]), f
        assert np.array_equal(decode_png16(open(os.path.join(a, "lens", f"depth16_{f:06d}.png"), "rb").read()),
                              depth_to_u16(exp["lens_depth"][0], 250.0)), f
        frag = json.load(open(os.path.join(a, "lens", f"coco_{f:06d}.json")))
        assert frag["image"] == {"id": f, "file_name": f"rgb_{f:06d}.png", "height": 200, "width": 288}
        ids = exp["lens_instance"][0]
        assert len(frag["annotations"]) >= 1
        for ann in frag["annotations"]:
            lab = ann["inst_idx"]
            mask = masks.decode(ann["segmentation"]["size"], ann["segmentation"]["counts"])
            assert np.array_equal(mask, ids == lab), (f, lab)
            px, x0, y0, x1, y1 = exp["lens_stats"][0][lab].tolist()
            assert ann["area"] == px and ann["bbox"] == [x0, y0, x1 - x0 + 1, y1 - y0 + 1]
            assert len(ann["keypoints"]) % 3 == 0 and all(v in (0, 1, 2) for v in ann["keypoints"][2::3])
    assert [meta["cause_totals"][n] for n in meta["cause_names"]] == totals.tolist()
    assert not os.path.exists(os.path.join(b, "lens"))
