"""csg_crop_amodal on the GPU: every mask is bit-exact against the restatement
of tests/test_crop_amodal.py (the CPU oracle renders the frame without the other
labels, the crops' restatement samples it) -- planned crops of rendered frames
behind a render and the crops on one stream, the near plane, more labels than
the coverage table holds, a texture swap, dead slots, argument checks and the
host-delivery wrapper.  Outputs are prefilled with 7."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import pose_frames
from tests.test_crop_amodal import (FIDS3, H3, K3, MINPX3, PAD3, S3, UNKNOWN, W3, amodal_image, c3_reference,
                                    restate_amodal)
from tests.test_object_crops import INFO_DTYPE

pytestmark = pytest.mark.gpu
FILL = 7


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def _filled(shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def _explicit(rows_per_frame, K):
    """info (n, K) from per-frame lists of (label, x0, y0, side); the other slots are empty."""
    info = np.zeros((len(rows_per_frame), K), INFO_DTYPE)
    info["label"] = -1
    for f, rows in enumerate(rows_per_frame):
        for k, (label, x0, y0, side) in enumerate(rows):
            info[f, k] = (label, 0, x0, y0, side, f, (0, 0))
    return info


def _amodal(r, fr, info, S):
    """crop_amodal of explicit windows ``info`` (n, K) on the context's stream -> (n, K, S, S) uint8."""
    n, K = info.shape
    d_info, out = _dev(info), _filled((n, K, S, S))
    r.crop_amodal(fr, size=S, per_frame=K, info=d_info.data_ptr(), crop_amodal=out.data_ptr())
    r.synchronize()
    assert d_info.cpu().numpy().tobytes() == info.tobytes(), "info was written"   # (bytes: a side may be NaN)
    return out.cpu().numpy()


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (f"{what}: {len(bad)} samples differ (got {int((got > 0).sum())} set, expected "
                           f"{int((exp > 0).sum())}), first at {bad[:4].tolist()}")


def _upload(r, wl, epochs):
    for k, e in enumerate(epochs):
        r.set_instance_transforms(k, wl.epoch(e).models)


def _device_path(r, ref):
    """render_into -> crop_objects (planned) -> crop_amodal on one stream, nothing in between."""
    import torch
    dev = torch.device("cuda", 0)
    n, fr = 3, ref["fr"]
    inst = torch.empty((n, H3, W3), dtype=torch.int32, device=dev)
    stats = torch.empty((n, r.n_labels, 5), dtype=torch.int32, device=dev)
    mask, amodal = _filled((n, K3, S3, S3)), _filled((n, K3, S3, S3))
    info = _filled((n, K3, INFO_DTYPE.itemsize))
    el = _dev(ref["elig"])
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    r.render_into(fr.ctypes.data, n, False, instance=inst.data_ptr(), stats=stats.data_ptr(), stream=stream.cuda_stream)
    r.crop_objects(n, size=S3, per_frame=K3, min_pixels=MINPX3, pad=PAD3, instance=inst.data_ptr(),
                   stats=stats.data_ptr(), eligible=el.data_ptr(), crop_mask=mask.data_ptr(), info=info.data_ptr(),
                   stream=stream.cuda_stream)
    r.crop_amodal(fr, size=S3, per_frame=K3, info=info.data_ptr(), crop_amodal=amodal.data_ptr(),
                  stream=stream.cuda_stream)
    stream.synchronize()
    r.synchronize()
    return (mask.cpu().numpy(), amodal.cpu().numpy(),
            info.cpu().numpy().view(INFO_DTYPE).reshape(n, K3), inst.cpu().numpy())


@pytest.mark.parametrize("kinds", [None, ("static",)])
def test_rendered_frames_behind_the_crops(kinds):
    from constructionsceneposeestimation_amd.renderer import Renderer
    ref = c3_reference(kinds)
    wl = ref["wl"]
    with Renderer(wl.scene, W3, H3, max_frames=3) as r:
        assert r._n_inst_labels == ref["n_labels"] == r.n_labels
        _upload(r, wl, ref["epochs"])
        mask, amodal, info, inst = _device_path(r, ref)
    assert np.array_equal(inst, ref["instance"])              # a difference here is the renderer's
    for name in INFO_DTYPE.names:                             # planned, and untouched by the amodal pass
        assert np.array_equal(np.ascontiguousarray(info[name]).view(np.uint32),
                              np.ascontiguousarray(ref["info"][name]).view(np.uint32)), name
    _same(mask, ref["crop_mask"], "visible masks")
    _same(amodal, ref["crop_amodal"], f"amodal masks, kinds {kinds}")
    assert (mask <= amodal).all()


def test_render_crops_delivers_the_same():
    """n = 3 with max_frames = 2: two chunks, the amodal pass behind the crops of each."""
    from constructionsceneposeestimation_amd.renderer import Renderer
    ref = c3_reference(None)
    wl = ref["wl"]
    with Renderer(wl.scene, W3, H3, max_frames=2) as r:
        _upload(r, wl, ref["epochs"])
        got = r.render_crops(ref["fr"], size=S3, per_frame=K3, min_pixels=MINPX3, pad=PAD3,
                             want=("rgb", "mask", "amodal"))
    assert set(got) == {"crop_rgb", "crop_mask", "crop_amodal", "info", "intrinsics"}
    assert np.array_equal(got["info"]["label"], ref["info"]["label"])
    _same(got["crop_mask"], ref["crop_mask"], "render_crops: visible")
    _same(got["crop_amodal"], ref["crop_amodal"], "render_crops: amodal")


def test_back_to_back_on_two_streams_with_reused_frame_records():
    """Two passes share the pass's scratch: the second, on another stream, waits for the first on the
    device, and the caller's frame records may be overwritten as soon as a call returns."""
    import torch
    from constructionsceneposeestimation_amd.renderer import Renderer
    ref = c3_reference(None)
    wl, dev = ref["wl"], torch.device("cuda", 0)
    info = _dev(ref["info"])
    first, second = _filled((3, K3, S3, S3)), _filled((1, K3, S3, S3))
    with Renderer(wl.scene, W3, H3, max_frames=3) as r:
        _upload(r, wl, ref["epochs"])
        r.synchronize()
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        fr = ref["fr"].copy()
        r.crop_amodal(fr, size=S3, per_frame=K3, info=info.data_ptr(), crop_amodal=first.data_ptr())
        fr[:] = fr[[2, 0, 1]]                                 # frame 2's record now stands first
        r.crop_amodal(fr[:1], size=S3, per_frame=K3, info=info[2:].data_ptr(), crop_amodal=second.data_ptr(),
                      stream=stream.cuda_stream)
        fr.view(np.uint8)[:] = 0
        stream.synchronize()
        r.synchronize()
    _same(first.cpu().numpy(), ref["crop_amodal"], "first pass, the context's stream")
    _same(second.cpu().numpy()[0], ref["crop_amodal"][2], "second pass, another stream")


def test_near_plane(cone):
    """The cone cut by the near plane (0.5): the near-clip fan, at step 1, minified and magnified."""
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from oracle.oracle import Oracle
    W, H = 96, 64
    V, P = pose_frames([([0.3, -0.55, 0.25], [0.0, 0.0, 0.25]), ([0.0, -0.6, 0.3], [0.0, 0.0, 0.2])], W, H)
    fr = make_frames(V, P, [0, 0], [0, 1])
    packed = pack_scene(cone)
    o = Oracle(packed, W, H)
    L = int(packed.inst_label[0])
    refs = [o.render(V[k], P[k]) for k in range(2)]
    for ref in refs:
        d = ref["depth"][ref["instance"] >= 0]
        print("nearest depth", d.min())
        assert d.min() < 0.501                                # the surface reaches the near plane
    info = _explicit([[(L, 0.0, -16.0, 96.0)]] * 2, 1)
    n_lab = L + 1
    with Renderer(cone, W, H, max_frames=2) as r:
        assert r._n_inst_labels == n_lab
        got = {S: _amodal(r, fr, info, S) for S in (96, 16, 512)}
    for S, g in got.items():
        for k in range(2):
            exp = restate_amodal(o, packed.inst_label, packed.inst_model, V[k], P[k], info[k], S, n_lab)
            assert exp.any() and not exp.all()
            _same(g[k], exp, f"near plane: frame {k}, S = {S}")
    for k in range(2):                                        # step 1: the window copies the frame
        win = np.zeros((96, 96), bool)
        win[16:16 + H] = refs[k]["instance"] >= 0
        assert np.array_equal(got[96][k, 0] == 255, win)


def _cones300(cone):
    from constructionsceneposeestimation_amd.scene.model import Instance, Scene
    sc = Scene(meshes=cone.meshes, materials=cone.materials, textures=cone.textures, light=cone.light)
    base = np.asarray(cone.instances[0].model, np.float64)
    for k in range(300):
        m = base.copy()
        m[0, 3] += 0.35 * (k % 20 - 9.5)
        m[1, 3] += 0.35 * (k // 20)
        sc.instances.append(Instance(mesh=cone.instances[0].mesh, model=m, inst_idx=k))
    return sc


def test_no_label_cap(cone):
    """300 labels seen from afar: tiles hold more labels than label_covered's table, the masks are exact."""
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from oracle.oracle import Oracle
    sc = _cones300(cone)
    W, H, K, S = 320, 180, 64, 16
    V, P = pose_frames([([0.0, -14.0, 4.0], [0.0, 3.0, 0.0])], W, H)
    fr = make_frames(V, P, [0], [0])
    packed = pack_scene(sc)
    o = Oracle(packed, W, H)
    full = o.render(V[0], P[0], covered=True)
    assert (full["label_covered"] & UNKNOWN).any()            # the count is unknown there
    labels = [int(l) for l in np.flatnonzero(full["label_covered"] & UNKNOWN)][:K]
    labels += [l for l in range(0, 300, 3) if l not in labels][:K - len(labels)]
    assert len(set(labels)) == K
    rows = []
    for L in labels:                                          # a side-32 window on the cone's amodal box
        ys, xs = np.nonzero(amodal_image(o, packed.inst_label, packed.inst_model, V[0], P[0], L))
        assert len(xs)
        rows.append((L, (xs.min() + xs.max() + 1) / 2 - 16.0, (ys.min() + ys.max() + 1) / 2 - 16.0, 32.0))
    info = _explicit([rows], K)
    exp = restate_amodal(o, packed.inst_label, packed.inst_model, V[0], P[0], info[0], S, 300)
    assert all(exp[k].any() for k in range(K))
    with Renderer(sc, W, H, max_frames=1) as r:
        got = _amodal(r, fr, info, S)
    _same(got[0], exp, "300 labels")


def test_texture_swap():
    """Tree label 28 of frame 4 under set 0 (the scene's textures) and set 1 (material 3 without its texture)."""
    from constructionsceneposeestimation_amd import _lib
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from oracle.oracle import Oracle
    ref = c3_reference(None)
    wl, L, S = ref["wl"], 28, 64
    V, P = ref["V"][[0, 0]], ref["P"][[0, 0]]
    fr = make_frames(V, P, [0, 1], [4, 4])
    packed = pack_scene(wl.scene)
    o = Oracle(packed, W3, H3)
    models = np.asarray(wl.epoch(0).models, np.float32).reshape(-1, 16)
    swap = [_lib.KEEP_TEXTURE] * len(packed.materials)
    swap[3] = -1
    img = [amodal_image(o, packed.inst_label, models, V[0], P[0], L, t) for t in (None, swap)]
    print("full-frame amodal pixels", int(img[0].sum()), int(img[1].sum()))
    assert (int(img[0].sum()), int(img[1].sum())) == (15327, 19307)
    ys, xs = np.nonzero(img[1])
    side = float(max(xs.max() - xs.min(), ys.max() - ys.min()) + 1) * 1.25
    box = (L, (xs.min() + xs.max() + 1) / 2 - side / 2, (ys.min() + ys.max() + 1) / 2 - side / 2, side)
    info = _explicit([[box], [box]], 1)
    exp = np.stack([restate_amodal(o, packed.inst_label, models, V[0], P[0], info[k], S, ref["n_labels"], t)
                    for k, t in enumerate((None, swap))])
    assert (exp[0] != exp[1]).any()
    with Renderer(wl.scene, W3, H3, max_frames=2) as r:
        r.set_instance_transforms(0, models)
        r.set_instance_transforms(1, models)
        r.set_dr_textures(1, swap)
        got = _amodal(r, fr, info, S)
    _same(got[0], exp[0], "set 0: the scene's textures")
    _same(got[1], exp[1], "set 1: material 3 without texture")


def _two_cones(cone):
    """Labels 0 and 2: label 1 is in the table and no instance carries it."""
    from constructionsceneposeestimation_amd.scene.model import Instance, Scene
    sc = Scene(meshes=cone.meshes, materials=cone.materials, textures=cone.textures, light=cone.light)
    base = np.asarray(cone.instances[0].model, np.float64)
    for k, label in enumerate((0, 2)):
        m = base.copy()
        m[0, 3] += 0.3 * k
        sc.instances.append(Instance(mesh=cone.instances[0].mesh, model=m, inst_idx=label))
    return sc


def test_dead_slots_write_zeros(cone):
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from oracle.oracle import Oracle
    sc = _two_cones(cone)
    W, H, S, K = 96, 64, 16, 8
    V, P = pose_frames([([0.0, -1.6, 0.4], [0.0, 0.0, 0.2])] * 2, W, H)
    fr = make_frames(V, P, [0, 1], [0, 1])                    # frame 1 names set 1: in range, never uploaded
    packed = pack_scene(sc)
    o = Oracle(packed, W, H)
    whole = (0.0, -16.0, 96.0)
    dead = [(-1, *whole), (3, *whole), (1, *whole), (0, 0.0, -16.0, np.nan), (0, 0.0, -16.0, 0.0),
            (0, float(2 ** 21), -16.0, 96.0), (0, 500.0, 500.0, 32.0)]
    info = _explicit([dead + [(2, *whole)], [(0, *whole), (2, *whole)]], K)
    live = restate_amodal(o, packed.inst_label, packed.inst_model, V[0], P[0], info[0, 7:8], S, 3)[0]
    assert live.any()
    with Renderer(sc, W, H, max_frames=2) as r:
        assert r._n_inst_labels == 3
        r.set_instance_transforms(2, packed.inst_model)       # sets 0 and 2 uploaded, set 1 is a gap
        got = _amodal(r, fr, info, S)
    _same(got[0, 7], live, "the live slot next to the dead ones")
    for k in range(7):
        assert not got[0, k].any(), f"dead slot {k} {dead[k]}"
    assert not got[1].any(), "slots of a frame whose set was never uploaded"


def test_arguments(cone):
    from constructionsceneposeestimation_amd import _lib
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    W, H, S, K = 96, 64, 16, 2
    V, P = pose_frames([([0.0, -1.6, 0.4], [0.0, 0.0, 0.2])], W, H)
    fr = make_frames(V, P, [0], [0])
    info = _dev(_explicit([[(0, 0.0, -16.0, 96.0)]], K))
    out = _filled((1, K, S, S + 4))                           # (room for a misaligned pointer)
    lib = _lib.load()

    def call(ctx, n=1, **kw):
        a = dict(size=S, per_frame=K, frames=fr.ctypes.data, info=info.data_ptr(), crop_amodal=out.data_ptr())
        a.update(kw)
        job = _lib.AmodalJob(a["size"], a["per_frame"], a["frames"], a["info"], a["crop_amodal"])
        return lib.csg_crop_amodal(ctx, C.byref(job) if a.get("job", True) else None, n, None)

    with Renderer(cone, W, H, max_frames=1) as r:
        bad_set = make_frames(V, P, [1], [0])
        cases = dict(null_job=dict(job=False), null_frames=dict(frames=None), null_info=dict(info=None),
                     null_output=dict(crop_amodal=None), no_frames=dict(n=0), size_small=dict(size=12),
                     size_large=dict(size=516), size_odd=dict(size=18), k_zero=dict(per_frame=0),
                     k_large=dict(per_frame=65), misaligned=dict(crop_amodal=out.data_ptr() + 2),
                     set_not_resident=dict(frames=bad_set.ctypes.data))
        exact = dict(size_odd="crop_amodal: size 18 is not a multiple of 4 in 16..512",   # shared checks: whole text
                     k_large="crop_amodal: per_frame 65 outside 1..64",
                     set_not_resident="crop_amodal: frame 0: transform set 1 is not resident (1 sets)")
        for name, kw in cases.items():
            assert call(r.ctx, **kw) == -1, name
            msg = lib.csg_last_error(r.ctx).decode()
            assert msg.startswith("crop_amodal:"), (name, msg)
            if name in exact:
                assert msg == exact[name], name
        r.synchronize()
        assert (out.cpu().numpy() == FILL).all()              # nothing was enqueued
        assert call(r.ctx) == 0                               # the same call without a fault is accepted
        r.synchronize()
    got = out.cpu().numpy().reshape(-1)
    assert set(np.unique(got[:K * S * S]).tolist()) == {0, 255} and (got[K * S * S:] == FILL).all()
    fresh = _filled((1, K, S, S))
    cfg = _lib.Config(0, W, H, 1, 0.5, 250.0, 0, 0, 0)
    ctx = C.c_void_p()
    assert lib.csg_create(C.byref(cfg), C.byref(ctx)) == 0
    try:
        assert call(ctx, crop_amodal=fresh.data_ptr()) == -1  # no scene uploaded
        assert "no scene" in lib.csg_last_error(ctx).decode()
    finally:
        lib.csg_destroy(ctx)
    assert (fresh.cpu().numpy() == FILL).all()
