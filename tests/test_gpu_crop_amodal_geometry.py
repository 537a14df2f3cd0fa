"""csg_crop_amodal_geometry on the GPU: mask bytes, depth bits and object
coordinates are exact against the restatement of
tests/test_crop_amodal_geometry.py (the CPU oracle renders the frame without
the other labels; the crops' restatement samples its depth and its coordinate
image) -- planned crops behind a render and the crops on one stream, one object
behind another, the near plane, a texture swap, sets and tables, dead slots,
each output alone, shared scratch and frame ranges, argument checks and the
host-delivery wrapper.  Outputs are prefilled with 7."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import pose_frames
from tests.test_crop_amodal import FIDS3, H3, K3, MINPX3, PAD3, S3, W3, c3_reference
from tests.test_crop_amodal_geometry import (amodal_render, bits, c3_geometry, frame_depth_at_samples,
                                             restate_amodal_geometry)
from tests.test_gpu_crop_amodal import _dev, _explicit, _filled, _two_cones
from tests.test_object_crops import INFO_DTYPE

pytestmark = pytest.mark.gpu
FILL = 7
TAIL = 64          # sentinel bytes kept behind every output
NAMES = ("crop_amodal", "crop_amodal_depth", "crop_amodal_coords")
ITEM = {"crop_amodal": (1, np.uint8), "crop_amodal_depth": (4, np.float32), "crop_amodal_coords": (6, np.uint16)}


def _outputs(n, K, S, names=NAMES):
    """Flat sentinel-filled device buffers, TAIL bytes longer than the arrays."""
    return {name: _filled((n * K * S * S * ITEM[name][0] + TAIL,)) for name in names}


def _host(bufs, n, K, S):
    """The arrays of ``bufs`` on the host; the bytes past each array still hold the sentinel."""
    out = {}
    for name, t in bufs.items():
        raw = t.cpu().numpy()
        size, dt = ITEM[name]
        assert (raw[-TAIL:] == FILL).all(), f"{name}: bytes past the array were written"
        a = raw[:-TAIL].view(dt)
        out[name] = a.reshape((n, K, S, S, 3) if name == "crop_amodal_coords" else (n, K, S, S))
    return out


def _geometry(r, fr, info, S, names=NAMES, stream=0):
    """crop_amodal_geometry of explicit windows ``info`` (n, K) -> the requested arrays on the host."""
    n, K = info.shape
    d_info, bufs = _dev(info), _outputs(n, K, S, names)
    r.crop_amodal_geometry(fr, size=S, per_frame=K, info=d_info.data_ptr(), stream=stream,
                           **{name: t.data_ptr() for name, t in bufs.items()})
    r.synchronize()
    assert d_info.cpu().numpy().tobytes() == info.tobytes(), "info was written"
    return _host(bufs, n, K, S)


def _same(got, exp, what, names=NAMES):
    """Mask bytes, depth bits and coordinates of ``got`` equal ``exp`` exactly."""
    for name in names:
        g, e = got[name], np.asarray(exp[name])
        assert g.dtype == e.dtype and g.shape == e.shape, (what, name)
        if name == "crop_amodal_depth":
            g, e = bits(g), bits(e)
        bad = np.argwhere(g != e)
        assert len(bad) == 0, f"{what}: {name}: {len(bad)} values differ, first at {bad[:4].tolist()}"


def _empty(got, what):
    for name, a in got.items():
        if name == "crop_amodal_depth":
            assert np.isposinf(a).all(), f"{what}: depth is not +inf"
        else:
            assert not a.any(), f"{what}: {name} is not zero"


def _stack(per_frame):
    return {name: np.stack([a[name] for a in per_frame]) for name in NAMES}


def _table(n_lab):
    """A hand-made object-frame table for scenes without objects: per label a
    world -> unit-box matrix that keeps the cones' surface strictly inside (0, 1)."""
    t = np.zeros((n_lab, 3, 4), np.float32)
    for L in range(n_lab):
        t[L] = [[0.31 + 0.02 * L, 0.01, 0.0, 0.5], [0.02, 0.11 + 0.01 * L, 0.0, 0.3], [0.0, 0.03, 0.7, 0.1]]
    return t


def _upload(r, wl, epochs, frames_too=True):
    for k, e in enumerate(epochs):
        st = wl.epoch(e)
        r.set_instance_transforms(k, st.models)
        if frames_too:
            r.set_object_frames(k, st.object_frames)


# -- behind the crops -------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [None, ("static",)])
def test_rendered_frames_behind_the_crops(kinds):
    """render -> crop_objects (planned, with depth and coordinates) -> crop_amodal_geometry on one stream."""
    import torch
    from constructionsceneposeestimation_amd.crops import hidden_mask
    from constructionsceneposeestimation_amd.renderer import Renderer
    ref, geo = c3_reference(kinds), c3_geometry(kinds)
    wl, fr, n = ref["wl"], ref["fr"], 3
    dev = torch.device("cuda", 0)
    with Renderer(wl.scene, W3, H3, max_frames=3) as r:
        assert r._n_inst_labels == ref["n_labels"] == r.n_labels
        _upload(r, wl, ref["epochs"])
        inst = torch.empty((n, H3, W3), dtype=torch.int32, device=dev)
        depth = torch.empty((n, H3, W3), dtype=torch.float32, device=dev)
        coords = torch.empty((n, H3, W3, 3), dtype=torch.int16, device=dev)
        stats = torch.empty((n, r.n_labels, 5), dtype=torch.int32, device=dev)
        mask, cdepth = _filled((n, K3, S3, S3)), _filled((n, K3, S3, S3, 4))
        ccoords, mask_only = _filled((n, K3, S3, S3, 6)), _filled((n, K3, S3, S3))
        info = _filled((n, K3, INFO_DTYPE.itemsize))
        bufs = _outputs(n, K3, S3)
        el = _dev(ref["elig"])
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        st = stream.cuda_stream
        r.render_into(fr.ctypes.data, n, False, instance=inst.data_ptr(), depth=depth.data_ptr(),
                      obj_coords=coords.data_ptr(), stats=stats.data_ptr(), stream=st)
        r.crop_objects(n, size=S3, per_frame=K3, min_pixels=MINPX3, pad=PAD3, instance=inst.data_ptr(),
                       depth=depth.data_ptr(), obj_coords=coords.data_ptr(), stats=stats.data_ptr(),
                       eligible=el.data_ptr(), crop_mask=mask.data_ptr(), crop_depth=cdepth.data_ptr(),
                       crop_coords=ccoords.data_ptr(), info=info.data_ptr(), stream=st)
        r.crop_amodal_geometry(fr, size=S3, per_frame=K3, info=info.data_ptr(), stream=st,
                               **{name: t.data_ptr() for name, t in bufs.items()})
        r.crop_amodal(fr, size=S3, per_frame=K3, info=info.data_ptr(), crop_amodal=mask_only.data_ptr(), stream=st)
        stream.synchronize()
        r.synchronize()
    got = _host(bufs, n, K3, S3)
    info = info.cpu().numpy().view(INFO_DTYPE).reshape(n, K3)
    mask, depth = mask.cpu().numpy(), depth.cpu().numpy()
    cdepth = cdepth.cpu().numpy().view(np.float32).reshape(n, K3, S3, S3)
    ccoords = ccoords.cpu().numpy().view(np.uint16).reshape(n, K3, S3, S3, 3)
    assert np.array_equal(inst.cpu().numpy(), ref["instance"])      # a difference here is the renderer's
    for name in INFO_DTYPE.names:                                   # planned, and untouched by the pass
        assert np.array_equal(np.ascontiguousarray(info[name]).view(np.uint32),
                              np.ascontiguousarray(ref["info"][name]).view(np.uint32)), name
    _same(got, geo, f"kinds {kinds}")
    assert np.array_equal(got["crop_amodal"], mask_only.cpu().numpy()), "the mask is not csg_crop_amodal's"
    # the consequences, against the GPU's own crops and rendered depth
    vis = mask == 255
    assert np.array_equal(mask, geo["crop_mask"]) and vis.sum() >= 5000
    assert np.array_equal(bits(got["crop_amodal_depth"])[vis], bits(cdepth)[vis])
    assert np.array_equal(got["crop_amodal_coords"][vis], ccoords[vis])
    hidden = hidden_mask(mask, got["crop_amodal"])
    assert hidden.sum() >= 500
    for f in range(n):
        at, inside = frame_depth_at_samples(info[f], S3, depth[f])
        assert inside[hidden[f]].all()
        assert (got["crop_amodal_depth"][f][hidden[f]] >= at[hidden[f]]).all(), f


# -- one object behind another ----------------------------------------------------------------------
def _cones_in_line(cone):
    from constructionsceneposeestimation_amd.scene.model import Instance, Scene
    sc = Scene(meshes=cone.meshes, materials=cone.materials, textures=cone.textures, light=cone.light)
    base = np.asarray(cone.instances[0].model, np.float64)
    for k in range(2):                                             # label 1 stands behind label 0
        m = base.copy()
        m[0, 3] += 0.15 * k
        m[1, 3] += 0.4 * k
        sc.instances.append(Instance(mesh=cone.instances[0].mesh, model=m, inst_idx=k))
    return sc


def test_one_object_behind_another(cone):
    """The rear cone, mostly hidden: minified (S = 16), at step 1 with an integer origin (S = 64) and
    magnified (S = 512: the largest key image)."""
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from oracle.oracle import Oracle
    sc = _cones_in_line(cone)
    W, H = 160, 96
    V, P = pose_frames([([0.0, -1.0, 0.35], [0.0, 0.0, 0.2])], W, H)
    fr = make_frames(V, P, [0], [0])
    packed = pack_scene(sc)
    o = Oracle(packed, W, H)
    full = o.render(V[0], P[0])
    rear = amodal_render(o, packed.inst_label, packed.inst_model, V[0], P[0], 1)
    amodal, visible = rear["instance"] == 1, full["instance"] == 1
    print("rear cone: amodal", int(amodal.sum()), "visible", int(visible.sum()))
    assert amodal.sum() >= 500 and (amodal & ~visible).sum() >= amodal.sum() / 4
    ys, xs = np.nonzero(amodal)
    assert 57 <= xs.min() and xs.max() < 121 and 9 <= ys.min() and ys.max() < 73
    table = _table(2)
    windows = {16: (56.0, 8.0, 64.0), 64: (57.0, 9.0, 64.0), 512: (65.0, 17.0, 48.0)}
    with Renderer(sc, W, H, max_frames=1) as r:
        r.set_object_frames(0, table)
        got = {S: _geometry(r, fr, _explicit([[(1, *win), (0, *win)]], 2), S) for S, win in windows.items()}
    for S, win in windows.items():
        info = _explicit([[(1, *win), (0, *win)]], 2)
        exp = restate_amodal_geometry(o, packed.inst_label, packed.inst_model, V[0], P[0], info[0], S, 2, table)
        assert exp["crop_amodal"][0].any() and exp["crop_amodal_coords"][0].any()
        _same({k: a[0] for k, a in got[S].items()}, exp, f"S = {S}")
    # step 1: the depth crop is the single-object depth window, copied
    assert np.array_equal(bits(got[64]["crop_amodal_depth"][0, 0]), bits(rear["depth"][9:73, 57:121]))
    hid = (amodal & ~visible)[9:73, 57:121]
    assert (got[64]["crop_amodal_depth"][0, 0][hid] >= full["depth"][9:73, 57:121][hid]).all()


# -- near plane --------------------------------------------------------------------------------------
def test_near_plane(cone):
    """The cone cut by the near plane (0.5): the sub-triangles of the near-clip fan share the original
    triangle's 1/W plane; depth bits exact at step 1, minified and magnified."""
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from oracle.oracle import Oracle
    W, H = 96, 64
    V, P = pose_frames([([0.3, -0.55, 0.25], [0.0, 0.0, 0.25]), ([0.0, -0.6, 0.3], [0.0, 0.0, 0.2])], W, H)
    fr = make_frames(V, P, [0, 0], [0, 1])
    packed = pack_scene(cone)
    o = Oracle(packed, W, H)
    L = int(packed.inst_label[0])
    n_lab = L + 1
    refs = [o.render(V[k], P[k]) for k in range(2)]
    for ref in refs:
        assert ref["depth"][ref["instance"] >= 0].min() < 0.501    # the surface reaches the near plane
    info = _explicit([[(L, 0.0, -16.0, 96.0)]] * 2, 1)
    table = _table(n_lab)
    with Renderer(cone, W, H, max_frames=2) as r:
        assert r._n_inst_labels == n_lab
        r.set_object_frames(0, table)
        got = {S: _geometry(r, fr, info, S) for S in (96, 16, 512)}
    for S, g in got.items():
        exp = _stack([restate_amodal_geometry(o, packed.inst_label, packed.inst_model, V[k], P[k], info[k], S, n_lab,
                                              table) for k in range(2)])
        assert exp["crop_amodal"].any() and not exp["crop_amodal"].all()
        _same(g, exp, f"near plane: S = {S}")
    for k in range(2):                                             # step 1: the window copies the frame
        win = np.full((96, 96), np.inf, np.float32)
        win[16:16 + H] = refs[k]["depth"]
        assert np.array_equal(bits(got[96]["crop_amodal_depth"][k, 0]), bits(win))


# -- texture swap ------------------------------------------------------------------------------------
def test_texture_swap():
    """Tree label 28 of frame 4 under set 0 (the scene's textures) and set 1 (material 3 without its
    texture): where the alpha test no longer cuts the foliage, nearer fragments win."""
    from constructionsceneposeestimation_amd import _lib
    from constructionsceneposeestimation_amd.labels import object_unit_transforms
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from oracle.oracle import Oracle
    ref = c3_reference(None)
    wl, L, S = ref["wl"], 28, 64
    V, P = ref["V"][[0, 0]], ref["P"][[0, 0]]
    fr = make_frames(V, P, [0, 1], [4, 4])
    packed = pack_scene(wl.scene)
    o = Oracle(packed, W3, H3)
    st = wl.epoch(0)
    models = np.asarray(st.models, np.float32).reshape(-1, 16)
    table = object_unit_transforms(wl.scene, st.object_frames)
    swap = [_lib.KEEP_TEXTURE] * len(packed.materials)
    swap[3] = -1
    ys, xs = np.nonzero(amodal_render(o, packed.inst_label, models, V[0], P[0], L, swap)["instance"] == L)
    side = float(max(xs.max() - xs.min(), ys.max() - ys.min()) + 1) * 1.25
    box = (L, (xs.min() + xs.max() + 1) / 2 - side / 2, (ys.min() + ys.max() + 1) / 2 - side / 2, side)
    info = _explicit([[box], [box]], 1)
    exp = _stack([restate_amodal_geometry(o, packed.inst_label, models, V[0], P[0], info[k], S, ref["n_labels"],
                                          table, t) for k, t in enumerate((None, swap))])
    both = (exp["crop_amodal"][0] == 255) & (exp["crop_amodal"][1] == 255)
    differ = both & (bits(exp["crop_amodal_depth"][0]) != bits(exp["crop_amodal_depth"][1]))
    print("samples on the object in both sets", int(both.sum()), "of them with another depth", int(differ.sum()))
    assert differ.sum() >= 20
    with Renderer(wl.scene, W3, H3, max_frames=2) as r:
        for k in range(2):
            r.set_instance_transforms(k, models)
            r.set_object_frames(k, st.object_frames)
        r.set_dr_textures(1, swap)
        got = _geometry(r, fr, info, S)
    assert (bits(got["crop_amodal_depth"][0]) != bits(got["crop_amodal_depth"][1])).any()
    _same({k: a[0] for k, a in got.items()}, {k: a[0] for k, a in exp.items()}, "set 0: the scene's textures")
    _same({k: a[1] for k, a in got.items()}, {k: a[1] for k, a in exp.items()}, "set 1: material 3 without texture")


# -- sets, tables and dead slots ---------------------------------------------------------------------
def test_sets_tables_and_dead_slots(cone):
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from oracle.oracle import Oracle
    sc = _two_cones(cone)                                           # labels 0 and 2
    W, H, S, K = 96, 64, 16, 8
    V, P = pose_frames([([0.0, -1.6, 0.4], [0.0, 0.0, 0.2])] * 3, W, H)
    fr = make_frames(V, P, [0, 1, 2], [0, 1, 2])     # set 1 is in range and never uploaded, set 2 has no table
    packed = pack_scene(sc)
    o = Oracle(packed, W, H)
    whole = (0.0, -16.0, 96.0)
    dead = [(-1, *whole), (3, *whole), (1, *whole), (0, 0.0, -16.0, np.nan), (0, 0.0, -16.0, 0.0),
            (0, float(2 ** 21), -16.0, 96.0), (0, 500.0, 500.0, 32.0)]
    info = _explicit([dead + [(2, *whole)], [(0, *whole), (2, *whole)], [(0, *whole), (2, *whole)]], K)
    table = _table(3)
    live = restate_amodal_geometry(o, packed.inst_label, packed.inst_model, V[0], P[0], info[0, 7:8], S, 3, table)
    bare = restate_amodal_geometry(o, packed.inst_label, packed.inst_model, V[2], P[2], info[2], S, 3, None)
    assert live["crop_amodal"].any() and live["crop_amodal_coords"].any()
    assert bare["crop_amodal"][0].any() and bare["crop_amodal"][1].any() and not bare["crop_amodal_coords"].any()
    with Renderer(sc, W, H, max_frames=3) as r:
        assert r._n_inst_labels == 3
        r.set_instance_transforms(2, packed.inst_model)            # sets 0 and 2 uploaded, set 1 is a gap
        r.set_object_frames(0, table)                              # only set 0 has a table
        got = _geometry(r, fr, info, S)
    _same({k: a[0, 7:8] for k, a in got.items()}, live, "the live slot next to the dead ones")
    for k in range(7):
        _empty({name: a[0, k] for name, a in got.items()}, f"dead slot {k} {dead[k]}")
    _empty({name: a[1] for name, a in got.items()}, "slots of a frame whose set was never uploaded")
    assert np.isfinite(got["crop_amodal_depth"][2, :2]).any()
    _same({k: a[2] for k, a in got.items()}, bare, "a set with transforms and no table")
    assert not got["crop_amodal_coords"][2].any()


# -- each output alone -------------------------------------------------------------------------------
def test_each_output_alone():
    """Depth alone (its buffer is the key image), coordinates alone and mask alone (scratch keys), and
    mask with coordinates, equal the outputs of the call with all three."""
    from constructionsceneposeestimation_amd.renderer import Renderer
    ref, geo = c3_reference(None), c3_geometry(None)
    wl = ref["wl"]
    with Renderer(wl.scene, W3, H3, max_frames=3) as r:
        _upload(r, wl, ref["epochs"])
        every = _geometry(r, ref["fr"], ref["info"], S3)
        some = [_geometry(r, ref["fr"], ref["info"], S3, names) for names in
                [("crop_amodal_depth",), ("crop_amodal_coords",), ("crop_amodal",),
                 ("crop_amodal", "crop_amodal_coords")]]
    _same(every, geo, "all three outputs")
    for got in some:
        assert got
        _same(got, every, f"outputs {sorted(got)} alone", tuple(got))


# -- shared scratch and frame ranges -----------------------------------------------------------------
def test_back_to_back_on_two_streams_with_reused_frame_records():
    """Two passes share the pass's scratch keys: the second, on another stream, waits for the first on
    the device, and the caller's frame records may be overwritten as soon as a call returns."""
    import torch
    from constructionsceneposeestimation_amd.renderer import Renderer
    ref, geo = c3_reference(None), c3_geometry(None)
    wl, dev = ref["wl"], torch.device("cuda", 0)
    info = _dev(ref["info"])
    names = ("crop_amodal", "crop_amodal_coords")                   # no depth output: both use the scratch
    first, second = _outputs(3, K3, S3, names), _outputs(1, K3, S3, names)
    with Renderer(wl.scene, W3, H3, max_frames=3) as r:
        _upload(r, wl, ref["epochs"])
        r.synchronize()
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        fr = ref["fr"].copy()
        r.crop_amodal_geometry(fr, size=S3, per_frame=K3, info=info.data_ptr(),
                               **{k: t.data_ptr() for k, t in first.items()})
        fr[:] = fr[[2, 0, 1]]                                       # frame 2's record now stands first
        r.crop_amodal_geometry(fr[:1], size=S3, per_frame=K3, info=info[2:].data_ptr(), stream=stream.cuda_stream,
                               **{k: t.data_ptr() for k, t in second.items()})
        fr.view(np.uint8)[:] = 0
        stream.synchronize()
        r.synchronize()
    _same(_host(first, 3, K3, S3), geo, "first pass, the context's stream", names)
    _same(_host(second, 1, K3, S3), {k: geo[k][2:] for k in names}, "second pass, another stream", names)


def test_frame_ranges_under_a_small_scratch_cap(monkeypatch):
    """A cap of one frame's keys (CSG_AMODAL_KEY_CAP, bytes) runs the three frames as three ranges."""
    from constructionsceneposeestimation_amd.renderer import Renderer
    ref, geo = c3_reference(None), c3_geometry(None)
    wl = ref["wl"]
    names = ("crop_amodal", "crop_amodal_coords")
    monkeypatch.setenv("CSG_AMODAL_KEY_CAP", str(K3 * S3 * S3 * 4))
    with Renderer(wl.scene, W3, H3, max_frames=3) as r:
        _upload(r, wl, ref["epochs"])
        got = _geometry(r, ref["fr"], ref["info"], S3, names)
        monkeypatch.setenv("CSG_AMODAL_KEY_CAP", str(2 * K3 * S3 * S3 * 4 + 100))   # ranges of 2 + 1
        two = _geometry(r, ref["fr"], ref["info"], S3, names)
    _same(got, geo, "three ranges of one frame", names)
    _same(two, geo, "ranges of two frames and one", names)


# -- arguments ---------------------------------------------------------------------------------------
def test_arguments(cone):
    from constructionsceneposeestimation_amd import _lib
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    W, H, S, K = 96, 64, 16, 2
    V, P = pose_frames([([0.0, -1.6, 0.4], [0.0, 0.0, 0.2])], W, H)
    fr = make_frames(V, P, [0], [0])
    info = _dev(_explicit([[(0, 0.0, -16.0, 96.0)]], K))
    bufs = _outputs(1, K, S)
    lib = _lib.load()
    good = dict(size=S, per_frame=K, frames=fr.ctypes.data, info=info.data_ptr(),
                **{name: t.data_ptr() for name, t in bufs.items()})

    def call(ctx, n=1, job=True, **kw):
        a = dict(good)
        a.update(kw)
        j = _lib.AmodalGeometryJob(a["size"], a["per_frame"], a["frames"], a["info"], a["crop_amodal"],
                                   a["crop_amodal_depth"], a["crop_amodal_coords"])
        return lib.csg_crop_amodal_geometry(ctx, C.byref(j) if job else None, n, None)

    with Renderer(cone, W, H, max_frames=1) as r:
        bad_set = make_frames(V, P, [1], [0])
        cases = dict(null_job=dict(job=False), null_frames=dict(frames=None), null_info=dict(info=None),
                     no_outputs=dict(crop_amodal=None, crop_amodal_depth=None, crop_amodal_coords=None),
                     no_frames=dict(n=0), size_small=dict(size=12), size_large=dict(size=516), size_odd=dict(size=18),
                     k_zero=dict(per_frame=0), k_large=dict(per_frame=65),
                     mask_misaligned=dict(crop_amodal=good["crop_amodal"] + 2),
                     depth_misaligned=dict(crop_amodal_depth=good["crop_amodal_depth"] + 8),
                     coords_misaligned=dict(crop_amodal_coords=good["crop_amodal_coords"] + 4),
                     set_not_resident=dict(frames=bad_set.ctypes.data))
        exact = dict(size_odd="crop_amodal_geometry: size 18 is not a multiple of 4 in 16..512",   # shared checks
                     k_large="crop_amodal_geometry: per_frame 65 outside 1..64",
                     set_not_resident="crop_amodal_geometry: frame 0: transform set 1 is not resident (1 sets)")
        for name, kw in cases.items():
            assert call(r.ctx, **kw) == -1, name
            msg = lib.csg_last_error(r.ctx).decode()
            assert msg.startswith("crop_amodal_geometry:"), (name, msg)
            if name in exact:
                assert msg == exact[name], name
        r.synchronize()
        for name, t in bufs.items():
            assert (t.cpu().numpy() == FILL).all(), f"{name} was written by a refused call"
        assert call(r.ctx) == 0                                     # the same call without a fault is accepted
        r.synchronize()
    got = _host(bufs, 1, K, S)
    assert set(np.unique(got["crop_amodal"]).tolist()) == {0, 255}
    assert np.isfinite(got["crop_amodal_depth"][got["crop_amodal"] == 255]).all()
    fresh = _outputs(1, K, S)
    cfg = _lib.Config(0, W, H, 1, 0.5, 250.0, 0, 0, 0)
    ctx = C.c_void_p()
    assert lib.csg_create(C.byref(cfg), C.byref(ctx)) == 0
    try:
        assert call(ctx, **{name: t.data_ptr() for name, t in fresh.items()}) == -1   # no scene uploaded
        msg = lib.csg_last_error(ctx).decode()
        assert msg.startswith("crop_amodal_geometry:") and "no scene" in msg
    finally:
        lib.csg_destroy(ctx)
    for t in fresh.values():
        assert (t.cpu().numpy() == FILL).all()


# -- render_crops ------------------------------------------------------------------------------------
def test_render_crops_delivers_the_geometry():
    """n = 3 with max_frames = 2: two chunks, one geometry pass behind the crops of each."""
    from constructionsceneposeestimation_amd.renderer import Renderer
    ref, geo = c3_reference(None), c3_geometry(None)
    wl = ref["wl"]
    with Renderer(wl.scene, W3, H3, max_frames=2) as r:
        _upload(r, wl, ref["epochs"])
        got = r.render_crops(ref["fr"], size=S3, per_frame=K3, min_pixels=MINPX3, pad=PAD3,
                             want=("mask", "amodal", "amodal_depth", "amodal_coords"))
        old = r.render_crops(ref["fr"], size=S3, per_frame=K3, min_pixels=MINPX3, pad=PAD3,
                             want=("rgb", "mask", "amodal"))
        with pytest.raises(Exception, match="amodal_depth, amodal_coords"):
            r.render_crops(ref["fr"], size=S3, per_frame=K3, want=("amodal_normals",))
    assert set(got) == {"crop_mask", "crop_amodal", "crop_amodal_depth", "crop_amodal_coords", "info", "intrinsics"}
    assert np.array_equal(got["info"]["label"], ref["info"]["label"])
    assert np.array_equal(got["crop_mask"], ref["crop_mask"])
    _same(got, geo, "render_crops: geometry")
    assert set(old) == {"crop_rgb", "crop_mask", "crop_amodal", "info", "intrinsics"}
    assert np.array_equal(old["crop_mask"], ref["crop_mask"]) and np.array_equal(old["crop_amodal"], ref["crop_amodal"])
