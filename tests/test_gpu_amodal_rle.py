"""csg_amodal_spans on the GPU: offsets, spans and stats are bit-exact against
the restatement of tests/test_amodal_rle.py (the CPU oracle renders the frame
without the other labels, the span restatement of tests/test_mask_rle.py walks
it) -- the three C3 reference frames, frame ranges, overflow, small shapes with a
frame-filling triangle and the near plane, eligible subsets, the crop pass as a
second opinion, argument checks, streams, and the generator's ``amodal_rle``
output.  Outputs are prefilled with 7 and followed by a guard."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.conftest import pose_frames
from tests.test_amodal_rle import EMPTY, amodal_reference, restate_amodal_spans
from tests.test_crop_amodal import H3, W3, amodal_image
from tests.test_object_crops import INFO_DTYPE

pytestmark = pytest.mark.gpu
FILL = 0x07070707
GUARD = 256          # records (and words) behind the outputs that must stay untouched


def _filled(shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.int32, device=torch.device("cuda", 0))


def _enqueue(r, fr, cap, eligible=None, stream=0, stats=True):
    n, L = len(fr), r._n_inst_labels
    d_sp, d_off = _filled((n * cap + GUARD, 2)), _filled((n * (L + 1) + GUARD,))
    d_st = _filled((n * L * 5 + GUARD,)) if stats else None
    r.amodal_spans(fr, spans=d_sp.data_ptr(), span_offsets=d_off.data_ptr(), capacity=cap,
                   amodal_stats=d_st.data_ptr() if stats else 0, eligible=eligible, stream=stream)
    return d_sp, d_off, d_st


def _fetch(bufs, n, L, cap):
    d_sp, d_off, d_st = bufs
    sp, off = d_sp.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint32)
    st = d_st.cpu().numpy().view(np.uint32) if d_st is not None else None
    assert (sp[n * cap:] == FILL).all(), "the guard behind spans was written"
    assert (off[n * (L + 1):] == FILL).all(), "the guard behind span_offsets was written"
    if st is not None:
        assert (st[n * L * 5:] == FILL).all(), "the guard behind amodal_stats was written"
        st = st[:n * L * 5].reshape(n, L, 5)
    return off[:n * (L + 1)].reshape(n, L + 1), sp[:n * cap].reshape(n, cap, 2), st


def _run(r, fr, cap, **kw):
    """The pass on the context's stream -> (offsets (n, L + 1), spans (n, cap, 2), stats (n, L, 5)) as uint32."""
    bufs = _enqueue(r, fr, cap, **kw)
    r.synchronize()
    return _fetch(bufs, len(fr), r._n_inst_labels, cap)


def _check(got, refs, cap, what):
    off, sp, st = got
    for f, (r_off, r_sp, r_st) in enumerate(refs):
        assert np.array_equal(off[f], r_off), f"{what}: frame {f} offsets {off[f].tolist()} != {r_off.tolist()}"
        if st is not None:
            bad = np.argwhere((st[f] != r_st).any(1)).ravel()
            assert len(bad) == 0, f"{what}: frame {f} stats of labels {bad.tolist()}: {st[f][bad].tolist()} != " \
                                  f"{r_st[bad].tolist()}"
        total = int(r_off[-1])
        if total <= cap:          # a frame that fits is exact, and nothing beyond its total is touched
            bad = np.argwhere((sp[f, :total] != r_sp).any(1)).ravel()
            assert len(bad) == 0, f"{what}: frame {f}: {len(bad)} of {total} spans differ, first at {bad[:4].tolist()}"
            assert (sp[f, total:] == FILL).all(), f"{what}: frame {f} wrote beyond its total"


def _decode(off, sp, l, H, W):
    from constructionsceneposeestimation_amd import masks
    return masks.spans_to_mask((H, W), masks.label_spans(sp, off, l))


@pytest.fixture(scope="module")
def c3():
    """One context on the C3 reference frames for the module, with the all-labels job run once."""
    from constructionsceneposeestimation_amd.renderer import Renderer
    am = amodal_reference()
    ref = am["ref"]
    wl = ref["wl"]
    top = max(int(o[-1]) for o, _, _ in am["frames"])
    cap = top + 64
    with Renderer(wl.scene, W3, H3, max_frames=3) as r:
        assert r._n_inst_labels == am["L"] == r.n_labels
        for k, e in enumerate(ref["epochs"]):
            r.set_instance_transforms(k, wl.epoch(e).models)
        base = _run(r, ref["fr"], cap)
        yield dict(r=r, am=am, ref=ref, fr=ref["fr"], L=am["L"], cap=cap, top=top, base=base)


def test_reference_frames_all_labels(c3):
    import torch
    am, L, r = c3["am"], c3["L"], c3["r"]
    print("spans per frame", [int(o[-1]) for o, _, _ in am["frames"]], "capacity", c3["cap"])
    assert all(int(o[-1]) > 100 for o, _, _ in am["frames"])
    _check(c3["base"], am["frames"], c3["cap"], "C3 frames, all labels")
    off, sp, st = c3["base"]
    inst = torch.empty((3, H3, W3), dtype=torch.int32, device="cuda")
    r.render_into(c3["fr"].ctypes.data, 3, False, instance=inst.data_ptr())
    r.synchronize()
    ids = inst.cpu().numpy()
    assert np.array_equal(ids, c3["ref"]["instance"])           # a difference here is the renderer's
    for f in range(3):
        for l in range(L):
            s = sp[f, int(off[f, l]):int(off[f, l + 1])]
            assert int(s[:, 1].sum()) == int(st[f, l, 0]), (f, l)
            vis = ids[f] == l
            if vis.any():                                       # every visible pixel lies in the amodal mask
                assert not (vis & ~_decode(off[f], sp[f], l, H3, W3)).any(), (f, l)


def test_frame_ranges_give_the_same_bytes(c3, monkeypatch):
    """The scratch bound lowered so that three frames take two ranges (two frames fit), then three."""
    per_frame = c3["L"] * ((H3 + 31) // 32) * W3 * 4            # bytes of one frame's planes, all labels
    for bound in (2 * per_frame + 100, 1):
        monkeypatch.setenv("CSG_AMODAL_PLANE_CAP", str(bound))
        got = _run(c3["r"], c3["fr"], c3["cap"])
        for a, b in zip(got, c3["base"]):
            assert np.array_equal(a, b), f"plane bound {bound}"


def test_overflow_reports_the_true_total(c3):
    am = c3["am"]
    cap = c3["top"] - 1
    full = [int(o[-1]) > cap for o, _, _ in am["frames"]]
    assert any(full) and not all(full)
    _check(_run(c3["r"], c3["fr"], cap), am["frames"], cap, f"C = {cap}")


def test_eligible_subsets(c3):
    am, L, r = c3["am"], c3["L"], c3["r"]
    present = [l for l in range(L) if any(int(st[l, 0]) for _, _, st in am["frames"])]
    assert len(present) >= 6
    chosen = np.zeros(L, np.uint8)
    chosen[present[1::2]] = 1
    chosen[[l for l in range(L) if l not in present][:1]] = 1   # ... and one label that is nowhere
    want = [restate_amodal_spans({l: img for l, img in am["images"][k].items() if chosen[l]}, L, (H3, W3))
            for k in range(3)]
    assert all(0 < int(w[0][-1]) < int(a[0][-1]) for w, a in zip(want, am["frames"]))
    got = _run(r, c3["fr"], c3["cap"], eligible=chosen)
    _check(got, want, c3["cap"], "a strict subset")
    off, sp, st = got
    b_off, b_sp, b_st = c3["base"]
    for f in range(3):
        for l in range(L):
            mine = sp[f, int(off[f, l]):int(off[f, l + 1])]
            if chosen[l]:                                       # exactly as in the all-labels job
                assert np.array_equal(mine, b_sp[f, int(b_off[f, l]):int(b_off[f, l + 1])]), (f, l)
                assert np.array_equal(st[f, l], b_st[f, l]), (f, l)
            else:
                assert len(mine) == 0 and tuple(st[f, l].tolist()) == EMPTY, (f, l)
    none = [restate_amodal_spans({}, L, (H3, W3))] * 3
    _check(_run(r, c3["fr"], c3["cap"], eligible=np.zeros(L, np.uint8)), none, c3["cap"], "no label eligible")
    _check(_run(r, c3["fr"], 1, eligible=np.zeros(L, np.uint8), stats=False), none, 1, "no label, no stats")


def test_crop_pass_agrees(c3):
    """No oracle involved: csg_crop_amodal on windows with integer corners and side == S (step 1, inside the
    frame) writes the decoded full-frame mask cut at the window."""
    import torch
    r, L, S, K = c3["r"], c3["L"], 64, 4
    off, sp, st = c3["base"]
    info = np.zeros((3, K), INFO_DTYPE)
    info["label"] = -1
    want = np.zeros((3, K, S, S), np.uint8)
    for f in range(3):
        labels = np.argsort(-st[f, :, 0].astype(np.int64), kind="stable")[:K]
        for k, l in enumerate(labels):
            px, x0, y0, x1, y1 = (int(v) for v in st[f, l])
            assert px > 0
            wx = min(max((x0 + x1) // 2 - S // 2, 0), W3 - S)   # centred on the amodal box, kept inside the frame
            wy = min(max((y0 + y1) // 2 - S // 2, 0), H3 - S)
            info[f, k] = (int(l), 0, float(wx), float(wy), float(S), f, (0, 0))
            want[f, k] = _decode(off[f], sp[f], int(l), H3, W3)[wy:wy + S, wx:wx + S] * 255
    assert want.any() and not want.all()
    d_info = torch.from_numpy(info.view(np.uint8).reshape(3, K, -1).copy()).to("cuda")
    out = torch.full((3, K, S, S), 7, dtype=torch.uint8, device="cuda")
    r.crop_amodal(c3["fr"], size=S, per_frame=K, info=d_info.data_ptr(), crop_amodal=out.data_ptr())
    r.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_behind_a_render_and_beside_one(c3):
    """On the render's stream with nothing in between, then on a second stream while the context's renders."""
    import torch
    r, fr, cap, L = c3["r"], c3["fr"], c3["cap"], c3["L"]
    dev = torch.device("cuda", 0)
    inst = torch.empty((3, H3, W3), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    r.render_into(fr.ctypes.data, 3, False, instance=inst.data_ptr(), stream=stream.cuda_stream)
    behind = _enqueue(r, fr, cap, stream=stream.cuda_stream)
    stream.synchronize()
    r.synchronize()
    other = torch.cuda.Stream(dev)
    other.wait_stream(torch.cuda.current_stream(dev))
    r.render_into(fr.ctypes.data, 3, False, instance=inst.data_ptr())          # the context's stream
    beside = _enqueue(r, fr, cap, stream=other.cuda_stream)
    again = _enqueue(r, fr[[2, 0, 1]], cap)                                    # a pass on another stream right behind it
    other.synchronize()
    r.synchronize()
    assert np.array_equal(inst.cpu().numpy(), c3["ref"]["instance"])
    for what, bufs in (("behind a render", behind), ("beside a render", beside)):
        for a, b in zip(_fetch(bufs, 3, L, cap), c3["base"]):
            assert np.array_equal(a, b), what
    for a, b in zip(_fetch(again, 3, L, cap), c3["base"]):
        assert np.array_equal(a, b[[2, 0, 1]]), "frames in another order, on the context's stream"


def test_three_amodal_passes_back_to_back_on_two_streams(cone):
    """crop_amodal on the context's stream, amodal_spans on a second stream and crop_amodal_geometry on the
    context's stream again, with nothing in between but the caller overwriting its frame records as soon as
    each call returns: the three share the device frame records, their staging and one order.  Each result
    is what the same call gives alone and synchronized (pinned to the oracle by each pass's own tests)."""
    import torch
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from tests.test_gpu_crop_amodal import _dev, _explicit
    W, H, S, K, cap = 96, 64, 16, 2, 512
    dev = torch.device("cuda", 0)
    V, P = pose_frames([([0.0, -1.6, 0.4], [0.0, 0.0, 0.2]), ([1.1, -1.2, 0.7], [0.0, 0.0, 0.2])], W, H)
    fr = make_frames(V, P, [0, 0], [0, 1])
    jobs = [fr, fr[::-1].copy(), fr]                             # the second pass sees the frames swapped
    info = _dev(_explicit([[(0, 0.0, -16.0, 96.0)]] * 2, K))

    def outputs():
        return dict(mask=torch.full((2, K, S, S), 7, dtype=torch.uint8, device=dev),
                    spans=_filled((2 * cap + GUARD, 2)), off=_filled((2 * 2 + GUARD,)), stats=_filled((2 * 5 + GUARD,)),
                    g_mask=torch.full((2, K, S, S), 7, dtype=torch.uint8, device=dev),
                    g_depth=torch.full((2, K, S, S), 7.0, dtype=torch.float32, device=dev))

    def enqueue(r, k, o, frames, stream):
        if k == 0:
            r.crop_amodal(frames, size=S, per_frame=K, info=info.data_ptr(), crop_amodal=o["mask"].data_ptr(),
                          stream=stream)
        elif k == 1:
            r.amodal_spans(frames, spans=o["spans"].data_ptr(), span_offsets=o["off"].data_ptr(), capacity=cap,
                           amodal_stats=o["stats"].data_ptr(), stream=stream)
        else:
            r.crop_amodal_geometry(frames, size=S, per_frame=K, info=info.data_ptr(), stream=stream,
                                   crop_amodal=o["g_mask"].data_ptr(), crop_amodal_depth=o["g_depth"].data_ptr())

    with Renderer(cone, W, H, max_frames=2) as r:
        side = torch.cuda.Stream(dev)
        got, alone = outputs(), outputs()
        torch.cuda.synchronize(dev)                              # the prefill is in place
        for k in range(3):
            work = jobs[k].copy()
            enqueue(r, k, got, work, side.cuda_stream if k == 1 else 0)
            work.view(np.uint8)[:] = 0xFF                        # the caller's records are its own again
        side.synchronize()
        r.synchronize()
        for k in range(3):
            enqueue(r, k, alone, jobs[k].copy(), 0)
            r.synchronize()
        got, alone = ({k: t.cpu().numpy() for k, t in o.items()} for o in (got, alone))
    for name in got:
        assert got[name].tobytes() == alone[name].tobytes(), name
    off = got["off"].view(np.uint32)[:4].reshape(2, 2)
    assert (off[:, 1] > 0).all() and (got["mask"][:, 0] == 255).any((1, 2)).all()
    assert not np.array_equal(got["mask"][0], got["mask"][1])    # two different views: a swap would show
    assert np.array_equal(got["g_mask"], got["mask"])


def test_host_delivery_grows_the_capacity(c3):
    am, L = c3["am"], c3["L"]
    frames, stats, cap = c3["r"].amodal_spans_host(c3["fr"], capacity=1)
    assert cap >= c3["top"] and len(frames) == 3 and stats.shape == (3, L, 5) and stats.dtype == np.uint32
    for (off, sp), (r_off, r_sp, r_st), st in zip(frames, am["frames"], stats):
        assert off.dtype == np.uint32 and sp.dtype == np.uint32
        assert np.array_equal(off, r_off) and np.array_equal(sp, r_sp) and np.array_equal(st, r_st)


# -- small shapes ------------------------------------------------------------------------------------
BIG = np.diag([1.0, 1.0, 1.0, 1.0]).astype(np.float32).reshape(1, 16)   # the cone 52 m wide: its base fills the view
CLOSE = ([10.126, 9.784, 1.115], [10.2, 9.8, 0.115])                    # 1 m above the base plate, looking down
CUT = ([0.3, -0.55, 0.25], [0.0, 0.0, 0.25])                            # the authored cone (0.01) cut by the near plane


def _frame_filling_triangles(cone, M, V, P, W, H, near=0.5):
    """Triangles in front of the near plane whose projection holds all four corners of the frame."""
    m = cone.meshes[0]
    pos = np.c_[np.asarray(m.positions, np.float64), np.ones(len(m.positions))] @ M.reshape(4, 4).astype(np.float64).T
    h = pos @ (P.astype(np.float64) @ V.astype(np.float64)).T
    n = 0
    for t in np.asarray(m.tris).reshape(-1, 3):
        q = h[t]
        if (q[:, 3] < near).any():
            continue
        xy = q[:, :2] / q[:, 3:4]
        inside = True
        for cx, cy in ((0, 0), (W, 0), (0, H), (W, H)):
            s = [(xy[(e + 1) % 3, 0] - xy[e, 0]) * (cy - xy[e, 1]) - (xy[(e + 1) % 3, 1] - xy[e, 1]) * (cx - xy[e, 0])
                 for e in range(3)]
            inside &= all(v > 0 for v in s) or all(v < 0 for v in s)
        n += inside
    return n


@pytest.mark.parametrize("H,W", [(31, 65), (33, 64), (64, 130)])
def test_small_shapes(cone, H, W):
    """A single partial word (31 rows), a word boundary at row 32, column-group boundaries at 64 and 128;
    a triangle that covers the whole frame (the queued path, every word of every column) in set 0 and the
    near plane cutting the cone (the clip fan) in set 1.  A context of its own per shape."""
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from oracle.oracle import Oracle
    packed = pack_scene(cone)
    small = np.asarray(packed.inst_model, np.float32).reshape(1, 16)
    V, P = pose_frames([CLOSE, CUT], W, H)
    fr = make_frames(V, P, [0, 1], [0, 1])
    o = Oracle(packed, W, H)
    imgs = [amodal_image(o, packed.inst_label, BIG, V[0], P[0], 0),
            amodal_image(o, packed.inst_label, small, V[1], P[1], 0)]
    assert imgs[0].all() and _frame_filling_triangles(cone, BIG, V[0], P[0], W, H) >= 1
    assert imgs[1].any() and not imgs[1].all()
    st = o.frame_state(models16=small)
    d = st.render(V[1], P[1])
    assert d["depth"][d["instance"] >= 0].min() < 0.501         # the surface reaches the near plane
    want = [restate_amodal_spans({0: img}, 1, (H, W)) for img in imgs]
    assert int(want[0][0][-1]) == W and want[0][2][0].tolist() == [W * H, 0, 0, W - 1, H - 1]
    cap = max(int(w[0][-1]) for w in want)
    with Renderer(cone, W, H, max_frames=2) as r:
        assert r._n_inst_labels == 1
        r.set_instance_transforms(0, BIG)
        r.set_instance_transforms(1, small)
        _check(_run(r, fr, cap), want, cap, f"{H} x {W}")
        _check(_run(r, fr[::-1].copy(), cap), want[::-1], cap, f"{H} x {W}, frames swapped")


def test_sets_and_argument_checks(cone):
    import torch
    from constructionsceneposeestimation_amd import _lib
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from tests.test_gpu_crop_amodal import _cones300
    W, H, cap = 96, 64, 512
    V, P = pose_frames([([0.0, -1.6, 0.4], [0.0, 0.0, 0.2])] * 2, W, H)
    packed = pack_scene(cone)
    INVALID, LIMIT_ERR = -1, -5
    with Renderer(cone, W, H, max_frames=2) as r:
        r.set_instance_transforms(2, packed.inst_model)          # sets 0 and 2 uploaded, set 1 is a gap
        off, sp, st = _run(r, make_frames(V, P, [2, 1], [0, 1]), cap)
        assert off[0, 1] > 0 and st[0, 0, 0] > 0                 # set 2 draws the cone ...
        assert off[1].tolist() == [0, 0] and tuple(st[1, 0].tolist()) == EMPTY   # ... the gap nothing
        assert (sp[1] == FILL).all()
        fr = make_frames(V, P, [0, 0], [0, 1])
        d_sp, d_off, d_st = _filled((2 * cap + 1, 2)), _filled((2 * 2 + 2,)), _filled((2 * 5 + 2,))
        ok = dict(capacity=cap, frames=fr.ctypes.data, eligible=None, spans=d_sp.data_ptr(),
                  span_offsets=d_off.data_ptr(), amodal_stats=d_st.data_ptr())

        def call(n=2, **kw):
            job = _lib.AmodalSpanJob(**dict(ok, **kw))
            return r.lib.csg_amodal_spans(r.ctx, C.byref(job), n, None)

        assert r.lib.csg_amodal_spans(r.ctx, None, 2, None) == INVALID
        assert call(n=0) == INVALID
        for name in ("frames", "spans", "span_offsets"):
            assert call(**{name: None}) == INVALID, name
        for kw in (dict(capacity=0), dict(spans=d_sp.data_ptr() + 4), dict(span_offsets=d_off.data_ptr() + 2),
                   dict(amodal_stats=d_st.data_ptr() + 2)):
            assert call(**kw) == INVALID, kw
        bad = make_frames(V, P, [0, 3], [0, 1])                  # three sets are resident: 3 is not
        assert call(frames=bad.ctypes.data) == INVALID
        assert b"not resident" in r.lib.csg_last_error(r.ctx)
        # the text of the check this entry point shares with the crop passes, byte for byte
        assert r.lib.csg_last_error(r.ctx) == b"amodal_spans: frame 1: transform set 3 is not resident (3 sets)"
        with pytest.raises(_lib.CsgError):
            r.amodal_spans(bad, spans=d_sp.data_ptr(), span_offsets=d_off.data_ptr(), capacity=cap)
        r.synchronize()
        for d in (d_sp, d_off, d_st):
            assert (d.cpu().numpy() == FILL).all()               # nothing was enqueued
        assert call() == 0                                       # ... and the job itself is fine
        r.synchronize()
        assert d_off.cpu().numpy().view(np.uint32)[:4].tolist()[0::2] == [0, 0] and d_off.cpu().numpy()[1] > 0
    # no scene uploaded: a bare context
    cfg = _lib.Config(0, W, H, 1, 0.5, 100.0, 0, 0, 0)
    ctx = C.c_void_p()
    lib = _lib.load()
    assert lib.csg_create(C.byref(cfg), C.byref(ctx)) == 0
    try:
        job = _lib.AmodalSpanJob(**ok)
        assert lib.csg_amodal_spans(ctx, C.byref(job), 2, None) == INVALID
        assert b"no scene" in lib.csg_last_error(ctx)
    finally:
        lib.csg_destroy(ctx)
    # more labels than the span limit
    with Renderer(_cones300(cone), W, H, max_frames=1) as r:
        assert r._n_inst_labels == 300
        big_off = _filled((302,))
        job = _lib.AmodalSpanJob(cap, fr.ctypes.data, None, d_sp.data_ptr(), big_off.data_ptr(), None)
        assert r.lib.csg_amodal_spans(r.ctx, C.byref(job), 1, None) == LIMIT_ERR
        assert b"CSG_SPAN_MAX_LABELS" in r.lib.csg_last_error(r.ctx)
        r.synchronize()
        assert (big_off.cpu().numpy() == FILL).all()
    torch.cuda.synchronize()


def test_generate_writes_amodal_annotations(tmp_path):
    from constructionsceneposeestimation_amd import masks
    from constructionsceneposeestimation_amd.generate import generate
    kw = dict(workload="C3", seed=2, batch=2, width=W3, height=H3, writers=2)
    outs = ("rgb", "mask_rle", "amodal_rle")
    full, plain, py = tmp_path / "full", tmp_path / "plain", tmp_path / "py"
    generate(str(full), [0, 1, 2, 3], outputs=outs, **kw)
    generate(str(plain), [0, 1, 2, 3], outputs=("rgb", "mask_rle"), **kw)
    generate(str(py), [0, 1, 2, 3], outputs=outs, writer_mode="process", **kw)  # fragments from masks.coco_fragment
    n_amodal = n_larger = 0
    for f in range(4):
        raw = open(masks.fragment_path(str(full), f), "rb").read()
        assert raw == open(masks.fragment_path(str(py), f), "rb").read(), f    # native and Python: the same bytes
        frag = json.loads(raw)
        assert masks.fragment_bytes(frag) == raw
        stripped = {"image": frag["image"],
                    "annotations": [{k: v for k, v in a.items() if not k.startswith("amodal_")}
                                    for a in frag["annotations"]]}
        # without amodal_rle the fragment is what it was: the same annotations, no new key
        assert masks.fragment_bytes(stripped) == open(masks.fragment_path(str(plain), f), "rb").read(), f
        for a in frag["annotations"]:
            if "amodal_segmentation" not in a:
                assert not any(k.startswith("amodal_") for k in a)
                continue
            keys = list(a)
            at = keys.index("segmentation")
            assert keys[at + 1:at + 4] == ["amodal_bbox", "amodal_area", "amodal_segmentation"]
            vis = masks.decode(a["segmentation"]["size"], a["segmentation"]["counts"])
            amo = masks.decode(a["amodal_segmentation"]["size"], a["amodal_segmentation"]["counts"])
            assert not (vis & ~amo).any() and a["amodal_area"] == int(amo.sum()) >= a["area"]
            ys, xs = np.nonzero(amo)
            assert a["amodal_bbox"] == [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1),
                                        int(ys.max() - ys.min() + 1)]
            n_amodal += 1
            n_larger += a["amodal_area"] > a["area"]
    print("annotations with amodal masks", n_amodal, "strictly larger", n_larger)
    assert n_amodal >= 4 and n_larger >= 1
    doc = json.load(open(masks.merge(str(full))))
    assert sum("amodal_segmentation" in a for a in doc["annotations"]) == n_amodal
    # every label, not only the dynamic kinds: every annotation carries the keys
    every = tmp_path / "every"
    generate(str(every), [0], outputs=outs, amodal_kinds=("all",), **kw)
    frag = json.load(open(masks.fragment_path(str(every), 0)))
    assert frag["annotations"] and all("amodal_segmentation" in a for a in frag["annotations"])
