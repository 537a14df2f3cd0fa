"""Full-frame amodal masks as run-length spans (csg_amodal_spans), host side (no
GPU): the restatement the GPU tests compare against (tests/test_gpu_amodal_rle.py)
-- per label, the span restatement of tests/test_mask_rle.py on the amodal image
of tests/test_crop_amodal.py (the CPU oracle's frame with every instance of
another label removed) --, its preconditions on the oracle alone, the COCO
fragment with the amodal keys in Python and natively, masks.visible_fraction and
the ABI bookkeeping."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from constructionsceneposeestimation_amd import masks, writers
from tests.test_crop_amodal import FIDS3, H3, UNKNOWN, W3, amodal_image, c3_reference
from tests.test_mask_rle import restate_spans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = (0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0)


def stats_of(mask):
    """amodal_stats of one label: pixels and inclusive box of a bool image, inst_stats' empty value without pixels."""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return EMPTY
    return (int(ys.size), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def restate_amodal_spans(images, n_labels, shape):
    """``images``: label -> (H, W) bool amodal image (labels left out have no pixels).  Returns (offsets
    (L + 1,) uint32, spans (total, 2) uint32, stats (L, 5) uint32): per label the spans of its own image
    under csg_mask_spans' rules, concatenated by label."""
    off = np.zeros(n_labels + 1, np.uint32)
    parts, stats = [], np.zeros((n_labels, 5), np.uint32)
    for l in range(n_labels):
        img = images.get(l)
        if img is None or not img.any():
            off[l + 1] = off[l]
            stats[l] = EMPTY
            continue
        assert img.shape == tuple(shape)
        o, sp = restate_spans(np.where(img, l, -1), n_labels)
        assert o[l] == 0 and o[l + 1] == sp.shape[0] == o[-1]
        parts.append(sp)
        off[l + 1] = off[l] + sp.shape[0]
        stats[l] = stats_of(img)
    spans = np.concatenate(parts) if parts else np.zeros((0, 2), np.uint32)
    return off, spans.astype(np.uint32).reshape(-1, 2), stats


def oracle_amodal_images(o, inst_label, models16, view, proj, labels):
    return {int(l): amodal_image(o, inst_label, models16, view, proj, int(l)) for l in labels}


@functools.lru_cache(maxsize=None)
def amodal_reference():
    """The three frames of ``c3_reference`` (480 x 272: 8.5 words high, 7.5 column groups wide; transform
    sets 0, 1, 2) with, per frame, every label's amodal image from the oracle -- run only for labels whose
    label_covered is non-zero; the others have no amodal pixel by the same definition -- and the restated
    spans, offsets and stats.  Computed once, read-only."""
    from constructionsceneposeestimation_amd.packing import pack_scene
    from oracle.oracle import Oracle
    ref = c3_reference(None)
    wl, L = ref["wl"], ref["n_labels"]
    packed = pack_scene(wl.scene)
    o = Oracle(packed, W3, H3)
    images, frames = [], []
    for k, f in enumerate(FIDS3):
        models = np.asarray(wl.epoch(f // 10).models, np.float32).reshape(-1, 16)
        labels = [l for l in range(L) if int(ref["covered"][k, l]) != 0]
        images.append(oracle_amodal_images(o, packed.inst_label, models, ref["V"][k], ref["P"][k], labels))
        frames.append(restate_amodal_spans(images[k], L, (H3, W3)))
    for fr in frames:
        for a in fr:
            a.setflags(write=False)
    for d in images:
        for a in d.values():
            a.setflags(write=False)
    return dict(ref=ref, L=L, images=images, frames=frames)


def test_preconditions_on_the_oracle():
    am = amodal_reference()
    ref, L = am["ref"], am["L"]
    larger = 0
    for k in range(3):
        off, spans, stats = am["frames"][k]
        assert off[0] == 0 and off[L] == spans.shape[0]
        for l in range(L):
            cov = int(ref["covered"][k, l])
            img = am["images"][k].get(l)
            px = int(img.sum()) if img is not None else 0
            assert int(stats[l, 0]) == px
            if not cov & UNKNOWN:                      # wherever label_covered is known it is the amodal pixel count
                assert cov == px, (k, l)
            vis = ref["instance"][k] == l
            if img is not None:
                assert not (vis & ~img).any(), (k, l)  # visible is a subset of amodal
                larger += int(px > int(vis.sum()))
                assert np.array_equal(masks.spans_to_mask((H3, W3), masks.label_spans(spans, off, l)), img)
            else:
                assert not vis.any() and off[l + 1] == off[l]
    print("labels with an amodal mask strictly larger than the visible one:", larger)
    assert larger >= 15
    assert H3 % 32 != 0 and W3 % 64 != 0               # both ragged edges
    assert sorted(int(s) for s in ref["fr"]["xform_set"]) == [0, 1, 2]


def test_restatement_on_a_tiny_image():
    a = np.zeros((5, 3), bool)
    a[1:4, 0] = True
    a[4, 1] = True
    a[0, 2] = True
    b = np.ones((5, 3), bool)                          # overlaps a: the point of amodal masks
    off, spans, stats = restate_amodal_spans({0: a, 2: b}, 4, (5, 3))
    assert off.tolist() == [0, 3, 3, 6, 6]
    assert spans.tolist() == [[1, 3], [9, 1], [10, 1], [0, 5], [5, 5], [10, 5]]
    assert stats.tolist() == [[5, 0, 0, 2, 4], list(EMPTY), [15, 0, 0, 2, 4], list(EMPTY)]


def test_visible_fraction():
    inst = np.zeros((2, 3, 5), np.uint32)
    amo = np.zeros((2, 3, 5), np.uint32)
    inst[0, 0, 0], amo[0, 0, 0] = 10, 40
    inst[0, 1, 0], amo[0, 1, 0] = 7, 7
    amo[1, 2, 0] = 9                                   # wholly hidden
    inst[1, 0, 0], amo[1, 0, 0] = 1, 3
    got = masks.visible_fraction(inst, amo)
    assert got.dtype == np.float64 and got.shape == (2, 3)
    exp = np.array([[0.25, 1.0, np.nan], [1.0 / 3.0, np.nan, 0.0]])
    assert np.array_equal(got, exp, equal_nan=True)
    one = masks.visible_fraction(inst[0, 0], amo[0, 0])
    assert one.shape == () and one == 0.25


def _synthetic_frame():
    """Three labels in a 40 x 30 frame: label 0 half hidden behind label 1, label 1 unoccluded, label 2
    visible but not eligible (no amodal data)."""
    H, W, L = 40, 30, 3
    ids = np.full((H, W), -1, np.int32)
    amodal = {0: np.zeros((H, W), bool), 1: np.zeros((H, W), bool)}
    amodal[0][5:25, 3:12] = True
    amodal[1][10:38, 8:20] = True
    ids[amodal[0]] = 0
    ids[amodal[1]] = 1                                 # in front of label 0
    ids[0:3, 25:30] = 2
    off, spans = restate_spans(ids, L)
    stats = np.array([stats_of(ids == l) for l in range(L)], np.uint32)
    a_off, a_spans, a_stats = restate_amodal_spans(amodal, L, (H, W))
    poses = [{"inst_idx": 0, "class_id": 2, "prim_path": "/World/half"},
             {"inst_idx": 1, "class_id": 5, "prim_path": "/World/front"},
             {"inst_idx": 2, "class_id": 1, "prim_path": "/World/static"}]
    table = [(0, "a"), (1, "b"), (0, "c")]
    uv = np.array([[4.5, 6.25], [9.0, 11.0], [-1.5, 3.0]], np.float32)
    vis = np.array([2, 1, 0], np.int32)
    return dict(H=H, W=W, L=L, ids=ids, amodal=amodal, off=off, spans=spans, stats=stats, a_off=a_off,
                a_spans=a_spans, a_stats=a_stats, poses=poses, table=table, uv=uv, vis=vis)


def test_fragment_with_and_without_the_amodal_keys(tmp_path):
    s = _synthetic_frame()
    H, W = s["H"], s["W"]
    base = dict(height=H, width=W, poses=s["poses"], inst_stats=s["stats"], spans=s["spans"], offsets=s["off"],
                kp_by_obj=masks.keypoints_by_object(s["table"]), kp_uv=s["uv"], kp_vis=s["vis"])
    amo = dict(amodal_spans=s["a_spans"], amodal_offsets=s["a_off"], amodal_stats=s["a_stats"])
    plain = masks.coco_fragment(9, **base)
    frag = masks.coco_fragment(9, **base, **amo)
    assert [a["inst_idx"] for a in frag["annotations"]] == [a["inst_idx"] for a in plain["annotations"]] == [0, 1, 2]
    for a, b in zip(frag["annotations"], plain["annotations"]):
        keys = list(a)
        if a["inst_idx"] == 2:                         # not eligible: the annotation is what it was
            assert a == b and keys == list(b)
            continue
        at = keys.index("segmentation")
        assert keys[at + 1:at + 5] == ["amodal_bbox", "amodal_area", "amodal_segmentation", "inst_idx"]
        assert {k: v for k, v in a.items() if not k.startswith("amodal_")} == b
        img = s["amodal"][a["inst_idx"]]
        assert a["amodal_segmentation"]["size"] == [H, W]
        m = masks.decode(a["amodal_segmentation"]["size"], a["amodal_segmentation"]["counts"])
        assert np.array_equal(m, img)
        assert not (masks.decode(a["segmentation"]["size"], a["segmentation"]["counts"]) & ~m).any()
        px, x0, y0, x1, y1 = stats_of(img)
        assert a["amodal_area"] == px >= a["area"] and a["amodal_bbox"] == [x0, y0, x1 - x0 + 1, y1 - y0 + 1]
    assert frag["annotations"][0]["amodal_area"] > frag["annotations"][0]["area"]
    assert frag["annotations"][1]["amodal_area"] == frag["annotations"][1]["area"]
    # without the amodal arguments the bytes are what they were
    assert masks.fragment_bytes(plain) == masks.fragment_bytes(masks.coco_fragment(9, **base, amodal_spans=None))
    # the native writer: byte for byte, with and without keypoints, with and without the amodal arrays
    fw = writers.FragmentWriter(s["poses"], s["table"], H, W)
    fw.write(str(tmp_path / "a.json"), 9, s["stats"], s["spans"], s["off"], s["uv"], s["vis"], **amo)
    assert open(tmp_path / "a.json", "rb").read() == masks.fragment_bytes(frag)
    fw.write(str(tmp_path / "b.json"), 9, s["stats"], s["spans"], s["off"], **amo)
    assert open(tmp_path / "b.json", "rb").read() == masks.fragment_bytes(
        masks.coco_fragment(9, **dict(base, kp_uv=None, kp_vis=None), **amo))
    fw.write(str(tmp_path / "c.json"), 9, s["stats"], s["spans"], s["off"], s["uv"], s["vis"])
    assert open(tmp_path / "c.json", "rb").read() == masks.fragment_bytes(plain)
    # all zeros eligible: empty amodal arrays add nothing
    none = dict(amodal_spans=np.zeros((0, 2), np.uint32), amodal_offsets=np.zeros(s["L"] + 1, np.uint32),
                amodal_stats=np.array([EMPTY] * s["L"], np.uint32))
    assert masks.fragment_bytes(masks.coco_fragment(9, **base, **none)) == masks.fragment_bytes(plain)
    fw.write(str(tmp_path / "d.json"), 9, s["stats"], s["spans"], s["off"], s["uv"], s["vis"], **none)
    assert open(tmp_path / "d.json", "rb").read() == masks.fragment_bytes(plain)
    # amodal pixels and no amodal spans: an error in both, as for the visible mask; so is a partial set
    bad = dict(none, amodal_stats=s["a_stats"])
    with pytest.raises(ValueError):
        masks.coco_fragment(9, **base, **bad)
    with pytest.raises(writers.CsgIoError):
        fw.write(str(tmp_path / "e.json"), 9, s["stats"], s["spans"], s["off"], **bad)
    with pytest.raises(ValueError):
        masks.coco_fragment(9, **base, amodal_spans=s["a_spans"])
    with pytest.raises(writers.CsgIoError):
        fw.write(str(tmp_path / "e.json"), 9, s["stats"], s["spans"], s["off"], amodal_stats=s["a_stats"])
    # a counts string with a backslash in the amodal mask is escaped natively as json.dumps escapes it
    H2, W2 = 50, 2
    ids = np.full((H2, W2), -1, np.int32)
    ids[44:, 0] = 0
    off2, sp2 = restate_spans(ids, 1)
    st2 = np.array([stats_of(ids == 0)], np.uint32)
    assert "\\" in masks.counts_to_string(masks.spans_to_counts((H2, W2), sp2))
    p2 = [{"inst_idx": 0, "class_id": 1, "prim_path": "/World/x"}]
    fw2 = writers.FragmentWriter(p2, [], H2, W2)
    fw2.write(str(tmp_path / "f.json"), 1, st2, sp2, off2, amodal_spans=sp2, amodal_offsets=off2, amodal_stats=st2)
    assert open(tmp_path / "f.json", "rb").read() == masks.fragment_bytes(
        masks.coco_fragment(1, H2, W2, p2, st2, sp2, off2, amodal_spans=sp2, amodal_offsets=off2, amodal_stats=st2))


def test_merge_keeps_the_amodal_keys(tmp_path):
    s = _synthetic_frame()
    args = dict(height=s["H"], width=s["W"], poses=s["poses"], inst_stats=s["stats"], spans=s["spans"],
                offsets=s["off"], amodal_spans=s["a_spans"], amodal_offsets=s["a_off"], amodal_stats=s["a_stats"])
    os.makedirs(tmp_path / "coco")
    for f in (3, 1):
        masks.write_fragment(masks.fragment_path(str(tmp_path), f), frame_id=f, **args)
    doc = json.load(open(masks.merge(str(tmp_path))))
    want = masks.coco_fragment(1, **args)["annotations"] + masks.coco_fragment(3, **args)["annotations"]
    assert doc["annotations"] == want
    assert sum("amodal_segmentation" in a for a in doc["annotations"]) == 4


def test_generator_knows_the_kind():
    from constructionsceneposeestimation_amd.generate import OUTPUTS, REFERENCE_OUTPUTS, main, parse_outputs
    assert "amodal_rle" in OUTPUTS and "amodal_rle" not in REFERENCE_OUTPUTS
    assert parse_outputs("rgb,mask_rle,amodal_rle") == ("rgb", "mask_rle", "amodal_rle")
    with pytest.raises(ValueError):
        parse_outputs("rgb,amodal_rle")
    with pytest.raises(SystemExit) as e:               # an argument error, before anything is rendered
        main(["--out", os.devnull, "--outputs", "rgb,amodal_rle"])
    assert e.value.code == 2


def test_header_and_abi():
    from constructionsceneposeestimation_amd import _lib
    assert "csg_amodal_spans" in _lib.EXPORTED and "csgio_write_coco_fragment_amodal" in writers.EXPORTED
    hdr = open(os.path.join(ROOT, "include", "csg_api.h")).read()
    assert re.search(r"\bint\s+csg_amodal_spans\s*\(\s*csg_ctx\s*\*\s*ctx,\s*const\s+csg_amodal_span_job\s*\*\s*job,"
                     r"\s*uint32_t\s+n_frames,\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    assert re.search(r"#define\s+CSG_ABI_VERSION\s+14\b", hdr) and _lib.ABI_VERSION == 14
    io_hdr = open(os.path.join(ROOT, "include", "csg_io.h")).read()
    assert re.search(r"\bint\s+csgio_write_coco_fragment_amodal\s*\(", io_hdr)
    m = re.search(r"#define\s+CSGIO_ABI_VERSION\s+(\d+)", io_hdr)
    assert int(m.group(1)) == writers.ABI_VERSION == writers.load().csgio_abi_version()
    fields = [n for n, _ in _lib.AmodalSpanJob._fields_]
    assert fields == ["capacity", "frames", "eligible", "spans", "span_offsets", "amodal_stats"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "csg_api.h"\n#include "csg_io.h"\nint main(void){\n'
    prog += 'printf("sizeof %zu\\ncoco %zu\\n", sizeof(csg_amodal_span_job), sizeof(csgio_coco));\n'
    for m in fields:
        prog += f'printf("{m} %zu\\n", offsetof(csg_amodal_span_job, {m}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:           # the headers still compile as C
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe],
                       check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert C.sizeof(_lib.AmodalSpanJob) == sizes["sizeof"] == 48
    assert C.sizeof(writers.Coco) == sizes["coco"]     # the fragment struct is unchanged
    for m in fields:
        assert getattr(_lib.AmodalSpanJob, m).offset == sizes[m], m
    lib = _lib.load()
    assert lib.csg_abi_version() == 14
    job = _lib.AmodalSpanJob(8, None, None, None, None, None)
    assert lib.csg_amodal_spans(None, C.byref(job), 1, None) == -1
