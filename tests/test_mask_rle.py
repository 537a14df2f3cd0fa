"""Per-object run-length masks, host side (no GPU): the NumPy restatement of
the span definition of include/csg_api.h (csg_mask_spans) that the GPU tests
compare against (tests/test_gpu_mask_rle.py), the readers of masks.py, the
native csgio_spans_to_rle against them byte for byte, the generator's COCO
fragment and the merge tool on a frame the CPU oracle rendered, and the ABI
bookkeeping."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from constructionsceneposeestimation_amd import masks, writers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN = -2 ** 31


def restate_spans(ids, n_labels):
    """The spec: ``ids`` (H, W) int -> (offsets (L + 1,) uint32, spans (total, 2)
    uint32).  A pixel belongs to label l iff its id equals l and 0 <= l < L; a
    span is a maximal vertical run of one label inside one column, stored as
    (x * H + y0, len); the records are ordered by label, then start."""
    ids = np.asarray(ids)
    H, W = ids.shape
    per = [[] for _ in range(n_labels)]
    for x in range(W):
        y = 0
        while y < H:
            l = int(ids[y, x])
            if 0 <= l < n_labels:
                y0 = y
                while y < H and int(ids[y, x]) == l:
                    y += 1
                per[l].append((x * H + y0, y - y0))
            else:
                y += 1
    off = np.zeros(n_labels + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in per])
    spans = np.array([s for p in per for s in p], np.uint32).reshape(-1, 2)
    return off, spans


def patterns(H, W, L, seed=0):
    """Named id images (H, W) int32 that exercise the definition."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    top = L - 1
    out = {
        "empty": np.full((H, W), -1),
        "one_label": np.full((H, W), top),                       # spans of length H: one COCO run
        "vertical_stripes": np.where(xx % 2 == 0, 0, -1),
        "horizontal_stripes": np.where(yy % 2 == 0, top, -1),    # the most spans a column can hold
        "checkerboard": np.where((xx + yy) % 2 == 0, 0, min(1, top)),
        "random": rng.integers(-1, min(L, 3), (H, W)),
        "foreign_ids": rng.choice([0, top, L, L + 5, -2, INT32_MIN, -1], (H, W)),
    }
    wrap = np.full((H, W), -1)                                   # ends a column's last row, starts the next
    wrap[H - 1, 0::2] = 0                                        # column's first row
    if W > 1:
        wrap[0, 1::2] = 0
    out["column_wrap"] = wrap
    return {k: v.astype(np.int32) for k, v in out.items()}


SHAPES = [(1, 1), (5, 3), (16, 64), (37, 70), (17, 129)]


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("L", [1, 3])
def test_round_trips(H, W, L):
    for name, ids in patterns(H, W, L).items():
        off, spans = restate_spans(ids, L)
        assert off[0] == 0 and off[L] == spans.shape[0]
        for l in range(L):
            sp = masks.label_spans(spans, off, l)
            want = ids == l
            assert np.array_equal(masks.spans_to_mask((H, W), sp), want), (name, l)
            counts = masks.spans_to_counts((H, W), sp)
            assert int(counts.sum()) == H * W and (counts[1:] > 0).all(), (name, l)
            s = masks.counts_to_string(counts)
            assert np.array_equal(masks.string_to_counts(s), counts), (name, l)
            assert np.array_equal(masks.decode((H, W), s), want), (name, l)
            assert np.array_equal(masks.decode((H, W), counts), want), (name, l)


def test_counts_merge_across_columns_and_end_at_the_last_pixel():
    H, W = 4, 3
    ids = np.full((H, W), -1, np.int32)
    ids[2:, 0] = 0
    ids[:, 1] = 0
    ids[:1, 2] = 0
    off, spans = restate_spans(ids, 1)
    assert spans.tolist() == [[2, 2], [4, 4], [8, 1]]
    assert masks.spans_to_counts((H, W), spans).tolist() == [2, 7, 3]
    ids[:, 2] = 0                                    # ... now the mask ends at the last pixel: no trailing zeros
    _, spans = restate_spans(ids, 1)
    assert masks.spans_to_counts((H, W), spans).tolist() == [2, 10]
    ids[:, 0] = 0                                    # a full frame: c0 = 0
    _, spans = restate_spans(ids, 1)
    assert masks.spans_to_counts((H, W), spans).tolist() == [0, 12]
    assert masks.spans_to_counts((H, W), np.zeros((0, 2), np.uint32)).tolist() == [12]
    with pytest.raises(ValueError):
        masks.spans_to_counts((H, W), [[4, 4], [2, 2]])
    with pytest.raises(ValueError):
        masks.spans_to_counts((H, W), [[10, 3]])


def test_string_anchors():
    assert masks.counts_to_string([0]) == "0"
    assert masks.counts_to_string([16]) == "`0"
    assert masks.counts_to_string([2, 5, 2, 4]) == "252O"           # the last count is a delta of -1
    assert masks.string_to_counts("252O").tolist() == [2, 5, 2, 4]
    for e in (5, 10, 15, 20, 26):
        s = masks.counts_to_string([2 ** e])
        assert len(s) == e // 5 + 1 and masks.string_to_counts(s).tolist() == [2 ** e]
    big = [0, 2 ** 26 - 5, 1, 2, 2]                                  # deltas of -(2^26 - 7) and +1
    assert masks.string_to_counts(masks.counts_to_string(big)).tolist() == big
    assert masks.decode((8192, 8192), masks.counts_to_string([2 ** 26])).sum() == 0
    with pytest.raises(ValueError):
        masks.string_to_counts("`")


def _native_equals_numpy(ids, L):
    H, W = ids.shape
    off, spans = restate_spans(ids, L)
    counts, c_off, text, s_off = writers.spans_to_rle(spans, off, H, W)
    assert c_off[0] == 0 and s_off[0] == 0 and c_off[L] == counts.shape[0] and s_off[L] == len(text)
    for l in range(L):
        got_c = counts[int(c_off[l]):int(c_off[l + 1])]
        got_s = text[int(s_off[l]):int(s_off[l + 1])]
        sp = masks.label_spans(spans, off, l)
        if sp.shape[0] == 0:                         # labels without a span have empty ranges
            assert got_c.shape[0] == 0 and got_s == b""
            continue
        want = masks.spans_to_counts((H, W), sp)
        assert got_c.dtype == np.uint32 and np.array_equal(got_c, want), l
        assert got_s == masks.counts_to_string(want).encode("ascii"), l


@pytest.mark.parametrize("H,W", SHAPES)
def test_native_equals_numpy(H, W):
    for L in (1, 3, 256):
        for ids in patterns(H, W, L).values():      # "empty", "one_label" (a full frame), masks ending at the last pixel
            _native_equals_numpy(ids, L)


def test_native_large_counts_and_bad_spans():
    H, W = 8192, 8192                                # counts up to 2^26; only the records are touched
    spans = np.array([[0, 1], [H * W - 1, 1]], np.uint32)
    off = np.array([0, 2], np.uint32)
    counts, _, text, _ = writers.spans_to_rle(spans, off, H, W)
    assert counts.tolist() == [0, 1, H * W - 2, 1]
    assert text == masks.counts_to_string(counts).encode() and masks.string_to_counts(text).tolist() == counts.tolist()
    for bad in ([[4, 4], [2, 2]], [[0, 0]], [[2, 4], [5, 1]], [[H * W - 1, 2]]):
        with pytest.raises(writers.CsgIoError):
            writers.spans_to_rle(np.array(bad, np.uint32), np.array([0, len(bad)], np.uint32), H, W)
    lib = writers.load()                             # capacities too small: -ENOSPC, and the offsets say what is needed
    c_off, s_off = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    small = np.zeros(2, np.uint32)
    rc = lib.csgio_spans_to_rle(spans.ctypes.data, off.ctypes.data, 1, H, W, small.ctypes.data, 2, c_off.ctypes.data,
                                None, 0, s_off.ctypes.data)
    assert rc == -28 and c_off[1] == 4 and s_off[1] == len(text) and small.tolist() == [0, 1]


def test_native_clean_under_asan_ubsan(tmp_path):
    """tests/rle_host.cpp (its own main) with csrc/csg_io.cpp under AddressSanitizer and
    UndefinedBehaviorSanitizer: output buffers of exactly the size asked for."""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "rle_host")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", os.path.join(ROOT, "tests", "rle_host.cpp"),
                    os.path.join(ROOT, "constructionsceneposeestimation_amd", "csrc", "csg_io.cpp"), "-lz", "-o", exe],
                   check=True)
    # (verify_asan_link_order=0: the environment may preload a library of its own)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "rle_host ok" in r.stdout, r.stdout + r.stderr


@pytest.fixture(scope="module")
def cone_frame():
    """The cone workload C1 at 96 x 64, rendered by the CPU oracle."""
    from constructionsceneposeestimation_amd.labels import object_poses
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import scene_labels
    from constructionsceneposeestimation_amd.workload import Workload
    from oracle.oracle import Oracle
    W, H, f = 96, 64, 3
    wl = Workload("C1", seed=0, width=W, height=H)
    st = wl.epoch(f // 10)
    V, P = wl.frame_params([f])
    o = Oracle(pack_scene(wl.scene), W, H)
    o.set_instance_models(np.asarray(st.models, np.float32).reshape(-1, 16))
    ref = o.render(V[0], P[0], want_stats=True)
    uv, vis = o.keypoints(V[0], P[0], st.keypoints, ref["depth"])
    L = scene_labels(wl.scene)
    return dict(wl=wl, f=f, H=H, W=W, L=L, ids=ref["instance"], stats=np.asarray(ref["inst_stats"])[:L],
                poses=object_poses(wl.scene, st.object_frames), uv=uv, vis=vis)


def _check_fragment(frag, fr, frame_id):
    H, W, ids = fr["H"], fr["W"], fr["ids"]
    assert frag["image"] == {"id": frame_id, "file_name": f"rgb/rgb_{frame_id:06d}.png", "height": H, "width": W}
    present = sorted(int(v) for v in np.unique(ids) if v >= 0)
    assert present and sorted(a["inst_idx"] for a in frag["annotations"]) == present
    by_idx = {p["inst_idx"]: p for p in fr["poses"]}
    for a in frag["annotations"]:
        i = a["inst_idx"]
        m = masks.decode(a["segmentation"]["size"], a["segmentation"]["counts"])
        assert a["segmentation"]["size"] == [H, W] and np.array_equal(m, ids == i)
        assert a["area"] == int(m.sum()) and a["iscrowd"] == 0
        ys, xs = np.nonzero(m)
        assert a["bbox"] == [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]
        assert a["id"] == frame_id * 65536 + i and a["image_id"] == frame_id
        assert a["category_id"] == by_idx[i]["class_id"] and a["prim_path"] == by_idx[i]["prim_path"]
        kp = np.array(a["keypoints"]).reshape(-1, 3)
        assert kp.shape[0] >= 9 and a["num_keypoints"] == int((kp[:, 2] > 0).sum())
        assert set(kp[:, 2].tolist()) <= {0, 1, 2}


def test_fragment_and_merge(cone_frame, tmp_path):
    fr = cone_frame
    off, spans = restate_spans(fr["ids"], fr["L"])
    kp = masks.keypoints_by_object(fr["wl"].kp_table)
    args = dict(height=fr["H"], width=fr["W"], poses=fr["poses"], inst_stats=fr["stats"], spans=spans, offsets=off,
                kp_by_obj=kp, kp_uv=fr["uv"], kp_vis=fr["vis"])
    frag = masks.coco_fragment(fr["f"], **args)
    _check_fragment(frag, fr, fr["f"])
    j = [k for k, p in enumerate(fr["poses"]) if p["inst_idx"] == frag["annotations"][0]["inst_idx"]][0]
    want_kp = [[float(fr["uv"][k][0]), float(fr["uv"][k][1]), int(fr["vis"][k])] for k in kp[j]]
    assert np.array(frag["annotations"][0]["keypoints"]).reshape(-1, 3).tolist() == want_kp
    # the generator's native writer makes the same bytes
    fw = writers.FragmentWriter(fr["poses"], fr["wl"].kp_table, fr["H"], fr["W"])
    fw.write(str(tmp_path / "native.json"), fr["f"], fr["stats"], spans, off, fr["uv"], fr["vis"])
    assert open(tmp_path / "native.json", "rb").read() == masks.fragment_bytes(frag)
    fw.write(str(tmp_path / "nokp.json"), fr["f"], fr["stats"], spans, off)
    assert open(tmp_path / "nokp.json", "rb").read() == masks.fragment_bytes(
        masks.coco_fragment(fr["f"], **dict(args, kp_uv=None, kp_vis=None)))
    with pytest.raises(writers.CsgIoError):
        fw.write(str(tmp_path / "bad.json"), fr["f"], fr["stats"], spans[:0], np.zeros_like(off))
    # the writer pool's "call" jobs: the fragment first, then the label file; the Python job can be pickled
    import pickle
    from functools import partial
    from constructionsceneposeestimation_amd.writer_pool import write_frame
    os.makedirs(tmp_path / "pool" / "coco")
    for job in (partial(fw.write, frame_id=fr["f"], inst_stats=fr["stats"], spans=spans, offsets=off, kp_uv=fr["uv"],
                        kp_vis=fr["vis"]),
                pickle.loads(pickle.dumps(partial(masks.write_fragment, frame_id=fr["f"], **args)))):
        path = masks.fragment_path(str(tmp_path / "pool"), fr["f"])
        write_frame({}, 0, [(path, "call", (job,))], {"frame_id": fr["f"]}, str(tmp_path / "pool" / "label.json"))
        assert open(path, "rb").read() == masks.fragment_bytes(frag) and not os.path.exists(path + ".tmp")
        assert json.load(open(tmp_path / "pool" / "label.json")) == {"frame_id": fr["f"]}
        os.remove(path)
    # two shards of two frames each against one directory holding all four
    one, two = tmp_path / "one", tmp_path / "two"
    for f in (7, 2, 11, 5):
        for d in (one, two / f"shard_{f % 2:02d}"):
            os.makedirs(d / "coco", exist_ok=True)
            masks.write_fragment(masks.fragment_path(str(d), f), frame_id=f, **args)
    assert json.load(open(masks.fragment_path(str(one), 7))) == masks.coco_fragment(7, **args)
    a = open(masks.merge(str(one)), "rb").read()
    b = open(masks.merge(str(two)), "rb").read()
    assert a == b and masks.main(["merge", str(one)]) == 0 and open(one / "coco" / "instances.json", "rb").read() == a
    doc = json.loads(a)
    assert sorted(doc) == ["annotations", "categories", "images"]
    assert [i["id"] for i in doc["images"]] == [2, 5, 7, 11]
    ids = [x["id"] for x in doc["annotations"]]
    assert ids == sorted(set(ids)) and len(ids) == 4 * len(frag["annotations"])
    from constructionsceneposeestimation_amd.identity import CONSTRUCTION_CLASS
    assert [c["id"] for c in doc["categories"]] == sorted(set(CONSTRUCTION_CLASS.values()))
    assert all(CONSTRUCTION_CLASS[c["name"]] == c["id"] for c in doc["categories"])
    assert {x["category_id"] for x in doc["annotations"]} <= {c["id"] for c in doc["categories"]}
    with pytest.raises(ValueError):                  # a label with pixels and no spans is an error, not an empty mask
        masks.coco_fragment(fr["f"], **dict(args, spans=spans[:0], offsets=np.zeros_like(off)))


def test_fragment_escapes_and_odd_values(tmp_path):
    """A counts string with a backslash (the character of a 5-bit group 12 with more to follow), a prim
    path that needs escaping, keypoints that are not finite, and objects that are skipped."""
    H, W = 50, 2
    ids = np.full((H, W), -1, np.int32)
    ids[44:, 0] = 1
    off, spans = restate_spans(ids, 3)
    assert "\\" in masks.counts_to_string(masks.spans_to_counts((H, W), masks.label_spans(spans, off, 1)))
    stats = np.zeros((3, 5), np.uint32)
    stats[1] = (6, 0, 44, 0, 49)
    poses = [{"inst_idx": 0, "class_id": 2, "prim_path": "/World/unseen"},
             {"inst_idx": 1, "class_id": 5, "prim_path": "/World/\"q\"\\b/é世"},
             {"inst_idx": 7, "class_id": 1, "prim_path": "/World/beyond"}]
    table = [(1, "a"), (1, "b"), (0, "c"), (1, "d")]
    uv = np.array([[0.1, 1e-7], [np.nan, np.inf], [3.0, 4.0], [-np.inf, 1e20]], np.float32)
    vis = np.array([2, 0, 1, 1], np.int32)
    frag = masks.coco_fragment(12, H, W, poses, stats, spans, off, masks.keypoints_by_object(table), uv, vis)
    assert len(frag["annotations"]) == 1 and frag["annotations"][0]["num_keypoints"] == 2
    assert frag["annotations"][0]["bbox"] == [0, 44, 1, 6] and frag["annotations"][0]["id"] == 12 * 65536 + 1
    fw = writers.FragmentWriter(poses, table, H, W)
    fw.write(str(tmp_path / "f.json"), 12, stats, spans, off, uv, vis)
    raw = open(tmp_path / "f.json", "rb").read()
    assert raw == masks.fragment_bytes(frag)
    back = json.loads(raw.decode("utf-8"))["annotations"][0]
    assert back["prim_path"] == poses[1]["prim_path"]
    assert np.array_equal(masks.decode((H, W), back["segmentation"]["counts"]), ids == 1)


def test_generator_knows_the_kind():
    from constructionsceneposeestimation_amd.generate import OUTPUTS, REFERENCE_OUTPUTS, parse_outputs
    assert "mask_rle" in OUTPUTS and "mask_rle" not in REFERENCE_OUTPUTS
    assert parse_outputs("rgb,mask_rle") == ("rgb", "mask_rle")


def test_header_and_abi():
    from constructionsceneposeestimation_amd import _lib
    for sym in ("csg_mask_spans", "csg_keep_instance", "csg_last_instance"):
        assert sym in _lib.EXPORTED
    assert "csgio_spans_to_rle" in writers.EXPORTED
    hdr = open(os.path.join(ROOT, "include", "csg_api.h")).read()
    assert re.search(r"\bint\s+csg_mask_spans\s*\(\s*csg_ctx\s*\*\s*ctx,\s*const\s+csg_span_job\s*\*\s*job,"
                     r"\s*uint32_t\s+n_frames,\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    assert re.search(r"#define\s+CSG_ABI_VERSION\s+14\b", hdr) and _lib.ABI_VERSION == 14
    io_hdr = open(os.path.join(ROOT, "include", "csg_io.h")).read()
    m = re.search(r"#define\s+CSGIO_ABI_VERSION\s+(\d+)", io_hdr)
    assert int(m.group(1)) == writers.ABI_VERSION == writers.load().csgio_abi_version()
    fields = [n for n, _ in _lib.SpanJob._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "csg_api.h"\n#include "csg_io.h"\nint main(void){\n'
    prog += 'printf("sizeof %zu\\nspan %zu\\nlimit %u\\n", sizeof(csg_span_job), sizeof(csg_span), CSG_SPAN_MAX_LABELS);\n'
    for m in fields:
        prog += f'printf("{m} %zu\\n", offsetof(csg_span_job, {m}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:          # the headers still compile as C
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe],
                       check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert C.sizeof(_lib.SpanJob) == sizes["sizeof"] == 40 and sizes["span"] == 8
    assert sizes["limit"] == _lib.SPAN_MAX_LABELS == 256
    for m in fields:
        assert getattr(_lib.SpanJob, m).offset == sizes[m], m
    lib = _lib.load()
    assert lib.csg_abi_version() == 14
    job = _lib.SpanJob(8, 8, 1, 8, None, None, None)
    assert lib.csg_mask_spans(None, C.byref(job), 1, None) == -1
