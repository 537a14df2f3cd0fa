"""Amodal crop masks (csg_crop_amodal), host side: the restatement the GPU
tests compare against (tests/test_gpu_crop_amodal.py) -- the CPU oracle renders
the frame with every instance of another label removed, and the crops'
restatement (tests/test_object_crops.py) samples that image --, its
preconditions on the crops' own test frames, crops.visible_fraction and the ABI
bookkeeping (no GPU)."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests.test_object_crops import INFO_DTYPE, restate_crops, slot_is_live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W3, H3 = 480, 272
FIDS3 = [4, 17, 23]          # epochs 0, 1, 2 -> transform sets 0, 1, 2
K3, S3, PAD3, MINPX3 = 8, 64, 1.5, 64
UNKNOWN = 0x80000000


def amodal_image(o, inst_label, models16, view, proj, label, textures=None):
    """The full-frame amodal mask of ``label`` (H, W) bool: the oracle's frame
    with the models of every instance of another label set to zero (a zero
    model draws nothing), which then holds only -1 and ``label``."""
    m = np.array(models16, np.float32).reshape(-1, 16)
    m[np.asarray(inst_label) != int(label)] = 0
    st = o.frame_state(models16=m, texture_per_material=textures)
    inst = st.render(view, proj)["instance"]
    assert set(np.unique(inst).tolist()) <= {-1, int(label)}
    return inst == int(label)


def restate_amodal(o, inst_label, models16, view, proj, info, S, n_labels, textures=None):
    """crop_amodal (K, S, S) of one frame's slots ``info`` (K,): a dead slot is
    zeros, a live one the crop_mask of the restated crops on its label's amodal image."""
    out = np.zeros((info.shape[0], S, S), np.uint8)
    images = {}
    for k, slot in enumerate(info):
        if not slot_is_live(slot, n_labels, True):
            continue
        L = int(slot["label"])
        if L not in images:
            images[L] = amodal_image(o, inst_label, models16, view, proj, L, textures)
        ids = np.where(images[L], L, -1).astype(np.int32)
        out[k] = restate_crops(ids[None], S, 1, n_labels, info=np.asarray(slot).reshape(1, 1))["crop_mask"][0, 0]
    return out


@functools.lru_cache(maxsize=None)
def c3_reference(kinds=None):
    """The crops' three test frames at 480x272 for one set of object kinds (None:
    the dynamic ones): the oracle's frames, the planned slots, the visible and
    the amodal masks, per-label full-frame amodal counts.  Computed once, read-only."""
    from constructionsceneposeestimation_amd.crops import DYNAMIC_KINDS, eligible_labels
    from constructionsceneposeestimation_amd.packing import pack_scene
    from constructionsceneposeestimation_amd.renderer import make_frames
    from constructionsceneposeestimation_amd.workload import Workload
    from oracle.oracle import Oracle
    wl = Workload("C3", seed=3, width=W3, height=H3)
    epochs = [0, 1, 2]
    V, P = wl.frame_params(FIDS3)
    fr = make_frames(V, P, [epochs.index(f // 10) for f in FIDS3], FIDS3)
    packed = pack_scene(wl.scene)
    o = Oracle(packed, W3, H3)
    elig = eligible_labels(wl.scene, DYNAMIC_KINDS if kinds is None else kinds)
    inst, stats, cov, models = [], [], [], []
    for k, f in enumerate(FIDS3):
        models.append(np.asarray(wl.epoch(f // 10).models, np.float32).reshape(-1, 16))
        ref = o.frame_state(models16=models[k]).render(V[k], P[k], covered=True)
        inst.append(ref["instance"])
        stats.append(ref["inst_stats"])
        cov.append(ref["label_covered"])
    inst, stats, cov = np.stack(inst), np.stack(stats), np.stack(cov)
    n_labels = stats.shape[1]
    vis = restate_crops(inst, S3, K3, n_labels, stats=stats, eligible=elig, min_pixels=MINPX3, pad=PAD3)
    info = vis["info"]
    amodal = np.stack([restate_amodal(o, packed.inst_label, models[k], V[k], P[k], info[k], S3, n_labels)
                       for k in range(3)])
    full = np.zeros(info.shape, np.int64)     # full-frame amodal pixels of each live slot's label
    for k in range(3):
        for j, slot in enumerate(info[k]):
            if slot["label"] >= 0:
                full[k, j] = amodal_image(o, packed.inst_label, models[k], V[k], P[k], slot["label"]).sum()
    out = dict(wl=wl, fr=fr, epochs=epochs, V=V, P=P, elig=elig, n_labels=n_labels, instance=inst, stats=stats,
               covered=cov, info=info, crop_mask=vis["crop_mask"], crop_amodal=amodal, full=full)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("kinds,live", [(None, [8, 6, 7]), (("static",), [8, 8, 8])])
def test_preconditions_on_the_oracle(kinds, live):
    ref = c3_reference(kinds)
    info, vis, amo = ref["info"], ref["crop_mask"], ref["crop_amodal"]
    on = info["label"] >= 0
    assert on.sum(1).tolist() == live
    assert set(np.unique(amo).tolist()) <= {0, 255}
    assert not amo[~on].any()
    assert (vis <= amo).all()                                   # visible is a subset of amodal
    larger = [(amo[f, k] > 0).sum() > (vis[f, k] > 0).sum() for f, k in np.argwhere(on)]
    print("slots", int(on.sum()), "strictly larger", int(np.sum(larger)))
    assert np.sum(larger) >= 15
    # the definition is label_covered made per pixel: same count, and none of these is unknown
    for f, k in np.argwhere(on):
        L = int(info[f, k]["label"])
        assert not ref["covered"][f, L] & UNKNOWN
        assert ref["full"][f, k] == int(ref["covered"][f, L]), (f, k, L)


def test_static_windows_reach_outside_the_frame():
    info = c3_reference(("static",))["info"]
    assert info["x0"].min() < -50 and info["y0"].min() < -60
    assert (info["side"] / np.float32(S3)).max() > 5                           # minified ...
    dyn = c3_reference(None)["info"]
    assert (dyn["side"][dyn["label"] >= 0] / np.float32(S3)).min() < 0.5       # ... and magnified windows


def test_visible_fraction():
    from constructionsceneposeestimation_amd.crops import visible_fraction
    S = 8
    mask = np.zeros((2, 3, S, S), np.uint8)
    amodal = np.zeros((2, 3, S, S), np.uint8)
    amodal[0, 0, :4] = 255
    mask[0, 0, :2] = 255                   # half of it visible
    amodal[0, 1, 2:5, 1:7] = 255
    mask[0, 1, 2:5, 1:7] = 255             # unoccluded
    amodal[1, 2, 0, :3] = 255
    mask[1, 2, 0, 0] = 255                 # one of three
    amodal[1, 0] = 255                     # wholly hidden
    got = visible_fraction(mask, amodal)
    assert got.dtype == np.float64 and got.shape == (2, 3)
    exp = np.array([[0.5, 1.0, np.nan], [0.0, np.nan, 1.0 / 3.0]])
    assert np.array_equal(got, exp, equal_nan=True)
    one = visible_fraction(mask[0, 0], amodal[0, 0])
    assert one.shape == () and one == 0.5


def test_header_declares_the_entry_point():
    from constructionsceneposeestimation_amd import _lib
    assert "csg_crop_amodal" in _lib.EXPORTED
    hdr = open(os.path.join(ROOT, "include", "csg_api.h")).read()
    assert re.search(r"\bint\s+csg_crop_amodal\s*\(\s*csg_ctx\s*\*\s*ctx,\s*const\s+csg_amodal_job\s*\*\s*job,"
                     r"\s*uint32_t\s+n_frames,\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    assert re.search(r"#define\s+CSG_ABI_VERSION\s+14\b", hdr)
    assert _lib.ABI_VERSION == 14


def test_job_struct_size_and_null_context():
    from constructionsceneposeestimation_amd import _lib
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "csg_api.h"\nint main(){\n'
            'printf("sizeof %zu\\n", sizeof(csg_amodal_job));\n')
    fields = ("size", "per_frame", "frames", "info", "crop_amodal")
    for m in fields:
        prog += f'printf("{m} %zu\\n", offsetof(csg_amodal_job, {m}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert C.sizeof(_lib.AmodalJob) == sizes["sizeof"] == 32
    for m in fields:
        assert getattr(_lib.AmodalJob, m).offset == sizes[m], m
    lib = _lib.load()
    assert lib.csg_abi_version() == 14
    job = _lib.AmodalJob(64, 8, None, None, None)
    assert lib.csg_crop_amodal(None, C.byref(job), 1, None) == -1
    assert INFO_DTYPE.itemsize == 32
