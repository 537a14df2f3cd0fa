"""Amodal depth and object coordinates of the crops (csg_crop_amodal_geometry),
host side: the restatement the GPU tests compare against
(tests/test_gpu_crop_amodal_geometry.py) -- per live slot the CPU oracle renders
the frame with every instance of another label removed; its depth is the amodal
depth image, the obj_coords restatement on its ids and points the amodal
coordinate image, and the crops' restatement samples both --, its preconditions
on the crops' own test frames, crops.hidden_mask and the ABI bookkeeping (no GPU)."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests.test_crop_amodal import FIDS3, c3_reference
from tests.test_obj_coords import restate_obj_coords
from tests.test_object_crops import INFO_DTYPE, restate_crops, slot_is_live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def amodal_render(o, inst_label, models16, view, proj, label, textures=None):
    """The oracle's frame (with ``points``) of ``label`` alone: the models of every
    instance of another label set to zero, as tests.test_crop_amodal.amodal_image."""
    m = np.array(models16, np.float32).reshape(-1, 16)
    m[np.asarray(inst_label) != int(label)] = 0
    ref = o.frame_state(models16=m, texture_per_material=textures).render(view, proj, extra=True)
    assert set(np.unique(ref["instance"]).tolist()) <= {-1, int(label)}
    return ref


def restate_amodal_geometry(o, inst_label, models16, view, proj, info, S, n_labels, table=None, textures=None):
    """crop_amodal (K, S, S) uint8, crop_amodal_depth (K, S, S) float32 and
    crop_amodal_coords (K, S, S, 3) uint16 of one frame's slots ``info`` (K,).
    ``table`` (n_labels, 3, 4) is the set's object-frame table (None: no table,
    zero coordinates).  A dead slot is 0, +inf and (0, 0, 0)."""
    K = info.shape[0]
    out = dict(crop_amodal=np.zeros((K, S, S), np.uint8), crop_amodal_depth=np.full((K, S, S), np.inf, np.float32),
               crop_amodal_coords=np.zeros((K, S, S, 3), np.uint16))
    if table is None:
        table = np.zeros((n_labels, 3, 4), np.float32)
    frames = {}
    for k, slot in enumerate(info):
        if not slot_is_live(slot, n_labels, True):
            continue
        L = int(slot["label"])
        if L not in frames:
            ref = amodal_render(o, inst_label, models16, view, proj, L, textures)
            frames[L] = (ref["instance"], ref["depth"], restate_obj_coords(ref["instance"], ref["points"], table))
        ids, depth, coords = frames[L]
        got = restate_crops(ids[None], S, 1, n_labels, depth=depth[None], obj_coords=coords[None],
                            info=np.asarray(slot).reshape(1, 1))
        out["crop_amodal"][k] = got["crop_mask"][0, 0]
        out["crop_amodal_depth"][k] = got["crop_depth"][0, 0]
        out["crop_amodal_coords"][k] = got["crop_coords"][0, 0]
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def c3_geometry(kinds=None):
    """tests.test_crop_amodal.c3_reference(kinds) with the geometry: the full
    frames' depth and object coordinates, the visible crops of both, and the
    restated amodal mask, depth and coordinates (n, K, ...).  Computed once, read-only."""
    from constructionsceneposeestimation_amd.labels import object_unit_transforms
    from constructionsceneposeestimation_amd.packing import pack_scene
    from oracle.oracle import Oracle
    from tests.test_crop_amodal import H3, K3, S3, W3
    ref = c3_reference(kinds)
    wl, V, P, info, n_labels = ref["wl"], ref["V"], ref["P"], ref["info"], ref["n_labels"]
    packed = pack_scene(wl.scene)
    o = Oracle(packed, W3, H3)
    depth, coords, tables, amo = [], [], [], []
    for k, f in enumerate(FIDS3):
        st = wl.epoch(f // 10)
        models = np.asarray(st.models, np.float32).reshape(-1, 16)
        tables.append(object_unit_transforms(wl.scene, st.object_frames))
        full = o.frame_state(models16=models).render(V[k], P[k], extra=True)
        assert np.array_equal(full["instance"], ref["instance"][k])
        depth.append(full["depth"])
        coords.append(restate_obj_coords(full["instance"], full["points"], tables[k]))
        amo.append(restate_amodal_geometry(o, packed.inst_label, models, V[k], P[k], info[k], S3, n_labels, tables[k]))
    depth, coords = np.stack(depth), np.stack(coords)
    vis = restate_crops(ref["instance"], S3, K3, n_labels, depth=depth, obj_coords=coords, info=info)
    out = dict(depth=depth, obj_coords=coords, tables=np.stack(tables), crop_mask=vis["crop_mask"],
               crop_depth=vis["crop_depth"], crop_coords=vis["crop_coords"])
    for name in ("crop_amodal", "crop_amodal_depth", "crop_amodal_coords"):
        out[name] = np.stack([a[name] for a in amo])
    for a in out.values():
        a.setflags(write=False)
    return out


def frame_depth_at_samples(info, S, depth):
    """(K, S, S) the frame's depth at each sample's source pixel and (K, S, S)
    bool `inside`, for one frame's explicit slots (dead slots: not inside)."""
    from tests.test_object_crops import _axis
    K = info.shape[0]
    at = np.full((K, S, S), np.inf, np.float32)
    inside = np.zeros((K, S, S), bool)
    H, W = depth.shape
    for k, slot in enumerate(info):
        if int(slot["label"]) < 0:
            continue
        step = np.float32(slot["side"]) / np.float32(S)
        nx, inx = _axis(slot["x0"], step, S, W)[:2]
        ny, iny = _axis(slot["y0"], step, S, H)[:2]
        inside[k] = iny[:, None] & inx[None, :]
        at[k] = depth[ny[:, None], nx[None, :]]
    return at, inside


@pytest.mark.parametrize("kinds", [None, ("static",)])
def test_preconditions_on_the_oracle(kinds):
    from constructionsceneposeestimation_amd.crops import hidden_mask
    ref, geo = c3_reference(kinds), c3_geometry(kinds)
    info, S = ref["info"], geo["crop_mask"].shape[-1]
    assert np.array_equal(geo["crop_mask"], ref["crop_mask"])
    assert np.array_equal(geo["crop_amodal"], ref["crop_amodal"])            # the mask of §13.2, byte for byte
    vis, amo = geo["crop_mask"] == 255, geo["crop_amodal"] == 255
    hidden = hidden_mask(geo["crop_mask"], geo["crop_amodal"])
    per_slot = hidden.sum((-2, -1))
    print("kinds", kinds, "amodal", int(amo.sum()), "hidden", int(hidden.sum()), "slots with >= 50",
          int((per_slot >= 50).sum()))
    assert hidden.sum() >= 500 and (per_slot >= 50).sum() >= 4
    # off the object: +inf and zeros; on it: a finite depth
    assert np.isposinf(geo["crop_amodal_depth"][~amo]).all() and not geo["crop_amodal_coords"][~amo].any()
    assert np.isfinite(geo["crop_amodal_depth"][amo]).all()
    # under the visible mask the amodal geometry is the visible one, bit for bit
    assert vis.sum() >= 5000
    assert np.array_equal(bits(geo["crop_amodal_depth"])[vis], bits(geo["crop_depth"])[vis])
    assert np.array_equal(geo["crop_amodal_coords"][vis], geo["crop_coords"][vis])
    # hidden samples lie behind what the frame shows there, and carry coordinates
    for f in range(info.shape[0]):
        at, inside = frame_depth_at_samples(info[f], S, geo["depth"][f])
        h = hidden[f]
        assert inside[h].all()
        assert (geo["crop_amodal_depth"][f][h] >= at[h]).all(), f
        assert geo["crop_amodal_coords"][f][h].any(-1).all(), f
        print("frame", FIDS3[f], "hidden", int(h.sum()), "visible", int((vis[f]).sum()))


def test_hidden_mask():
    from constructionsceneposeestimation_amd.crops import hidden_mask
    S = 4
    mask = np.zeros((2, S, S), np.uint8)
    amodal = np.zeros((2, S, S), np.uint8)
    amodal[0, :2] = 255
    mask[0, 0] = 255                       # the first row visible, the second hidden
    mask[1, 3, 3] = 255                    # (visible without amodal does not occur; it is not hidden)
    amodal[1, 0, 1] = 1                    # any non-zero value marks a sample
    got = hidden_mask(mask, amodal)
    exp = np.zeros((2, S, S), bool)
    exp[0, 1] = True
    exp[1, 0, 1] = True
    assert got.dtype == np.bool_ and np.array_equal(got, exp)
    assert hidden_mask(mask[0], amodal[0]).shape == (S, S)


def test_header_declares_the_entry_point():
    from constructionsceneposeestimation_amd import _lib
    assert "csg_crop_amodal_geometry" in _lib.EXPORTED
    hdr = open(os.path.join(ROOT, "include", "csg_api.h")).read()
    assert re.search(r"\bint\s+csg_crop_amodal_geometry\s*\(\s*csg_ctx\s*\*\s*ctx,\s*const\s+csg_amodal_geometry_job"
                     r"\s*\*\s*job,\s*uint32_t\s+n_frames,\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    assert re.search(r"\}\s*csg_amodal_geometry_job\s*;", hdr)
    assert re.search(r"#define\s+CSG_ABI_VERSION\s+14\b", hdr)
    assert _lib.ABI_VERSION == 14


def test_job_struct_layout_and_null_context():
    from constructionsceneposeestimation_amd import _lib
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "csg_api.h"\nint main(){\n'
            'printf("sizeof %zu\\n", sizeof(csg_amodal_geometry_job));\n'
            'printf("mask_job %zu\\n", sizeof(csg_amodal_job));\n')
    fields = ("size", "per_frame", "frames", "info", "crop_amodal", "crop_amodal_depth", "crop_amodal_coords")
    for m in fields:
        prog += f'printf("{m} %zu\\n", offsetof(csg_amodal_geometry_job, {m}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert C.sizeof(_lib.AmodalGeometryJob) == sizes["sizeof"] == 48
    assert C.sizeof(_lib.AmodalJob) == sizes["mask_job"] == 32
    for m in fields:
        assert getattr(_lib.AmodalGeometryJob, m).offset == sizes[m], m
    lib = _lib.load()
    assert lib.csg_abi_version() == 14
    job = _lib.AmodalGeometryJob(64, 8, None, None, None, None, None)
    assert lib.csg_crop_amodal_geometry(None, C.byref(job), 1, None) == -1
    assert INFO_DTYPE.itemsize == 32
