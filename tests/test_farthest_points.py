"""csg_farthest_points without a GPU: the properties of the NumPy restatement of
the definition (tests/farthest_points_ref.py) -- non-increasing distances,
distinct samples, the covering radius by an independent brute force, prefixes,
ties on a lattice, coincident points, the candidates' stride -- and
farthest_points.py, the header text, the exports, the library's entry point and
the new keyword arguments and flags."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from constructionsceneposeestimation_amd import farthest_points as fp
from tests.farthest_points_ref import (EMPTY, F32, NAN_BITS, brute_cover, candidate_rows, cloud, farthest_points_ref,
                                       fmix32, lattice, run_set, spoil, start_candidate)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs():
    """A few sets run once: (points, m, pool, K, (index, t0, v, dist2))."""
    rng = np.random.default_rng(7)
    sets = [(cloud(rng, 700), 700, 16384, 96), (spoil(rng, cloud(rng, 500), 0.2), 500, 16384, 64),
            (cloud(rng, 3000, 5.0), 3000, 256, 256), (lattice(8), 64, 64, 64),
            (np.repeat(cloud(rng, 40), 3, axis=0), 120, 16384, 80)]
    return [(p, m, pool, K, run_set(p, m, pool, K, seed=3, key=i)) for i, (p, m, pool, K) in enumerate(sets)]


def test_distances_do_not_increase_and_samples_are_distinct(runs):
    for p, m, pool, K, (idx, t0, v, d2) in runs:
        assert 1 <= t0 <= min(K, v)
        assert d2[0] == np.inf and (d2[2:t0] <= d2[1:t0 - 1]).all() and (d2[1:t0] > 0).all()
        assert (d2[t0:] == 0).all()
        assert len(set(idx[:t0].tolist())) == t0
        assert (idx[t0:] == idx[np.arange(t0, K) % t0]).all()
        rows = candidate_rows(m, pool)
        assert np.isin(idx, rows).all() and np.isfinite(p[idx]).all()


def test_every_candidate_lies_within_the_last_distance_of_a_sample(runs):
    for i, (p, m, pool, K, (idx, t0, v, d2)) in enumerate(runs):
        cand = p[candidate_rows(m, pool)]
        cover = brute_cover(cand, p[idx[:t0]])
        if t0 < K:          # the run stopped: every valid candidate coincides with a sample
            assert cover == 0.0
        elif t0 > 1:
            assert cover <= d2[t0 - 1]
        # ... and the next sample would be chosen exactly at the cover
        if t0 == K and K < v:
            longer = run_set(p, m, pool, K + 1, seed=3, key=i)
            assert longer[3][K] == F32(cover)


def test_a_shorter_run_is_a_prefix(runs):
    for i, (p, m, pool, K, (idx, t0, v, d2)) in enumerate(runs):
        for k in (1, 2, t0 // 2 or 1, t0, K):
            short = run_set(p, m, pool, k, seed=3, key=i)
            assert (short[0] == idx[:k]).all() and short[1] == min(t0, k) and short[2] == v
            assert (short[3].view(np.uint32) == d2[:k].view(np.uint32)).all()
    out = farthest_points_ref(np.stack([runs[3][0]] * 2), samples=64, seed=3, set_keys=[3, 9], payloads=[
        np.arange(2 * 64 * 2, dtype=np.uint16).reshape(2, 64, 2)])
    pre = fp.take_prefix({"index": out["index"], "xyz": out["xyz"], "dist2": out["dist2"], "count": out["count"],
                          "tag": out["payloads"][0]}, 16)
    ref = farthest_points_ref(np.stack([runs[3][0]] * 2), samples=16, seed=3, set_keys=[3, 9], payloads=[
        np.arange(2 * 64 * 2, dtype=np.uint16).reshape(2, 64, 2)])
    for k, v in (("index", ref["index"]), ("xyz", ref["xyz"]), ("dist2", ref["dist2"]), ("count", ref["count"]),
                 ("tag", ref["payloads"][0])):
        assert pre[k].shape == v.shape and pre[k].tobytes() == v.tobytes(), k
    whole = fp.take_prefix(out, 16)        # the dict of farthest_points_host, its list of payloads included
    assert sorted(whole) == sorted(ref) and whole["payloads"][0].tobytes() == ref["payloads"][0].tobytes()
    assert all(whole[k].tobytes() == ref[k].tobytes() for k in ("index", "xyz", "dist2", "count"))
    with pytest.raises(ValueError):
        fp.take_prefix({"index": out["index"]}, 65)


def test_lattice_ties_go_to_the_lowest_index():
    p = lattice(8)
    for key in range(6):
        idx, t0, v, d2 = run_set(p, 64, 64, 16, seed=0, key=key)
        assert (t0, v) == (16, 64)
        mind = np.full(64, np.inf, F32)
        for t in range(16):
            if t:
                g = mind.max()
                tied = np.flatnonzero(mind == g)
                assert idx[t] == tied[0] and d2[t] == g
            d = p - p[idx[t]]
            mind = np.minimum(mind, (d * d).sum(axis=1).astype(F32))
    # the chosen distances themselves repeat: ties that were resolved one after the other
    start = start_candidate(np.ones(64, bool), 0, 0)
    idx, t0, v, d2 = run_set(p, 64, 64, 16, seed=0, key=0)
    assert idx[0] == start
    assert any(d2[t] == d2[t + 1] for t in range(1, 15)), "the lattice must meet exact ties"
    # +inf ties: points at +-3e38 are at distance inf from each other; the lowest index goes first
    big = np.array([[3e38, 0, 0], [-3e38, 0, 0], [0, 3e38, 0], [0, -3e38, 0], [0, 0, 0]], F32)
    idx, t0, v, d2 = run_set(big, 5, 5, 5, seed=0, key=0)
    assert t0 == 5 and np.isinf(d2[:2]).all() and (d2[2:] <= d2[1:-1]).all()
    s = int(idx[0])
    rest = [j for j in range(5) if j != s]
    with np.errstate(over="ignore"):
        far = [j for j in rest if np.isinf(((big[j] - big[s]).astype(F32) ** 2).astype(F32).sum(dtype=F32))]
    assert idx[1] == far[0]


def test_coincident_points_give_one_sample():
    p = np.tile(np.array([[1.5, -2.0, 0.25]], F32), (50, 1))
    idx, t0, v, d2 = run_set(p, 50, 16384, 8, seed=1, key=2)
    assert (t0, v) == (1, 50) and (idx == idx[0]).all() and d2[0] == np.inf and (d2[1:] == 0).all()
    out = farthest_points_ref(p[None], samples=8, seed=1, set_keys=[2])
    assert out["count"].tolist() == [[1, 50]] and (out["xyz"][0] == p[0]).all()


def test_empty_sets_and_invalid_starts():
    p = np.full((10, 3), np.nan, F32)
    out = farthest_points_ref(p[None], samples=4, payloads=[np.ones((1, 10, 3), np.uint8)], fills=[0xFF])
    assert out["count"].tolist() == [[0, 0]] and (out["index"] == EMPTY).all()
    assert (out["xyz"].view(np.uint32) == NAN_BITS).all() and (out["dist2"] == 0).all()
    assert (out["payloads"][0] == 0xFF).all()
    out = farthest_points_ref(np.zeros((2, 10, 3), F32), np.array([0, EMPTY], np.uint32), samples=4)
    assert out["count"].tolist() == [[0, 0], [0, 0]]
    # a start that lands on an invalid candidate moves on, cyclically past the end
    q = np.arange(30, dtype=F32).reshape(10, 3)
    c = 10
    for key in range(40):
        h = fmix32(fmix32(key) ^ 0x9E3779B9)
        j0 = (h * c) >> 32
        valid = np.ones(c, bool)
        valid[j0] = False
        if j0 == c - 1:
            valid[0] = False
        want = (j0 + 1) % c if j0 != c - 1 else 1
        assert start_candidate(valid, 0, key) == want
        r = q.copy()
        r[~valid, 1] = np.inf
        assert run_set(r, 10, 16384, 3, seed=0, key=key)[0][0] == want
    assert any(((fmix32(fmix32(k) ^ 0x9E3779B9) * c) >> 32) == c - 1 for k in range(40))


def test_candidate_rows():
    for m, pool in ((0, 5), (1, 1), (5, 5), (5, 16384), (6, 5), (40000, 1000), (16385, 16384), (1 << 24, 16384), (7, 1)):
        r = fp.candidate_rows(m, pool)
        assert r.shape == (min(m, pool),) and (r == candidate_rows(m, pool)).all() if m else r.size == 0
        if m:
            assert r[0] == 0 and r[-1] < m and (np.diff(r) > 0).all()
        if m <= pool:
            assert (r == np.arange(m)).all()
    assert fp.candidate_rows(40000, 1000)[-1] == 39960 and fp.candidate_rows(16385, 16384)[-1] == 16383
    with pytest.raises(ValueError):
        fp.candidate_rows(3, 0)


def test_coverage_radius(runs):
    p, m, pool, K, (idx, t0, v, d2) = runs[0]
    r = fp.coverage_radius(d2[None], np.array([[t0, v]], np.uint32))
    assert r.shape == (1,) and r[0] == np.sqrt(np.float64(d2[t0 - 1]))
    cand = p[candidate_rows(m, pool)]
    assert brute_cover(cand, p[idx[:t0]]) <= r[0] ** 2 * (1 + 1e-6)
    r = fp.coverage_radius(np.array([[np.inf, 0, 0], [0, 0, 0], [np.inf, 4.0, 1.0]], F32), np.array([1, 0, 3]))
    assert np.isinf(r[0]) and np.isnan(r[1]) and r[2] == 1.0


def test_header_exports_and_abi():
    from constructionsceneposeestimation_amd import _lib
    text = open(os.path.join(ROOT, "include", "csg_api.h")).read()
    assert re.search(r"#define CSG_ABI_VERSION 14\b", text) and _lib.ABI_VERSION == 14
    assert "csg_farthest_points" in _lib.EXPORTED
    assert "int csg_farthest_points(csg_ctx* ctx, const csg_fps_job* job, uint32_t n_sets, void* stream);" in text
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("m_s = 0 when counts[s] == 0xFFFFFFFF", "otherwise m_s = min(counts[s], C).",
                   "c_s = min(m_s, P).", "r_j = ((uint64)j * m_s) / c_s",
                   "A candidate is valid iff its three coordinates are finite.",
                   "d2 = fl32(fl32(fl32(dx*dx) + fl32(dy*dy)) + fl32(dz*dz)).",
                   "h = fmix32(fmix32(seed ^ key_s) ^ 0x9E3779B9u)", "j0 = (uint32)(((uint64)h * c_s) >> 32).",
                   "minimises (j + c_s - j0) % c_s", "fp_dist2[s][0] = +inf.", "If g == 0, t0 = t and the run stops",
                   "chooses the lowest j with mind_j == g", "repeat entry t mod t0", "fp_count[s] = {t0, v_s}.",
                   "fp_index all 0xFFFFFFFF", "the bits 0x7FC00000", "dst[s][t] = src[s][fp_index[s][t]]",
                   "an output that overlaps a source or another output", "Returns -1 for a NULL ctx."):
        assert phrase in flat, phrase
    assert re.search(r"#define CSG_FPS_MAX_PAYLOADS 4u", text) and _lib.FPS_MAX_PAYLOADS == 4 == fp.MAX_PAYLOADS
    fields = [f for f, _ in _lib.FpsJob._fields_]
    assert fields == ["rows", "pool", "samples", "seed", "n_payloads", "pad", "xyz", "counts", "set_keys", "fp_index",
                      "fp_xyz", "fp_dist2", "fp_count", "payloads"]
    assert C.sizeof(_lib.FpsPayload) == 24 and C.sizeof(_lib.FpsJob) == 24 + 7 * 8 + 4 * 24
    struct = text[text.index("typedef struct {", text.index("} csg_fps_payload;")):text.index("} csg_fps_job;")]
    names = re.findall(r"(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    assert names == fields
    assert [f for f, _ in _lib.FpsPayload._fields_] == ["src", "dst", "row_bytes", "fill"]


def test_library_has_the_entry_point():
    from constructionsceneposeestimation_amd import _lib
    lib = _lib.load()
    job = _lib.FpsJob()
    assert lib.csg_farthest_points(None, C.byref(job), 1, None) == -1      # a null context
    assert lib.csg_abi_version() == 14


def test_new_arguments_default_to_todays_behaviour():
    from constructionsceneposeestimation_amd.generate import generate, main
    from constructionsceneposeestimation_amd.renderer import Renderer
    sig = inspect.signature(Renderer.render_crops).parameters
    assert sig["sampling"].default == "stratified" and sig["candidates"].default == 4096
    sig = inspect.signature(Renderer.voxel_cloud_host).parameters
    assert (sig["keep"].default, sig["keep_pool"].default, sig["keep_seed"].default, sig["frame_keys"].default) == \
        (0, 16384, 0, None)
    sig = inspect.signature(Renderer.farthest_points).parameters
    assert list(sig)[1:] == ["n_sets", "rows", "pool", "samples", "xyz", "counts", "set_keys", "seed", "fp_index",
                             "fp_xyz", "fp_dist2", "fp_count", "payloads", "stream"]
    assert sig["pool"].default == 16384 and sig["payloads"].default == ()
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[2:])
    sig = inspect.signature(Renderer.farthest_points_host).parameters
    assert list(sig)[1:] == ["xyz", "counts", "samples", "pool", "seed", "set_keys", "payloads"]
    sig = inspect.signature(generate).parameters
    assert sig["voxel_points"].default == 0 and sig["voxel_points_seed"].default == 0
    for argv in (["--voxel-points", "many"], ["--voxel-points-seed", "x"], ["--voxel-points"]):
        with pytest.raises(SystemExit):
            main(["--out", "/nonexistent", "--outputs", "pointcloud_voxel_ply"] + argv)
    with pytest.raises(ValueError):
        generate("/nonexistent", [0], outputs=("pointcloud_voxel_ply",), voxel_points=16385)
