"""bench.py's host-side arithmetic (CPU): rank sharding of the timed steps,
the verified sample, the max-over-ranks elapsed time (gloo, world size 2)
and the roofline / baseline bookkeeping."""
import os
import socket
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_step_frames_are_disjoint_and_fixed_per_rank(world):
    F, W, K = 40, 2, 3
    per_rank = [bench.rank_frames(r, world, W + K, F) for r in range(world)]
    for r, fr in enumerate(per_rank):
        assert len(fr) == (W + K) * F                      # weak scaling: fixed work per rank
        assert all((f // 10) % world == r for f in fr)     # the rank's own epochs only
        assert bench.timed_frames(fr, W, K, F) == fr[W * F:]
    flat = [f for fr in per_rank for f in fr]
    assert len(set(flat)) == len(flat)                     # no frame rendered twice


def test_sample_frames_lie_in_the_last_timed_step():
    F, W, K = 240, 3, 20
    idx = bench.verify_sample_indices(F, 32)
    assert len(idx) == 32 and len(set(idx)) == 32
    assert idx[0] == 0 and idx[-1] == F - 1 and all(0 <= k < F for k in idx)
    assert bench.verify_sample_indices(F, 0) == []
    assert bench.verify_sample_indices(5, 9) == [0, 1, 2, 3, 4]
    fr = bench.rank_frames(0, 1, W + K, F)
    timed = bench.timed_frames(fr, W, K, F)
    last = timed[(K - 1) * F:]
    assert all(last[k] in timed for k in idx)


def test_dump_pixel_sample_is_fixed_and_fits_the_budget():
    import numpy as np
    npix = 2880 * 1920 * 1080                                  # one C3 step: past 2^31 pixels
    a = bench.dump_pixel_sample(npix, 20, bench.DUMP_MAX_BYTES)
    b = bench.dump_pixel_sample(npix, 20, bench.DUMP_MAX_BYTES)
    assert a.dtype == np.int64 and np.array_equal(a, b)        # the same pixels every run
    assert 0.99 * bench.DUMP_MAX_PIXELS < len(a) <= bench.DUMP_MAX_PIXELS
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < npix and a[-1] > 2 ** 31
    # a tighter budget takes fewer pixels, never more bytes than it allows
    c = bench.dump_pixel_sample(npix, 48, 1000 * 48)
    assert 0 < len(c) <= 1000 and len(c) * 48 <= 1000 * 48
    # outputs smaller than the sample are written whole
    assert np.array_equal(bench.dump_pixel_sample(12, 20, bench.DUMP_MAX_BYTES), np.arange(12))
    assert bench.DUMP_MAX_BYTES <= 64 * 1000 * 1000


def test_dump_outputs_writes_float_arrays_of_the_sampled_pixels(tmp_path, monkeypatch):
    import numpy as np
    import torch
    F, H, W, K = 3, 5, 7, 4
    g = torch.Generator().manual_seed(1)
    out = {"rgb": torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, generator=g),
           "instance": torch.randint(-1, 2 ** 31 - 1, (F, H, W), dtype=torch.int32, generator=g),
           "depth": torch.rand((F, H, W), generator=g),
           "normals": torch.rand((F, H, W, 3), generator=g).to(torch.float16),
           "keypoints_uv": torch.rand((F, K, 2), generator=g),
           "keypoints_vis": torch.randint(0, 3, (F, K), dtype=torch.int32, generator=g)}
    shapes = bench.dump_outputs(str(tmp_path / "whole"), out)
    got = {n[:-4]: np.load(tmp_path / "whole" / n) for n in os.listdir(tmp_path / "whole")}
    assert set(got) == set(out) and {k: list(a.shape) for k, a in got.items()} == shapes
    # small outputs: every pixel, in frame / row / column order; ints exact in float64
    assert got["instance"].dtype == np.float64 and got["keypoints_vis"].dtype == np.float64
    assert all(got[k].dtype == np.float32 for k in ("rgb", "depth", "normals", "keypoints_uv"))
    assert np.array_equal(got["rgb"], out["rgb"].numpy().reshape(-1, 3).astype(np.float32))
    assert np.array_equal(got["instance"], out["instance"].numpy().reshape(-1).astype(np.float64))
    assert np.array_equal(got["depth"], out["depth"].numpy().reshape(-1))
    assert np.array_equal(got["normals"], out["normals"].numpy().reshape(-1, 3).astype(np.float32))
    assert np.array_equal(got["keypoints_uv"], out["keypoints_uv"].numpy())
    assert np.array_equal(got["keypoints_vis"], out["keypoints_vis"].numpy().astype(np.float64))
    # a sample: the same pixels of every per-pixel output, keypoints still whole
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 20)
    idx = bench.dump_pixel_sample(F * H * W, 1, 1 << 20)
    assert 0 < len(idx) <= 20
    bench.dump_outputs(str(tmp_path / "part"), out)
    part = {n[:-4]: np.load(tmp_path / "part" / n) for n in os.listdir(tmp_path / "part")}
    assert np.array_equal(part["rgb"], got["rgb"][idx]) and np.array_equal(part["instance"], got["instance"][idx])
    assert np.array_equal(part["depth"], got["depth"][idx]) and np.array_equal(part["normals"], got["normals"][idx])
    assert np.array_equal(part["keypoints_uv"], got["keypoints_uv"])


def test_prep_worker_count_follows_the_cpu_share():
    n = bench.prep_worker_count
    big = bench.PREP_MIN_EPOCHS
    assert n(-1, big, 1, {"OMP_NUM_THREADS": "16"}) == 16
    assert n(-1, big, 1, {"OMP_NUM_THREADS": "64"}) == bench.PREP_WORKERS_MAX
    assert n(-1, big, 8, {"OMP_NUM_THREADS": "16"}) == 2          # the ranks of a node share its CPUs
    assert n(-1, big, 16, {"OMP_NUM_THREADS": "16"}) == 0
    assert n(-1, big - 1, 1, {"OMP_NUM_THREADS": "16"}) == 0      # a short schedule: computed in this process
    assert n(3, 1, 1, {}) == 3 and n(0, big, 1, {"OMP_NUM_THREADS": "16"}) == 0
    # never under a profiler: its preloaded library would load in every worker
    assert n(-1, big, 1, {"OMP_NUM_THREADS": "16", "ROCPROF_OUTPUT_PATH": "x"}) == 0
    assert n(4, big, 1, {"LD_PRELOAD": "librocprofiler-sdk-tool.so"}) == 0


def test_schedule_from_worker_processes_equals_this_process():
    """The epochs and cameras the workers compute are, bit for bit, those of
    Workload.epoch / frame_params here, chunk by chunk in schedule order."""
    import numpy as np
    from constructionsceneposeestimation_amd.workload import Workload
    wl = Workload("C4", seed=3, width=64, height=36)              # C4: the DR light and textures travel too
    fids = bench.rank_frames(1, 2, 2, 24)                         # 48 frames: epochs straddle the chunks below
    assert [len(c) for c in bench.prep_chunks(fids, 32)] == [32, 16]
    here = list(bench.SchedulePrep(wl, "C4", 3, fids, 0).chunks())
    there = list(bench.SchedulePrep(wl, "C4", 3, fids, 2).chunks())
    assert len(here) == len(there) == len(bench.prep_chunks(fids)) == 1
    v, p = Workload("C4", seed=3, width=64, height=36).frame_params(fids)
    for (sa, va, pa), (sb, vb, pb) in zip(here, there):
        assert np.array_equal(va, vb) and np.array_equal(pa, pb) and np.array_equal(va, v) and np.array_equal(pa, p)
        assert list(sa) == list(sb) == sorted({f // 10 for f in fids})
        for e in sa:
            assert np.array_equal(sa[e].models, sb[e].models) and np.array_equal(sa[e].keypoints, sb[e].keypoints)
            assert np.array_equal(sa[e].dr.light.sun_dir, sb[e].dr.light.sun_dir)
            assert sa[e].dr.textures == sb[e].dr.textures


def test_value_is_aggregate_over_ranks():
    assert bench.aggregate_value(steps=20, frames_per_step=240, world=8, elapsed_max=2.0) == 20 * 240 * 8 / 2.0


def test_roofline_formula_follows_survey_8d():
    M = 10 ** 6
    r = bench.roofline(b_geom=1000 * M, b_tex=200 * M, b_out=300 * M, frames_per_launch=10, raster_ms=2.0,
                       setup_ms=1.0, records_per_frame=5 * M, fps=1000.0, traffic={"k_raster": 99})
    b_frame = 1500 * M
    # headline: BASELINE.md:44, fps x B_frame / peak
    assert r["B_frame"] == b_frame
    assert r["achieved"] == pytest.approx(1000.0 * b_frame / 1e9, rel=1e-3)
    assert r["frac"] == pytest.approx(1000.0 * b_frame / (bench.HBM_PEAK_GBS * 1e9), rel=1e-3)
    assert r["traffic"] == 99 and r["bound"] == "hbm" and r["unit"] == "GB/s" and r["avg_launch_ms"] == 2.0
    own, whole, setup = r["kernels"]
    assert own["kernel"] == whole["kernel"] == "k_raster" and setup["kernel"] == "k_setup"
    assert own["bytes_per_launch"] == 10 * (200 + 300) * M
    assert whole["bytes_per_launch"] == 10 * b_frame
    assert whole["achieved"] == pytest.approx(10 * b_frame / 2e-3 / 1e9, rel=1e-3)
    assert setup["bytes_per_launch"] == (1000 + 10 * 5 * bench.RECORD_BYTES) * M   # geometry once per launch


def test_median_timing_runs_warmup_then_five():
    calls = []
    t = bench.median_time(lambda: calls.append(1), runs=5, warmup=1)
    assert len(calls) == 6 and t >= 0.0


def test_cpu_description_is_recorded():
    assert bench.available_cpus() >= 1
    assert isinstance(bench.cpu_model(), str) and bench.cpu_model()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got = bench.max_over_ranks(0.5 + rank, world)
    tot = bench.sum_over_ranks([4, rank], world)
    if rank == 0:
        with open(out, "w") as fh:
            fh.write(repr((got, tot)))
    dist.barrier()
    dist.destroy_process_group()


def test_elapsed_is_max_and_counts_sum_over_ranks_gloo(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "res.txt")
    mp.spawn(_rank_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got, tot = eval(open(out).read())
    assert got == 1.5 and tot == [8, 1]


def test_default_frames_per_step_by_frame_size():
    assert bench.default_frames_per_step(1920, 1080) == bench.DEFAULT_FRAMES_PER_STEP
    assert bench.default_frames_per_step(3840, 2160) == bench.LARGE_FRAMES_PER_STEP < bench.DEFAULT_FRAMES_PER_STEP


def test_shard_report_single_rank_and_gloo_pair(tmp_path):
    import bench
    r = bench.shard_report(list(range(20, 40)), 1)
    assert r == {"ranks": 1, "timed_frames_per_rank": [20], "union": 20, "disjoint": True,
                 "epochs_mod_world": [[0]]}
    import torch.multiprocessing as mp
    mp.spawn(_shard_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    import json
    rep = json.load(open(tmp_path / "rep.json"))
    assert rep["disjoint"] and rep["union"] == 2 * 3 * 20 and rep["epochs_mod_world"] == [[0], [1]]
    # two ranks on the one device of a rehearsal box say so
    assert [d["rank"] for d in rep["devices"]] == [0, 1]
    assert rep["distinct_devices"] == 1 and rep["shared_devices"] is True
    # each rank's own timing, gathered: which rank set elapsed_max, by how much
    assert [p["rank"] for p in rep["per_rank"]] == [0, 1]
    assert rep["per_rank"][1]["stage_ms_per_step"]["ms_raster"] == 11.0
    assert rep["slowest_rank"] == 1 and rep["imbalance"] == 1.25
    # every rank's host-delivery leg: per-rank rates and the aggregate over the slowest rank's time
    dl = json.load(open(tmp_path / "delivery.json"))
    assert dl["ranks"] == 2 and [x["rank"] for x in dl["per_rank"]] == [0, 1]
    assert dl["value"] == round((480 + 480) / 2.0, 2)
    assert dl["per_rank"][0]["frames_per_s"] == 320.0 and dl["per_rank"][1]["frames_per_s"] == 240.0
    assert dl["wire_gbs"] == round((480 + 480) * 8.0e6 / 2.0 / 1e9, 2)
    assert bench.gather_delivery(None, 1) is None


def _shard_worker(rank, port, out_dir):
    import json
    import os
    import torch.distributed as dist
    import bench
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    fids = bench.rank_frames(rank, 2, 4, 20)
    dev = {"rank": rank, "local_rank": rank, "device": 0, "device_count": 1, "pci": "0000:05:00"}
    mine = {"rank": rank, "elapsed_s": 2.0 + 0.5 * rank, "frames_per_s": 30.0 / (2.0 + 0.5 * rank),
            "stage_ms_per_step": {"ms_setup": 1.0, "ms_bin": 0.5, "ms_raster": 10.0 + rank, "ms_keypoints": 0.1}}
    rep = bench.shard_report(bench.timed_frames(fids, 1, 3, 20), 2, dev, mine)
    leg = {"frames": 480, "seconds": 1.5 + 0.5 * rank, "wire_bytes": 480 * 8.0e6, "delivered_bytes": 480 * 14.5e6}
    dl = bench.gather_delivery(leg, 2)
    if rank == 0:
        json.dump(rep, open(os.path.join(out_dir, "rep.json"), "w"))
        json.dump(dl, open(os.path.join(out_dir, "delivery.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


_CHILD = r"""
import os, sys, time
r, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
assert os.environ["LOCAL_RANK"] == str(r) and os.environ["MASTER_ADDR"] == "127.0.0.1"
assert int(os.environ["MASTER_PORT"]) > 0
mode = sys.argv[1]
if mode == "fail" and r == n - 1:
    sys.stderr.write("rank failing on purpose\n")
    sys.exit(7)
if mode == "crash" and r == 1:
    os.kill(os.getpid(), 9)
if mode in ("fail", "crash", "hang"):
    time.sleep(120 if mode == "hang" or r == 0 else 0)   # the others wait: they must be stopped
print("noise that is not a result line")
if r == 0:
    print('{"n_gpus": %d, "rank": 0}' % n, flush=True)
"""


def _launch(mode, n, tmp_path):
    import io
    import time as _t
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    buf = io.StringIO()
    t0 = _t.time()
    rc = bench.launch_ranks(n, [sys.executable, str(script), mode], env=dict(os.environ), out=buf,
                            poll_s=0.05, grace_s=5.0)
    return rc, buf.getvalue(), _t.time() - t0


@pytest.mark.parametrize("n", [2, 4])
def test_launcher_forwards_rank0_line(tmp_path, n):
    """A plain `bench.py --gpus N` starts N ranks itself: each child sees its
    RANK / LOCAL_RANK and the shared WORLD_SIZE / MASTER_*, and only rank 0's
    JSON line is forwarded."""
    env_before = dict(os.environ)
    rc, out, _ = _launch("ok", n, tmp_path)
    assert rc == 0
    assert out.splitlines() == ['{"n_gpus": %d, "rank": 0}' % n]
    assert dict(os.environ) == env_before          # the parent's environment is untouched


@pytest.mark.parametrize("mode,code", [("fail", 7), ("crash", 1)])
def test_launcher_failing_child_gives_no_line(tmp_path, mode, code):
    """Any failing rank -- an error exit, or a rank killed by a signal --
    stops the other ranks (rank 0 sleeps 120 s here), and the launcher exits
    non-zero without printing a line."""
    rc, out, dt = _launch(mode, 3, tmp_path)
    assert rc == code and out == ""
    assert dt < 60


def test_bench_main_launches_ranks_without_torchrun(tmp_path, monkeypatch):
    """`main()` with --gpus 2 and no WORLD_SIZE hands over to launch_ranks
    before importing torch, passing its own arguments to the children."""
    seen = {}

    def fake(n, argv, **kw):
        seen["n"], seen["argv"] = n, argv
        return 5
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench, "launch_ranks", fake)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3"])
    with pytest.raises(SystemExit) as ex:
        bench.main()
    assert ex.value.code == 5 and seen["n"] == 2
    assert seen["argv"][0] == sys.executable and seen["argv"][1].endswith("bench.py")
    assert seen["argv"][2:] == ["--gpus", "2", "--steps", "3"]


def test_shard_report_devices():
    r = bench.shard_report([1, 2], 1, {"rank": 0, "local_rank": 0, "device": 0, "device_count": 1, "pci": "0000:05:00"})
    assert r["devices"][0]["pci"] == "0000:05:00" and r["distinct_devices"] == 1 and r["shared_devices"] is False


@pytest.mark.parametrize("steps,warmup", [(20, 5), (10, 2), (200, 10)])
def test_transform_sets_fit_the_library_for_driver_runs(steps, warmup):
    """Every randomisation epoch of a rank's schedule takes one transform set:
    at the default 2,880 frames per step the driver's `--steps 20 --warmup 5`
    needs 7,200 sets (past round 4's first limit of 4,096); the library holds
    MAX_SETS and the bench fails early, with a message, beyond that."""
    F = bench.DEFAULT_FRAMES_PER_STEP
    fids = bench.rank_frames(0, 1, steps + warmup, F)
    assert len({f // 10 for f in fids}) <= bench.MAX_SETS
    src = open(os.path.join(os.path.dirname(bench.__file__), "constructionsceneposeestimation_amd", "csrc",
                            "csg_api.cpp")).read()
    assert f"constexpr uint32_t kMaxSets = {bench.MAX_SETS};" in src


def test_profiler_preload_is_detected():
    """`rocprofv3 --pmc -- python bench.py --gpus N` would start the
    ranks from a process the profiler's preload already initialised the GPU in."""
    assert bench.profiler_preload({}) is None
    assert bench.profiler_preload({"LD_PRELOAD": "/usr/lib/libfoo.so"}) is None
    assert bench.profiler_preload({"LD_PRELOAD": "/opt/rocm/lib/librocprofiler-sdk-tool.so"})
    assert bench.profiler_preload({"ROCPROF_OUTPUT_PATH": "/tmp/x"})


def test_plain_multi_gpu_bench_refuses_under_a_profiler(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("ROCPROF_OUTPUT_PATH", "/tmp/x")
    called = []
    monkeypatch.setattr(bench, "launch_ranks", lambda *a, **k: called.append(a) or 0)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and not called
