#!/usr/bin/env python3
"""Benchmark: annotated frames/s of the render + annotate hot path on MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``.  For
N > 1 it runs one process per GPU: either launched once per GPU by
``torch.distributed.run`` (RANK / WORLD_SIZE in the environment), or -- a
plain ``python bench.py --gpus N`` -- this process starts the N ranks itself
as fresh child processes before anything touches the GPU (``launch_ranks``),
waits for all of them and forwards rank 0's line; if any rank fails it exits
non-zero with no line.  One *step*
= one batch of ``--frames-per-step`` frames of workload C3 (BASELINE.json
configs[2]: world2 + rigged-human proxies, 1920x1080, RGB + instance
segmentation + 2D keypoints) rendered into HBM-resident output buffers.

Frames are seed-sharded: rank r owns randomisation epochs e = r (mod N),
10 frames per epoch, so per-GPU work is fixed as N grows ("weak" scaling)
and no collective touches the data path; the only inter-rank traffic is the
gloo barrier, the max-over-ranks of the elapsed time and the verification
counts.

A plain run does what the headline figure needs and no more: it sets up,
warms up, times the K steps, writes the last timed step's outputs if
``--dump-outputs DIR`` is given, and prints the line.  The library's overflow
word is sticky across asynchronous batches, so the ``synchronize()`` after
the timed loop fails if any warm-up or timed batch truncated its records or
bin lists (no line is printed).  ``roofline`` (BASELINE.md:44 / SURVEY §8(d):
fps x B_frame / 8 TB/s, plus per-kernel entries priced against the average
launch of each kernel) comes from the HIP events the library records on its
stream during the timed steps, so it takes no run of its own.

``--full`` adds the legs that take runs of their own, after the timed steps:
* frames of the last timed step are rendered again by the CPU oracle and
  compared byte for byte with what the GPU wrote during the timed region
  (RGB, instance ids, keypoint uv bits and visibility); any difference
  aborts the run.  On rank 0 at N=1 the same oracle runs are
  ``cpu_baseline`` (oracle/csg_oracle.c, a port of the same arithmetic --
  the reference has no CPU render path -- single-thread and on the box's CPU
  share, median of 5 after a warm-up, wall clock without file I/O);
* ``with_label_stats``: batches timed with label statistics, occlusion
  coverage and the depth visualisation;
* ``pcie_inclusive``: batches timed with host outputs.
Without ``--full`` those fields are null and ``verified.frames`` is 0.

``--dump-outputs DIR`` writes what the last timed step left in the output
buffers as ``DIR/<name>.npy``: the keypoint arrays of every frame of the
step whole, and of each per-pixel output the same fixed, seeded sample of
pixels (``dump_pixel_sample``), float32 (float64 for the int32 outputs, so
every id is exact), at most 64 MB in all.  The schedule is a function of the
arguments alone, so two builds run with the same arguments write arrays that
can be compared element for element.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from typing import Callable, Dict, List, Optional

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "annotated frames/sec (RGB+seg+2D kpts) at 1920×1080, 1/2/4/8 MI355X"
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec (MI355X_MICROARCH.md)
RECORD_BYTES = 80 + 4  # k_setup writes one 80-B raster record + its 4-B tile rectangle per record
# 2,880 frames per step = one launch chain: the kernels' ramp-down and the
# short kernels' fixed cost are paid once per launch (C3 frames/s with the work
# buffers sized by csg_size_work: 960 -> 22.62k, 1,920 -> 22.80k, 2,880 ->
# 22.90k, 3,840 -> 22.92k; profiles/r04/ab/frames_per_step.txt).  At 2,880 a
# rank holds ~68 GB of work buffers and ~42 GB of outputs on its 288-GB GPU.
DEFAULT_STEPS, DEFAULT_WARMUP, DEFAULT_FRAMES_PER_STEP = 10, 2, 2880
# Larger frames (C5 at 3840x2160 with depth, normals and points: ~240 MB of
# outputs per frame) take 480 frames per step (240 -> 6.30k, 480 -> 6.34k
# frames/s): ~115 GB of outputs and ~16 GB of work per rank.
LARGE_FRAME_PIXELS, LARGE_FRAMES_PER_STEP = 1920 * 1080, 480
MAX_SETS = 65536   # transform sets per context (kMaxSets, csg_api.cpp)
# Host-delivery batches at N > 1 (every rank at once): 480 frames of C3 are
# ~7 GB of pinned host outputs per rank, ~56 GB for the 8 ranks of a node.
PCIE_FRAMES_MULTI = 480
# --dump-outputs: bytes of all files together, and the most pixels sampled
DUMP_MAX_BYTES, DUMP_MAX_PIXELS, DUMP_SEED = 60 << 20, 1 << 20, 0x5EED
# schedule preparation in worker processes: from this many epochs on, at most this many workers
PREP_MIN_EPOCHS, PREP_WORKERS_MAX = 512, 16


def default_frames_per_step(width: int, height: int) -> int:
    return DEFAULT_FRAMES_PER_STEP if width * height <= LARGE_FRAME_PIXELS else LARGE_FRAMES_PER_STEP


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# ---------------------------------------------------------------------------
# host arithmetic (unit-tested on CPU: tests/test_bench_logic.py)
# ---------------------------------------------------------------------------

def rank_frames(rank: int, world: int, steps: int, frames_per_step: int) -> List[int]:
    """Frame ids of every step of ``rank``: the epoch-interleaved seed shard
    (SURVEY §8e), ``steps * frames_per_step`` frames, step s = slice s."""
    from constructionsceneposeestimation_amd.shard import shard_frames
    return shard_frames(rank, world, steps * frames_per_step)


def timed_frames(fids: List[int], warmup: int, steps: int, frames_per_step: int) -> List[int]:
    return fids[warmup * frames_per_step:(warmup + steps) * frames_per_step]


def verify_sample_indices(frames_per_step: int, n: int) -> List[int]:
    """``n`` distinct frame slots of one step, evenly spread, first and last included."""
    n = max(0, min(n, frames_per_step))
    if n == 0:
        return []
    if n == 1:
        return [frames_per_step - 1]
    return [int(round(k * (frames_per_step - 1) / (n - 1))) for k in range(n)]


def dump_pixel_sample(n_pixels_total: int, bytes_per_pixel: int, budget: int) -> np.ndarray:
    """Flat pixel indices (frame-major, row, column) of the ``--dump-outputs``
    sample: sorted, distinct, drawn with a fixed seed, as many as ``budget``
    bytes hold at ``bytes_per_pixel`` (at most DUMP_MAX_PIXELS, and every
    pixel if the outputs are that small)."""
    n = int(max(0, min(DUMP_MAX_PIXELS, budget // max(bytes_per_pixel, 1), n_pixels_total)))
    if n == n_pixels_total:
        return np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(DUMP_SEED)
    idx = np.unique(rng.integers(0, n_pixels_total, size=n, dtype=np.int64))
    return idx


def dump_outputs(out_dir: str, dev_out: dict) -> dict:
    """Write the step's outputs (``dev_out``: name -> device tensor, frames
    first) as ``out_dir/<name>.npy``.  Keypoint arrays whole; per-pixel
    arrays at the pixels of ``dump_pixel_sample``.  Integer outputs as
    float64 (exact for every int32), the others as float32."""
    import torch
    os.makedirs(out_dir, exist_ok=True)

    def as_float(t):
        return t.to(torch.float64 if t.dtype in (torch.int32, torch.int64) else torch.float32)

    small = {k: t for k, t in dev_out.items() if k.startswith("keypoints")}
    images = {k: t for k, t in dev_out.items() if k not in small}
    written = {}
    used = 0
    for k, t in small.items():
        a = as_float(t).cpu().numpy()
        used += a.nbytes
        written[k] = a
    if used > DUMP_MAX_BYTES:
        raise SystemExit(f"bench: --dump-outputs: the keypoint arrays alone hold {used} bytes")
    if images:
        first = next(iter(images.values()))
        npix = first.shape[0] * first.shape[1] * first.shape[2]
        per_px = sum((8 if t.dtype in (torch.int32, torch.int64) else 4) * (t.shape[3] if t.dim() == 4 else 1)
                     for t in images.values())
        idx = dump_pixel_sample(npix, per_px, DUMP_MAX_BYTES - used)
        ix = torch.from_numpy(idx).to(first.device)
        for k, t in images.items():
            flat = t.reshape(npix, -1) if t.dim() == 4 else t.reshape(npix)
            written[k] = as_float(flat.index_select(0, ix)).cpu().numpy()
    for k, a in written.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    return {k: list(a.shape) for k, a in written.items()}


def aggregate_value(steps: int, frames_per_step: int, world: int, elapsed_max: float) -> float:
    """Whole-job frames/s: every rank renders ``steps * frames_per_step`` frames."""
    return steps * frames_per_step * world / elapsed_max


def max_over_ranks(x: float, world: int) -> float:
    if world <= 1:
        return float(x)
    import torch
    import torch.distributed as dist
    t = torch.tensor([float(x)], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(vals: List[int], world: int) -> List[int]:
    if world <= 1:
        return [int(v) for v in vals]
    import torch
    import torch.distributed as dist
    t = torch.tensor([int(v) for v in vals], dtype=torch.int64)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return [int(v) for v in t.tolist()]


def shard_report(timed: List[int], world: int, device: Optional[dict] = None, per_rank: Optional[dict] = None) -> dict:
    """Each rank's timed frame ids gathered on every rank (gloo): the seed
    shards must be disjoint, and their union is what ``value`` counts.
    ``device`` (this rank's GPU: ordinal, the process's device count, PCI
    address) is gathered beside them, so a line proves N ranks on N distinct
    devices -- or says that ranks shared one (a rehearsal on a smaller box).
    ``per_rank`` (this rank's own timing: elapsed seconds of the timed steps,
    per-stage ms per step, frames/s) is gathered likewise, so an N > 1 line
    shows which rank set ``elapsed_max`` and by how much (``imbalance`` =
    slowest / fastest rank's elapsed time)."""
    lists = [(list(timed), device, per_rank)]
    if world > 1:
        import torch.distributed as dist
        lists = [None] * world
        dist.all_gather_object(lists, (list(timed), device, per_rank))
    sets = [set(x) for x, _, _ in lists]
    union = set().union(*sets)
    rep = {"ranks": world, "timed_frames_per_rank": [len(x) for x, _, _ in lists],
           "union": len(union), "disjoint": len(union) == sum(len(x) for x, _, _ in lists),
           "epochs_mod_world": [sorted({(f // 10) % world for f in x}) for x, _, _ in lists]}
    devs = [d for _, d, _ in lists]
    if all(d is not None for d in devs):
        ids = [d.get("pci") or d["device"] for d in devs]
        rep["devices"] = devs
        rep["distinct_devices"] = len(set(ids))
        rep["shared_devices"] = len(set(ids)) < world
    prs = [p for _, _, p in lists]
    if all(p is not None for p in prs):
        rep["per_rank"] = prs
        el = [p["elapsed_s"] for p in prs if p.get("elapsed_s")]
        if el:
            rep["slowest_rank"] = max(range(len(prs)), key=lambda k: prs[k].get("elapsed_s") or 0.0)
            rep["imbalance"] = round(max(el) / min(el), 4)
    return rep


def gather_delivery(mine: Optional[dict], world: int) -> Optional[dict]:
    """Host delivery at N > 1: every rank timed its own leg, all started at one
    barrier.  Per-rank frames/s and GB/s, and the aggregate the N ranks
    delivered together into host memory: all ranks' frames over the slowest
    rank's time (what a user of the node's N GPUs gets)."""
    legs = [mine]
    if world > 1:
        import torch.distributed as dist
        legs = [None] * world
        dist.all_gather_object(legs, mine)
    if any(x is None for x in legs):
        return None
    t = max(x["seconds"] for x in legs)
    frames = sum(x["frames"] for x in legs)
    return {"value": round(frames / t, 2), "unit": "frames/s",
            "wire_gbs": round(sum(x["wire_bytes"] for x in legs) / t / 1e9, 2),
            "delivered_gbs": round(sum(x["delivered_bytes"] for x in legs) / t / 1e9, 2),
            "per_rank": [{"rank": k, "frames_per_s": round(x["frames"] / x["seconds"], 2),
                          "wire_gbs": round(x["wire_bytes"] / x["seconds"] / 1e9, 2), "frames": x["frames"],
                          "seconds": round(x["seconds"], 4)} for k, x in enumerate(legs)],
            "ranks": world}


# ---------------------------------------------------------------------------
# N ranks from a plain `python bench.py --gpus N` (no torchrun in front)
# ---------------------------------------------------------------------------

def free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _die_with_parent():   # pragma: no cover - runs in the forked child before exec
    try:
        import ctypes
        import signal
        ctypes.CDLL("libc.so.6", use_errno=True).prctl(1, signal.SIGKILL)   # PR_SET_PDEATHSIG
    except Exception:
        pass


def launch_ranks(n: int, child_argv: List[str], env: Optional[Dict[str, str]] = None,
                 out=None, poll_s: float = 0.2, grace_s: float = 10.0) -> int:
    """Start ``n`` fresh child processes running ``child_argv`` -- one rank
    each, RANK = LOCAL_RANK = r, WORLD_SIZE = n, MASTER_ADDR 127.0.0.1 and a
    free MASTER_PORT -- wait for all of them, and write rank 0's JSON line(s)
    to ``out`` (stdout).  The children are started with ``subprocess`` (never
    exec) from a process that has not touched the GPU; their stderr is
    inherited, their stdout captured.  If any child fails, the others are
    terminated (their own PIDs only), nothing is written and the return code
    is non-zero (the first failure's, or 1)."""
    import subprocess
    import tempfile
    out = out or sys.stdout
    base = dict(os.environ if env is None else env)
    base.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), WORLD_SIZE=str(n),
                LOCAL_WORLD_SIZE=str(n), GROUP_RANK="0", ROLE_RANK="0", ROLE_WORLD_SIZE=str(n))
    procs, files = [], []
    try:
        for r in range(n):
            e = dict(base, RANK=str(r), LOCAL_RANK=str(r), ROLE_RANK=str(r))
            fh = tempfile.TemporaryFile(mode="w+")
            files.append(fh)
            procs.append(subprocess.Popen(child_argv, env=e, stdout=fh, stderr=None, preexec_fn=_die_with_parent))
        failed = 0
        while True:
            codes = [p.poll() for p in procs]
            bad = [c for c in codes if c not in (None, 0)]
            if bad:
                failed = bad[0]
                break
            if all(c == 0 for c in codes):
                break
            time.sleep(poll_s)
        if failed:
            log(f"bench: a rank failed (exit {failed}); stopping the other ranks, no result")
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            t_end = time.time() + grace_s
            for p in procs:
                try:
                    p.wait(timeout=max(0.1, t_end - time.time()))
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()
            return failed if failed > 0 else 1
        files[0].seek(0)
        lines = [ln for ln in files[0].read().splitlines() if ln.startswith("{")]
        if not lines:
            log("bench: rank 0 printed no result line")
            return 1
        for ln in lines:
            print(ln, file=out, flush=True)
        return 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        for fh in files:
            fh.close()


def profiler_preload(env: Dict[str, str]) -> Optional[str]:
    """Why this process is running under rocprofv3 (its preloaded library
    initialises the GPU before main), or None."""
    pre = env.get("LD_PRELOAD", "")
    if "rocprof" in pre or "roctracer" in pre:
        return "LD_PRELOAD names the profiler"
    for k in env:
        if k.startswith("ROCPROF_") or k.startswith("ROCPROFILER_"):
            return f"{k} is set"
    return None


def prep_worker_count(requested: int, n_epochs: int, world: int, env: Dict[str, str]) -> int:
    """Worker processes that compute the schedule's epochs and cameras.  ``requested`` >= 0 is taken as given; -1 = this rank's
    share of the CPUs (OMP_NUM_THREADS where it is set, else the CPUs this
    process may use; at most PREP_WORKERS_MAX) for schedules of at least
    PREP_MIN_EPOCHS epochs, else none: a short schedule is computed in this
    process sooner than workers start.  Never under a profiler, whose preloaded
    library every child process would load too."""
    if profiler_preload(env):
        return 0
    if requested >= 0:
        return requested
    if n_epochs < PREP_MIN_EPOCHS:
        return 0
    cpus = int(env.get("OMP_NUM_THREADS") or 0) or available_cpus()
    n = min(PREP_WORKERS_MAX, cpus // max(world, 1))
    return n if n >= 2 else 0


def prep_chunks(fids: List[int], chunk: int = 320) -> List[List[int]]:
    """The schedule's frames in runs of ``chunk``, one task each."""
    return [fids[k:k + chunk] for k in range(0, len(fids), chunk)]


_PREP_WL = None   # a worker process's own Workload


def _prep_init(workload: str, seed: int, width: int, height: int) -> None:
    """Worker initialiser (as prep_pool.init): the same scene, the same seed."""
    global _PREP_WL
    from constructionsceneposeestimation_amd.workload import Workload
    _PREP_WL = Workload(workload, seed=seed, width=width, height=height)


def _prep_chunk(wl, frames: List[int]):
    """What the bench uploads for a run of frames: its epochs' states (instance
    transforms, keypoints, DR; not the object frames and joints, which only
    labels need) and its frames' view and projection matrices."""
    import dataclasses
    wl = wl or _PREP_WL
    views, projs = wl.frame_params(frames)
    states = {e: dataclasses.replace(wl.epoch(e), object_frames=[], joints={}) for e in sorted({f // 10 for f in frames})}
    return states, views, projs


class SchedulePrep:
    """The schedule's epoch states and camera matrices.  With ``workers`` > 0
    they are computed by worker processes (as prep_pool.py does for the
    generator: each worker builds its own Workload from the same arguments,
    so the same numbers), started by ``__init__`` -- call it before this
    process touches the GPU -- and handed out by ``chunks``; with none,
    ``chunks`` computes them here."""

    def __init__(self, wl, workload: str, seed: int, fids: List[int], workers: int):
        self.wl, self.todo, self.pool, self.futs = wl, prep_chunks(fids), None, []
        if workers > 0:
            import multiprocessing as mp
            from concurrent.futures import ProcessPoolExecutor
            self.pool = ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn"),
                                            initializer=_prep_init, initargs=(workload, seed, wl.width, wl.height))
            self.futs = [self.pool.submit(_prep_chunk, None, c) for c in self.todo]

    def chunks(self):
        """Per run of frames, in schedule order: (epoch -> EpochState of the
        run's epochs, views, projs of its frames)."""
        if self.pool is None:
            for c in self.todo:
                yield _prep_chunk(self.wl, c)
            return
        try:
            for fut in self.futs:
                yield fut.result()
        finally:
            self.pool.shutdown(wait=True, cancel_futures=True)


def median_time(fn: Callable[[], None], runs: int = 5, warmup: int = 1, what: str = "") -> float:
    """Median wall time of ``runs`` calls after ``warmup`` untimed ones.
    A progress line per call (stderr): a long CPU baseline is not silent."""
    for _ in range(warmup):
        fn()
    ts = []
    for k in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if what:
            log(f"cpu baseline {what}: run {k + 1}/{runs} {ts[-1]:.2f} s")
    return statistics.median(ts)


def roofline(b_geom: int, b_tex: int, b_out: int, frames_per_launch: float, raster_ms: float, setup_ms: float,
             records_per_frame: float, fps: float, traffic: Optional[Dict[str, int]] = None) -> dict:
    """SURVEY §8(d) / BASELINE.md:44: B_frame = B_geom + B_tex + B_out per
    frame, and the headline fraction is ``fps x B_frame / 8 TB/s`` with fps
    the per-GPU rate of the timed steps.  ``kernels`` prices the dominant
    kernel (k_raster, whose average launch the HIP events on its stream
    measure; rocprofv3 in profiles/ agrees) two ways -- its own algorithmic
    bytes (B_out + B_tex) and the whole B_frame per launch -- and k_setup by
    its own bytes."""
    traffic = traffic or {}
    b_frame = b_geom + b_tex + b_out
    achieved = fps * b_frame / 1e9

    def kern(name, nbytes, ms, what):
        a = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        return {"kernel": name, "bytes_per_launch": int(nbytes), "avg_launch_ms": round(ms, 4),
                "achieved": round(a, 2), "frac": round(a / HBM_PEAK_GBS, 5), "traffic": traffic.get(name),
                "bytes": what}

    kernels = [
        kern("k_raster", round(frames_per_launch * (b_tex + b_out)), raster_ms,
             "own bytes: B_out + B_tex (outputs written once, bound textures read once) per launch"),
        kern("k_raster", round(frames_per_launch * b_frame), raster_ms,
             "B_frame x frames per launch against k_raster's launch alone (the round-2 headline; it counts "
             "B_geom, which k_setup reads)"),
        kern("k_setup", round(b_geom + frames_per_launch * records_per_frame * RECORD_BYTES), setup_ms,
             "B_geom once per launch (the launch's frames share the geometry through L2 and the Infinity "
             "Cache: the grid runs frame-fast) + 84 B written per raster record: the 80-B record and its 4-B tile rectangle"),
    ]
    return {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic.get("k_raster"),
            "kernel": "k_raster", "avg_launch_ms": round(raster_ms, 4), "frames_per_launch": frames_per_launch,
            "formula": "fps (per GPU, timed steps) x B_frame / 8 TB/s (BASELINE.md:44, SURVEY §8(d)); "
                       "traffic = k_raster's PMC HBM bytes per launch",
            "B_frame": int(b_frame), "B_geom": int(b_geom), "B_tex": int(b_tex), "B_out": int(b_out),
            "kernels": kernels}


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown"


def device_pci(ordinal: int) -> Optional[str]:
    """PCI address of GPU ``ordinal`` (domain:bus:device), or None."""
    try:
        import torch
        p = torch.cuda.get_device_properties(ordinal)
        return f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}"
    except Exception:
        return None


def available_cpus() -> int:
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        return os.cpu_count() or 1


# ---------------------------------------------------------------------------
# oracle check of the timed outputs (checker only: tests/, smoke() and this leg)
# ---------------------------------------------------------------------------

class Verifier:
    """Renders sampled frames with the CPU oracle and compares them with the
    GPU's outputs of the same frames."""

    def __init__(self, wl, want_kp: bool):
        from constructionsceneposeestimation_amd.packing import pack_scene
        from oracle.oracle import Oracle
        self.wl, self.want_kp = wl, want_kp
        self.o = Oracle(pack_scene(wl.scene), wl.width, wl.height)
        self.extra = any(k in wl.outputs for k in ("normals", "points"))

    def render(self, frames: List[int], threads: int):
        """(rgb, inst, depth[, normals, points]) of ``frames`` on ``threads``
        CPU threads: OpenMP over frames in the C oracle, or -- for frames of DR
        epochs (C4, per-frame light and textures) and the C5 outputs -- one
        oracle state per frame rendered on a thread pool."""
        wl, o = self.wl, self.o
        v, p = wl.frame_params(frames)
        if not wl.dr and not self.extra:
            models = np.stack([wl.epoch(f // 10).models.reshape(-1, 16) for f in frames])
            rgb, inst, depth = o.render_many(v, p, threads=threads, outputs=True, models=models)
            return v, p, {"rgb": rgb, "instance": inst, "depth": depth}
        jobs = []
        for k, f in enumerate(frames):
            st = wl.epoch(f // 10)
            dr = st.dr
            jobs.append((o.frame_state(st.models.reshape(-1, 16), dr.light if dr is not None else None,
                                       dr.textures if dr is not None else None), v[k], p[k]))
        outs = {}
        for r in o.render_parallel(jobs, threads, extra=self.extra):
            for key, a in r.items():
                if key != "inst_stats":
                    outs.setdefault(key, []).append(a)
        return v, p, {k: np.stack(a) for k, a in outs.items()}

    def compare(self, frames: List[int], v, p, ref: Dict[str, np.ndarray], gpu: Dict[str, np.ndarray]) -> List[str]:
        bad = []
        for k, f in enumerate(frames):
            for key, g in gpu.items():
                if key.startswith("keypoints") or key not in ref:
                    continue
                a, b = g[k], ref[key][k]
                if a.dtype.kind == "f":
                    a, b = a.view(np.uint32 if a.itemsize == 4 else np.uint16), b.view(np.uint32 if b.itemsize == 4 else np.uint16)
                if not np.array_equal(a, b):
                    bad.append(f"frame {f}: {key} ({int((a != b).sum())} values differ)")
            if self.want_kp:
                uv, vis = self.o.keypoints(v[k], p[k], self.wl.epoch(f // 10).keypoints, ref["depth"][k])
                if not np.array_equal(gpu["keypoints_uv"][k].view(np.uint32), uv.view(np.uint32)):
                    bad.append(f"frame {f}: keypoint uv")
                if not np.array_equal(gpu["keypoints_vis"][k], vis):
                    bad.append(f"frame {f}: keypoint visibility")
        return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=DEFAULT_STEPS)
    ap.add_argument("--warmup", type=int, default=DEFAULT_WARMUP)
    ap.add_argument("--frames-per-step", type=int, default=0,
                    help=f"frames per step = per launch chain (0: {DEFAULT_FRAMES_PER_STEP}, or "
                         f"{LARGE_FRAMES_PER_STEP} above 1920x1080)")
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--frames-per-launch", type=int, default=0, help="frames per kernel chain (0 = library default)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--contexts", type=int, default=1,
                    help="renderer contexts per GPU, each with its own stream, work buffers and output buffers; "
                         "steps alternate between them so one step's short kernels overlap the other's k_raster")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the legs that take runs of their own: the oracle check "
                         "of the timed outputs with the CPU baseline, the label-statistics batches and the "
                         "host-delivery batches (--verify-frames, --stats-steps and --pcie-steps size them)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's outputs to DIR/<name>.npy (keypoints whole, per-pixel "
                         "outputs at a fixed seeded sample of pixels; float32 / float64, at most 64 MB)")
    ap.add_argument("--verify-frames", type=int, default=32,
                    help="with --full: frames of the last timed step re-rendered by the oracle and compared (rank 0 "
                         "at N=1: also the all-cores CPU baseline sample); 0 skips the check and the CPU baseline")
    ap.add_argument("--verify-frames-multi", type=int, default=4, help="frames each rank checks when N > 1")
    ap.add_argument("--cpu-single-frames", type=int, default=3, help="frames of the single-thread CPU baseline run")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the all-cores CPU run (0 = all available)")
    ap.add_argument("--pcie-steps", type=int, default=3, help="with --full: batches timed with host outputs (0 = skip)")
    ap.add_argument("--stats-steps", type=int, default=5,
                    help="with --full: batches timed with label statistics (0 = skip)")
    ap.add_argument("--prep-workers", type=int, default=-1,
                    help="processes that compute the schedule's epochs and cameras before the GPU is touched "
                         "(-1: this rank's share of the CPUs for schedules of 512 epochs or more, else none)")
    ap.add_argument("--size-work", type=int, default=1,
                    help="1: size the work buffers by a sizing pass over the schedule (csg_size_work); "
                         "0: the library's full-scene caps")
    ap.add_argument("--work-margin", type=float, default=0.25, help="cap = largest measured count x (1 + margin)")
    ap.add_argument("--profile-json", default=os.path.join(ROOT, "profiles", "pmc_traffic.json"))
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # a plain `python bench.py --gpus N`: start the N ranks here, before
        # torch is imported (nothing in this process touches the GPU) -- unless
        # a profiler's preloaded library already initialised the GPU in this
        # process: children started from it would inherit that state and the
        # preload
        why = profiler_preload(os.environ)
        if why:
            log(f"bench: --gpus {args.gpus} under a profiler ({why}): this process has already initialised the "
                "GPU, so it cannot start its ranks; profile one rank per command, or put torchrun in front")
            sys.exit(2)
        sys.exit(launch_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"note: WORLD_SIZE={world} but --gpus={args.gpus}; using WORLD_SIZE")

    # ---- schedule for every step: its epochs and cameras are numpy work of
    # ~2 ms per epoch, computed in worker processes that start here, before
    # this process imports torch or touches the GPU, and collected below
    from constructionsceneposeestimation_amd.workload import WORKLOADS, Workload
    t0 = time.time()
    K, W = args.steps, args.warmup
    wl = Workload(args.workload, seed=args.seed)
    H, Wd = wl.height, wl.width
    F = args.frames_per_step or default_frames_per_step(Wd, H)
    fids = rank_frames(rank, world, W + K, F)
    epochs = sorted({f // 10 for f in fids})
    if len(epochs) > MAX_SETS:
        raise SystemExit(f"bench: {len(epochs)} randomisation epochs on rank {rank}, the library holds {MAX_SETS} "
                         "transform sets: fewer --steps or --frames-per-step")
    n_prep = prep_worker_count(args.prep_workers, len(epochs), world, os.environ)
    prep = SchedulePrep(wl, args.workload, args.seed, fids, n_prep)

    import torch
    import torch.distributed as dist
    if world > 1:
        # Gloo's C++ side prints its connection report ("[Gloo] Rank r is connected
        # to ...") on stdout while the mesh forms; stdout carries only the JSON line,
        # so the descriptor points at stderr until the first barrier has completed
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("gloo", init_method="env://")
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)

    from constructionsceneposeestimation_amd.renderer import FRAME_DTYPE, Renderer, make_frames

    # one rank per GPU (the driver's 8-GPU node: local = device); on a box with
    # fewer GPUs than ranks (a rehearsal) ranks share devices round-robin
    ndev = torch.cuda.device_count()
    local = local % ndev if ndev else local
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    device_info = {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "device": local,
                   "device_count": ndev, "pci": device_pci(local)}
    outs = set(WORKLOADS[args.workload]["outputs"])   # C5 adds depth, normals and world points
    want_kp = "keypoints" in outs

    # ---- the schedule, uploaded before timing -------------------------------
    set_of = {e: i for i, e in enumerate(epochs)}
    NC = max(1, args.contexts)
    ctxs = [Renderer(wl.scene, Wd, H, max_frames=F, device=local, frames_per_launch=args.frames_per_launch)
            for _ in range(NC)]
    r = ctxs[0]
    views, projs, uploaded = [], [], set()
    for states, v, p in prep.chunks():
        views.append(v)
        projs.append(p)
        for e, st in states.items():
            if e in uploaded:
                continue
            uploaded.add(e)
            for c in ctxs:
                c.set_instance_transforms(set_of[e], st.models)
                if want_kp:
                    c.set_keypoints(set_of[e], st.keypoints)
                if st.dr is not None:                      # C4: per-epoch lighting and texture DR
                    c.set_dr_light(set_of[e], st.dr.light)
                    c.set_dr_textures(set_of[e], st.dr.textures)
    views, projs = np.concatenate(views), np.concatenate(projs)
    t_sched = time.time() - t0
    frames = make_frames(views, projs, [set_of[f // 10] for f in fids], fids)
    frames_dev = torch.from_numpy(frames.view(np.uint8).copy()).to(dev)
    fsz = FRAME_DTYPE.itemsize
    Kp = r.n_kp
    # Work buffers sized by a sizing pass over this rank's whole schedule (setup
    # and binning kernels only, outside the timed region): each frame record
    # gets its measured record / bin-entry counts x 1.25 as hints, and the
    # record and bin pools hold the heaviest run of F consecutive frames, so no
    # step can overflow (the counts are a pure function of the frame); without
    # it the library sizes every frame for every scene triangle (~100 GB at C3 x
    # 960 frames)
    winfo = None
    t1 = time.time()
    if args.size_work:
        for c in ctxs:
            winfo = c.size_work(frames_dev.data_ptr(), len(fids), on_device=True, margin=args.work_margin)
    else:
        winfo = r.work_info()
    t_size = time.time() - t1

    def out_set():
        d = {"rgb": torch.empty((F, H, Wd, 3), dtype=torch.uint8, device=dev),
             "instance": torch.empty((F, H, Wd), dtype=torch.int32, device=dev)}
        if "depth" in outs:
            d["depth"] = torch.empty((F, H, Wd), dtype=torch.float32, device=dev)
        if "normals" in outs:
            d["normals"] = torch.empty((F, H, Wd, 3), dtype=torch.float16, device=dev)
        if "points" in outs:
            d["points"] = torch.empty((F, H, Wd, 3), dtype=torch.float32, device=dev)
        if want_kp:
            d["keypoints_uv"] = torch.empty((F, Kp, 2), dtype=torch.float32, device=dev)
            d["keypoints_vis"] = torch.empty((F, Kp), dtype=torch.int32, device=dev)
        return d
    # one output set per context: consecutive steps on different contexts run
    # concurrently, so they must not share output buffers
    out_sets = [out_set() for _ in range(NC)]
    dev_out = out_sets[0]
    rgb, inst = dev_out["rgb"], dev_out["instance"]
    extras = [{k: d[k].data_ptr() for k in ("depth", "normals", "points", "keypoints_uv", "keypoints_vis") if k in d}
              for d in out_sets]
    for x in extras:
        for a, b in (("keypoints_uv", "kp_uv"), ("keypoints_vis", "kp_vis")):
            if a in x:
                x[b] = x.pop(a)
    extra = extras[0]
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(NC - 1)]
    stream = streams[0].cuda_stream
    log(f"[rank {rank}] setup {time.time() - t0:.1f}s (schedule {t_sched:.1f}s with {n_prep} workers, sizing pass "
        f"{t_size:.1f}s): {len(fids)} frames, {len(epochs)} epochs, "
        f"{wl.scene.n_tris_per_frame} tris/frame, K={Kp} keypoints")

    def step(s, **kw):
        base = frames_dev.data_ptr() + s * F * fsz
        r.render_into(base, F, True, rgb.data_ptr(), inst.data_ptr(), stream=stream, **extra, **kw)

    def timed_step(s):
        # step s runs on context s % NC, into that context's outputs, on its stream
        c = s % NC
        base = frames_dev.data_ptr() + s * F * fsz
        o = out_sets[c]
        ctxs[c].render_into(base, F, True, o["rgb"].data_ptr(), o["instance"].data_ptr(),
                            stream=streams[c].cuda_stream, **extras[c])

    for s in range(W):
        timed_step(s)
    torch.cuda.synchronize(dev)
    for c in ctxs:
        c.synchronize()       # raises on any warm-up overflow (sticky flag), then clears it
        c.timing_reset()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t_start = time.perf_counter()
    for s in range(W, W + K):
        timed_step(s)
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t_start
    if world > 1:
        dist.barrier()
    # The overflow flag is sticky across the asynchronous batches: this raises
    # (and no line is printed) if any timed batch truncated records or bins.
    tms, bsts = [], []
    for c in ctxs:
        c.synchronize()
        tms.append(c.timing_read())
        bsts.append(c.batch_stats())
    tm = {k: sum(t[k] for t in tms) for k in tms[0]}
    bst = {k: sum(b[k] for b in bsts) for k in bsts[0]}
    elapsed_max = max_over_ranks(elapsed, world)
    dev_out = out_sets[(W + K - 1) % NC]        # the context that rendered the last timed step

    # ---- the last timed step's outputs, copied before anything reuses them --
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, dev_out)
        log(f"[rank {rank}] wrote the last timed step's outputs to {args.dump_outputs}: {dumped}")
    nver = args.verify_frames if world == 1 else min(args.verify_frames, args.verify_frames_multi)
    vidx = verify_sample_indices(F, nver if args.full else 0)
    last = fids[(W + K - 1) * F:(W + K) * F]
    sample_frames = [last[k] for k in vidx]
    gpu_sample = {}
    if vidx:
        ix = torch.tensor(vidx, device=dev)
        gpu_sample = {k: t.index_select(0, ix).cpu().numpy() for k, t in dev_out.items()}

    # ---- roofline (HIP events on the launch stream) --------------------------
    npx = H * Wd
    px_bytes = 3 + 4 + (4 if "depth" in dev_out else 0) + (6 if "normals" in dev_out else 0) + \
        (12 if "points" in dev_out else 0)             # RGB8 + int32 instance (+ C5's f32 depth, f16x3, f32x3)
    b_out = npx * px_bytes
    b_tex = int(wl.scene.texture_bytes())
    b_geom = int(wl.scene.authored_bytes())
    launches = max(tm["batches"], 1)                   # k_raster launches (one per launch chain)
    frames_per_launch = tm["frames"] / launches
    value = aggregate_value(K, F, world, elapsed_max)
    traffic = None
    valu = None
    work = None
    if os.path.exists(args.profile_json):
        try:
            pj = json.load(open(args.profile_json))
            if (pj.get("workload") == args.workload and pj.get("frames_per_launch") == frames_per_launch
                    and pj.get("B_frame") == b_geom + b_tex + b_out):
                traffic = {k: v for k, v in pj.get("bytes_per_launch", {}).items()}
                work = pj.get("k_raster_work_per_frame")
                if pj.get("k_raster_valu_pipe_occupancy") is not None:
                    valu = {"pipe_occupancy": round(pj["k_raster_valu_pipe_occupancy"], 3),
                            "pipe_occupancy_ceiling": pj.get("valu_pipe_ceiling"),
                            "wave_cycles": pj.get("k_raster_wave_cycles"),
                            "lane_util": round(pj.get("k_raster_valu_lane_util") or 0.0, 3),
                            "note": "calibrated on gfx950 (tools/calib_valu.hip, profiles/r06/calib): VALU pipe "
                                    "occupancy = SQ_INSTS_VALU x 2 cycles / (1,024 SIMDs x cycles) against the "
                                    "ceiling 8 waves per SIMD of independent FMAs reach; k_raster's limiter is "
                                    "latency: the share of its wave-cycles parked on s_waitcnt / s_barrier "
                                    "(SQ_WAIT_ANY), profiles/pmc_traffic.json"}
        except Exception:
            traffic = valu = work = None
    rf = roofline(b_geom, b_tex, b_out, frames_per_launch, tm["ms_raster"] / launches, tm["ms_setup"] / launches,
                  bst["records"] / max(bst["frames"], 1), value / world, traffic)
    rf["valu"] = valu
    if NC > 1:
        # steps on different contexts run at the same time, so each stream's
        # event interval includes time spent sharing the GPU with the other
        # context: no per-kernel time (the frame-level figure stands)
        rf["kernels"] = []
        rf["avg_launch_ms"] = None
        rf["kernels_note"] = (f"{NC} contexts overlap on the GPU: per-kernel HIP-event times are not kernel times; "
                              "time kernels with --contexts 1")
    # work rates (a tris/s and fragments/s figure beside the bytes)
    fps_gpu = value / world
    rates = {"tris_per_s": round(fps_gpu * wl.scene.n_tris_per_frame),
             "raster_records_per_s": round(fps_gpu * bst["records"] / max(bst["frames"], 1)),
             "bin_entries_per_s": round(fps_gpu * bst["bin_entries"] / max(bst["frames"], 1)),
             "per": "GPU"}
    if work is not None:
        rates["fragments_per_s"] = round(fps_gpu * work["fragments"])
        rates["fragments_note"] = work.get("source")
    rf["rates"] = rates
    if traffic is not None:
        rf["traffic_note"] = ("HBM bytes per launch from rocprofv3 PMC: FETCH_SIZE x 2 (gfx950 counts half of a "
                              "128-B read request, MI355X_MICROARCH.md §HBM) + WRITE_SIZE, KB = 1024 B")

    # ---- verification + CPU baseline (oracle) --------------------------------
    cpu = None
    bad: List[str] = []
    if vidx:
        ver = Verifier(wl, want_kp)
        if rank == 0 and world == 1:
            # the box's CPU share (OMP_NUM_THREADS is set to it there), else every CPU of this process
            thr = args.cpu_threads or int(os.environ.get("OMP_NUM_THREADS") or 0) or available_cpus()
            res = {}

            def run_all():
                res["out"] = ver.render(sample_frames, thr)
            t_all = median_time(run_all, runs=5, warmup=1, what=f"{thr} threads")
            n1 = max(1, min(args.cpu_single_frames, len(sample_frames)))
            t_one = median_time(lambda: ver.render(sample_frames[:n1], 1), runs=5, warmup=1, what="1 thread")
            v_, p_, ref = res["out"]
            bad = ver.compare(sample_frames, v_, p_, ref, gpu_sample)
            how = ("OpenMP over frames" if not (wl.dr or ver.extra) else
                   "a thread pool of per-frame oracle states (DR light/textures or C5 outputs)")
            cpu = {"value": round(len(sample_frames) / t_all, 3), "unit": "frames/s", "cores": thr, "kind": "port",
                   "single_thread": round(n1 / t_one, 3),
                   "share": (f"{thr} of the {available_cpus()} CPUs this process may use: the GPU box's CPU share "
                             f"(OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS')})"
                             if os.environ.get("OMP_NUM_THREADS") and not args.cpu_threads else
                             f"{thr} of the {available_cpus()} CPUs this process may use"),
                   "sample": f"{len(sample_frames)} frames of the last timed step of the {args.workload} schedule "
                             f"(seed {args.seed}) at {Wd}x{H} on {thr} threads ({how}); the first {n1} of them "
                             f"also single-threaded; oracle/csg_oracle.c, median of 5 after 1 warm-up, wall clock, "
                             f"no file I/O",
                   "method": "median of 5 after 1 warm-up", "nproc": os.cpu_count(), "available_cpus": available_cpus(),
                   "cpu_model": cpu_model()}
        else:
            v_, p_, ref = ver.render(sample_frames, 2)
            bad = ver.compare(sample_frames, v_, p_, ref, gpu_sample)
    n_checked, n_bad = sum_over_ranks([len(sample_frames), len(bad)], world)
    stage_ms = {k: round(tm[k] / K, 4) for k in ("ms_setup", "ms_bin", "ms_raster", "ms_keypoints")}
    per_rank = {"rank": rank, "elapsed_s": round(elapsed, 6), "frames_per_s": round(K * F / elapsed, 2),
                "stage_ms_per_step": stage_ms}
    shards = shard_report(timed_frames(fids, W, K, F), world, device_info, per_rank)
    if n_bad:
        for b in bad[:20]:
            log(f"[rank {rank}] VERIFY FAILED: {b}")
        log(f"[rank {rank}] {n_bad} mismatches between the timed GPU outputs and the oracle: no result")
        if world > 1:
            dist.destroy_process_group()
        sys.exit(3)

    # ---- with label statistics (rank 0, N=1 only; never `value`) -------------
    with_stats = None
    if args.full and rank == 0 and world == 1 and args.stats_steps > 0:
        try:
            st_buf = torch.empty((F, r.n_labels, 5), dtype=torch.int32, device=dev)
            step(0, stats=st_buf.data_ptr())
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for k in range(args.stats_steps):
                step(k % (W + K), stats=st_buf.data_ptr())
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t1
            r.synchronize()
            with_stats = {"value": round(args.stats_steps * F / dt, 2), "unit": "frames/s",
                          "note": f"the timed batches plus per-label pixel count and 2D box (inst_stats); "
                                  f"{args.stats_steps} batches of {F}"}
            # + occlusion coverage (k_raster<true>) and the JET depth image (GDP:1690-1709)
            cov_buf = torch.empty((F, r.n_labels), dtype=torch.int32, device=dev)
            dv_buf = torch.empty((F, H, Wd, 3), dtype=torch.uint8, device=dev)
            kw = dict(stats=st_buf.data_ptr(), covered=cov_buf.data_ptr(), depth_vis=dv_buf.data_ptr())
            step(0, **kw)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for k in range(args.stats_steps):
                step(k % (W + K), **kw)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t1
            r.synchronize()
            with_stats["with_occlusion_and_depth_png"] = {
                "value": round(args.stats_steps * F / dt, 2), "unit": "frames/s",
                "note": "plus per-label unoccluded coverage (occlusionRatio) and the JET depth visualisation "
                        "(depth written to scratch, per-frame min/max, colour map)"}
        except Exception as e:  # the extra figure must never break the bench line
            log(f"with-stats measurement failed: {e}")

    # ---- host delivery, PCIe included (never `value`) --------------------------
    # The reference's boundary hands its caller host arrays (get_rgba,
    # generate_construction_data.py:1669; the int32 mask :1909-1910).  At N = 1
    # rank 0 times its batches of F frames with host outputs; at N > 1 every rank
    # does so at once (batches of at most PCIE_FRAMES_MULTI frames, started at one
    # barrier), since what 8 GPUs deliver into one host's memory is the figure a
    # user of the node gets.  Instance ids cross PCIe narrowed (csg_host_id_bytes)
    # and are widened to int32 on host threads inside the timed region.
    pcie = None
    if args.full and args.pcie_steps > 0:
        import ctypes as C
        from constructionsceneposeestimation_amd import _lib
        Fp = F if world == 1 else min(F, PCIE_FRAMES_MULTI)
        leg, idb = None, 4
        kpb = Kp * 12 if want_kp else 0
        try:
            h_rgb = torch.empty((Fp, H, Wd, 3), dtype=torch.uint8, pin_memory=True)
            h_inst = torch.empty((Fp, H, Wd), dtype=torch.int32, pin_memory=True)
            h_uv = torch.empty((Fp, max(Kp, 1), 2), dtype=torch.float32, pin_memory=True)
            h_vis = torch.empty((Fp, max(Kp, 1)), dtype=torch.int32, pin_memory=True)
            o = _lib.Outputs(h_rgb.data_ptr(), h_inst.data_ptr(), None, h_uv.data_ptr() if want_kp else None,
                             h_vis.data_ptr() if want_kp else None, None, r.n_labels, 0, None, None)
            # the first step's records as the device holds them: with their work
            # hints (csg_size_work wrote those into frames_dev, not `frames`)
            hframes = frames_dev[:Fp * fsz].cpu().numpy().view(FRAME_DTYPE)

            def leg():
                r._check(r.lib.csg_render_batch_async(r.ctx, hframes.ctypes.data, Fp, 0, C.byref(o), None), "pcie")
            leg()
            r.synchronize()
            idb = r.host_id_bytes()
        except Exception as e:  # the extra figure must never break the bench line
            leg = None
            log(f"[rank {rank}] host-delivery leg setup failed: {e}")
        if world > 1:
            dist.barrier()   # every rank starts its leg together (a failed setup still joins)
        mine = None
        if leg is not None:
            try:
                t1 = time.perf_counter()
                for _ in range(args.pcie_steps):
                    leg()
                r.synchronize()
                dt = time.perf_counter() - t1
                nf = args.pcie_steps * Fp
                mine = {"frames": nf, "seconds": dt, "wire_bytes": nf * (npx * (3 + idb) + kpb),
                        "delivered_bytes": nf * (npx * 7 + kpb)}
            except Exception as e:
                log(f"[rank {rank}] host-delivery measurement failed: {e}")
        if world > 1:
            pcie = gather_delivery(mine, world)
        elif mine is not None:
            pcie = {"value": round(mine["frames"] / mine["seconds"], 2), "unit": "frames/s",
                    "wire_gbs": round(mine["wire_bytes"] / mine["seconds"] / 1e9, 2),
                    "delivered_gbs": round(mine["delivered_bytes"] / mine["seconds"] / 1e9, 2)}
        if pcie is not None:
            pcie["gbs"] = pcie["wire_gbs"]
            pcie["ids_wire_bytes"] = idb
            pcie["note"] = (f"RGB8 + int32 instance ids + keypoints delivered into pinned host memory inside the timed "
                            f"region, {args.pcie_steps} batches of {Fp} frames per rank"
                            + (f", all {world} ranks at once" if world > 1 else "")
                            + f"; the ids cross PCIe as {idb}-byte values (id + 1) and host threads widen them to "
                              f"int32 ({npx * (3 + idb) / 1e6:.1f} MB/frame on the wire, "
                              f"{npx * 7 / 1e6:.1f} MB/frame delivered); each launch chain's slice is copied while "
                              f"the next chains render")

    if rank == 0:
        line = {
            "metric": METRIC, "value": round(value, 2), "unit": "frames/s", "n_gpus": world, "steps": K,
            "warmup": W, "ms_per_step": round(elapsed_max / K * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "full": bool(args.full),
            "config": {"workload": f"{args.workload}: " + WORKLOADS[args.workload]["title"]
                                   + f", {Wd}x{H}, RGB8 + int32 instance mask"
                                   + (f" + {Kp} 2D keypoints/frame" if want_kp else "")
                                   + "".join(f" + {o}" for o in ("depth", "normals", "points") if o in outs),
                       "frames_per_step": F, "frames_per_launch": frames_per_launch, "seed": args.seed,
                       "contexts": NC,
                       "width": Wd, "height": H, "tris_per_frame": wl.scene.n_tris_per_frame,
                       "parallelism": f"seed-sharded epochs x{world}, no collectives"},
            "roofline": rf,
            "cpu_baseline": cpu,
            "verified": {"frames": n_checked, "bit_exact": n_checked > 0,
                         "outputs": sorted(gpu_sample) if gpu_sample else [],
                         "against": "oracle/csg_oracle.c on frames of the last timed step",
                         "overflow": "none: sticky flag checked after the warm-up and after the timed steps"},
            "shards": shards,
            "pcie_inclusive": pcie,
            "with_label_stats": with_stats,
            "stage_ms_per_step": stage_ms,
            "work": {"bytes": int(winfo["work_bytes"]), "contexts": NC,
                     "pool_records": int(winfo["pool_records"]), "pool_bins": int(winfo["pool_bins"]),
                     "hinted": bool(winfo["hinted"]), "hint_retries": int(r.work_info()["hint_retries"]),
                     "records_per_frame_cap": int(winfo["records_per_frame"]),
                     "bins_per_frame_cap": int(winfo["bins_per_frame"]),
                     "frames_per_launch": int(winfo["frames_per_launch"]),
                     "sized_frames": int(winfo["sized_frames"]), "max_records": int(winfo["max_records"]),
                     "max_bins": int(winfo["max_bins"]), "mean_records": round(winfo["mean_records"], 1),
                     "mean_bins": round(winfo["mean_bins"], 1),
                     "how": (f"csg_size_work over the rank's {len(fids)} scheduled frames, margin {args.work_margin}: "
                             "per-frame hints, pools for the heaviest run of frames_per_launch frames"
                             if args.size_work else "full-scene caps (1.125 x triangles per frame)")},
            "records_per_frame": round(bst["records"] / max(bst["frames"], 1), 1),
            "bin_entries_per_frame": round(bst["bin_entries"] / max(bst["frames"], 1), 1),
        }
        print(json.dumps(line), flush=True)
    r.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
