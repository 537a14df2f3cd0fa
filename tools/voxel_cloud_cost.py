"""Cost of the voxel-downsampled point clouds (csg_voxel_cloud: k_vx_init +
k_vx_insert + k_vx_mark + k_vx_scan + k_vx_emit) behind a render.

C3 at 1080p, device-resident batches of F frames (device frame records, device
outputs, Renderer.render_into on the caller's stream), timed with HIP events
around the enqueue, variants alternated, median of --reps after one warm-up of
each (the method of tools/object_points_cost.py), per voxel size:

  render            rgb + instance + points
  render_voxels     ... + csg_voxel_cloud on them, all six outputs
  voxels_only       csg_voxel_cloud alone on what the last render left
  voxels_only_plain the same with CSG_VOXEL_COMBINE=0: an atomic per point instead
                    of one per run of equal keys inside a wave

`render_voxels - render` is the pass behind the render, `voxels_only` the same
kernels timed directly.  Also recorded: the distribution of the voxel count V
per frame, the capacity the retries settle on from the default, the dropped
points, the bytes a frame's records take against the dense PLY's 15 B per
pixel, and the time the NumPy restatement (tests/test_voxel_cloud.py) takes
on --host-frames delivered dense frames.  Writes one JSON file.

    python tools/voxel_cloud_cost.py --frames 480 --out profiles/voxel_cloud/cost.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=8)
    ap.add_argument("--voxel-sizes", default="0.05,0.10")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--out", default=os.path.join("profiles", "voxel_cloud", "cost.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from constructionsceneposeestimation_amd.voxel_cloud import DEFAULT_VOXEL_CAPACITY, OVERFLOW, RECORD_DTYPE
    from constructionsceneposeestimation_amd.workload import Workload
    from tests.test_voxel_cloud import restate_frame
    if not torch.cuda.is_available():
        raise SystemExit("voxel_cloud_cost: needs the GPU (no CPU timing stands in for it)")
    wl = Workload("C3", seed=0, width=a.width, height=a.height)
    n, H, W = a.frames, wl.height, wl.width
    fids = list(range(n))
    epochs = sorted({f // 10 for f in fids})
    dev = torch.device("cuda", 0)
    res = {"workload": "C3", "width": W, "height": H, "frames": n,
           "method": f"HIP events around the enqueue on the caller's stream, device frame records and outputs, "
                     f"variants alternated, median of {a.reps} after one warm-up each",
           "dense_ply_bytes_per_frame": 15 * H * W, "record_bytes": RECORD_DTYPE.itemsize, "voxel_sizes": {}}
    with Renderer(wl.scene, W, H, max_frames=n) as r:
        L = r.n_labels
        res["n_labels"] = L
        for k, e in enumerate(epochs):
            r.set_instance_transforms(k, wl.epoch(e).models)
        V, P = wl.frame_params(fids)
        fr = make_frames(V, P, [epochs.index(f // 10) for f in fids], fids)
        frames_dev = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
        r.size_work(frames_dev.data_ptr(), n, on_device=True)   # work buffers sized for these frames, as bench.py

        def buf(shape, dt):
            return torch.empty(shape, dtype=dt, device=dev)

        rgb, inst, pts = buf((n, H, W, 3), torch.uint8), buf((n, H, W), torch.int32), buf((n, H, W, 3), torch.float32)
        tot = buf((2, n), torch.int32)
        stream = torch.cuda.Stream(dev)   # (the null stream's handle 0 would mean "the context's own stream")

        def render():
            r.render_into(frames_dev.data_ptr(), n, True, rgb.data_ptr(), inst.data_ptr(), points=pts.data_ptr(),
                          stream=stream.cuda_stream)

        def once(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for s in steps:
                s()
            e1.record(stream)
            e1.synchronize()
            r.synchronize()
            return e0.elapsed_time(e1) / 1e3

        once((render,))
        host = {k: t[:a.host_frames].cpu().numpy() for k, t in (("points", pts), ("rgb", rgb), ("instance", inst))}
        for size in [float(x) for x in a.voxel_sizes.split(",") if x.strip()]:
            cap, tries = min(DEFAULT_VOXEL_CAPACITY, H * W), 0
            while True:   # the capacity the retries settle on, from the default
                out = {"vx_xyz": buf((n, cap, 3), torch.float32), "vx_rgb": buf((n, cap, 3), torch.uint8),
                       "vx_label": buf((n, cap), torch.int32), "vx_count": buf((n, cap), torch.int32)}

                def voxels(combine="1", cap=cap, out=out, size=size):
                    os.environ["CSG_VOXEL_COMBINE"] = combine   # read by the call
                    r.voxel_cloud(n, voxel_size=size, capacity=cap, points=pts.data_ptr(), rgb=rgb.data_ptr(),
                                  instance=inst.data_ptr(), vx_total=tot[0].data_ptr(), vx_dropped=tot[1].data_ptr(),
                                  stream=stream.cuda_stream, **{k: t.data_ptr() for k, t in out.items()})

                once((voxels,))
                totals = tot.cpu().numpy().view(np.uint32)
                if not (totals[0] == OVERFLOW).any() or cap >= H * W:
                    break
                del out
                cap, tries = min(2 * cap, H * W), tries + 1
            variants = {"render": (render,), "render_voxels": (render, voxels), "voxels_only": (voxels,),
                        "voxels_only_plain": (lambda: voxels("0"),)}
            for steps in variants.values():   # warm-up of every variant
                once(steps)
            times = {k: [] for k in variants}
            for _ in range(a.reps):           # alternating
                for k, steps in variants.items():
                    times[k].append(once(steps))
            os.environ.pop("CSG_VOXEL_COMBINE", None)
            plain = {k: t.clone() for k, t in out.items()}             # the last run was the plain form
            once((voxels,))
            same = all(torch.equal(plain[k].view(torch.uint8), out[k].view(torch.uint8)) for k in out)   # bytes: NaN fill
            vcount = totals[0].astype(np.int64)
            # the host's way: the same voxelisation in NumPy on delivered dense arrays
            t0 = time.perf_counter()
            ref = [restate_frame(host["points"][f], host["rgb"][f], host["instance"][f], L, size, cap)
                   for f in range(a.host_frames)]
            host_s = time.perf_counter() - t0
            agree = all(int(ref[f]["total"]) == int(vcount[f]) and
                        np.array_equal(ref[f]["vx_xyz"][:vcount[f]].view(np.uint32),
                                       out["vx_xyz"][f, :int(vcount[f])].cpu().numpy().view(np.uint32))
                        for f in range(a.host_frames))
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            print(f"voxel size {size:g}: {med}", file=sys.stderr, flush=True)
            behind = med["render_voxels"] - med["render"]
            res["voxel_sizes"][f"{size:g}"] = {
                **{f"{k}_s": round(v, 6) for k, v in med.items()},
                "runs_s": {k: [round(t, 6) for t in v] for k, v in times.items()},
                "voxels_behind_render_us_per_frame": round(behind / n * 1e6, 2),
                "voxels_only_us_per_frame": round(med["voxels_only"] / n * 1e6, 2),
                "voxels_only_plain_us_per_frame": round(med["voxels_only_plain"] / n * 1e6, 2),
                "plain_over_combined": round(med["voxels_only_plain"] / med["voxels_only"], 3),
                "extra_fraction_of_render": round(behind / med["render"], 4),
                "source_bytes_read_per_frame": H * W * 19,
                "read_tb_per_s_voxels_only": round(n * H * W * 19 / med["voxels_only"] / 1e12, 3),
                "voxels_per_frame": {"mean": round(float(vcount.mean()), 1), "max": int(vcount.max()),
                                     "min": int(vcount.min()), "p99": int(np.percentile(vcount, 99))},
                "capacity_settled_on": cap, "capacity_retries": tries,
                "dropped_points": {"total": int(totals[1].sum()), "max_per_frame": int(totals[1].max())},
                "record_bytes_per_frame": {"mean": round(float(vcount.mean()) * RECORD_DTYPE.itemsize),
                                           "max": int(vcount.max()) * RECORD_DTYPE.itemsize},
                "fraction_of_dense_ply": round(float(vcount.mean()) * RECORD_DTYPE.itemsize / (15 * H * W), 5),
                "both_forms_give_equal_bytes": bool(same),
                "numpy_restatement": {"frames": a.host_frames, "s_per_frame": round(host_s / max(a.host_frames, 1), 4),
                                      "agrees_with_the_gpu": bool(agree)}}
            del out, plain
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
