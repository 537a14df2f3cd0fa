"""Cost of the per-object point samples (csg_sample_object_points: k_pts_count +
k_pts_scan + k_pts_emit) behind a render and the crops.

C3 at 1080p, device-resident batches of F frames (device frame records, device
outputs, Renderer.render_into on the caller's stream), timed with HIP events
around the enqueue, variants alternated, median of --reps after one warm-up of
each (the method of tools/crop_cost.py and tools/mask_rle_cost.py):

  render               rgb + instance + depth + stats + obj_coords
  render_crops         ... + csg_crop_objects (plan; crop_rgb, crop_mask, crop_coords)
  render_crops_points  ... + csg_sample_object_points on the planned slots, all five outputs
  points_only          csg_sample_object_points alone on what the last render and plan left
  spans_only           csg_mask_spans alone on the same ids: the pass of the same kind, same session

`render_crops_points - render_crops` is the pass behind the crops, `points_only`
the same kernels timed directly.  The kernels read the id image twice (8 B per
pixel) and gather some 25 B per sample.  Writes one JSON file.

    python tools/object_points_cost.py --frames 480 --out profiles/object_points/cost.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--per-frame", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--out", default=os.path.join("profiles", "object_points", "cost.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from constructionsceneposeestimation_amd.crops import CROP_INFO_DTYPE, eligible_labels
    from constructionsceneposeestimation_amd.object_points import intrinsics_rows
    from constructionsceneposeestimation_amd.renderer import DEFAULT_SPAN_CAPACITY, Renderer, make_frames
    from constructionsceneposeestimation_amd.workload import Workload
    if not torch.cuda.is_available():
        raise SystemExit("object_points_cost: needs the GPU (no CPU timing stands in for it)")
    wl = Workload("C3", seed=0, width=a.width, height=a.height)
    n, H, W, K, N, S = a.frames, wl.height, wl.width, a.per_frame, a.samples, a.size
    cap = DEFAULT_SPAN_CAPACITY
    fids = list(range(n))
    epochs = sorted({f // 10 for f in fids})
    dev = torch.device("cuda", 0)
    with Renderer(wl.scene, W, H, max_frames=n) as r:
        L = r.n_labels
        for k, e in enumerate(epochs):
            st = wl.epoch(e)
            r.set_instance_transforms(k, st.models)
            r.set_object_frames(k, st.object_frames)
        V, P = wl.frame_params(fids)
        fr = make_frames(V, P, [epochs.index(f // 10) for f in fids], fids)
        frames_dev = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
        r.size_work(frames_dev.data_ptr(), n, on_device=True)   # work buffers sized for these frames, as bench.py

        def buf(shape, dt):
            return torch.empty(shape, dtype=dt, device=dev)

        rgb, inst, depth = buf((n, H, W, 3), torch.uint8), buf((n, H, W), torch.int32), buf((n, H, W), torch.float32)
        coords, stats = buf((n, H, W, 3), torch.int16), buf((n, L, 5), torch.int32)
        crop_rgb, crop_mask = buf((n, K, S, S, 3), torch.uint8), buf((n, K, S, S), torch.uint8)
        crop_coords, info = buf((n, K, S, S, 3), torch.int16), buf((n, K, CROP_INFO_DTYPE.itemsize), torch.uint8)
        pt_count, pt_choose = buf((n, K), torch.int32), buf((n, K, N), torch.int32)
        pt_xyz, pt_rgb = buf((n, K, N, 3), torch.float32), buf((n, K, N, 3), torch.uint8)
        pt_coords = buf((n, K, N, 3), torch.int16)
        spans, offs = buf((n, cap, 2), torch.int32), buf((n, L + 1), torch.int32)
        elig = torch.from_numpy(eligible_labels(wl.scene)[:L].copy()).to(dev)
        intr = torch.from_numpy(intrinsics_rows(fr)).to(dev)
        keys = torch.from_numpy(np.ascontiguousarray(fr["frame_id"]).view(np.int32)).to(dev)
        stream = torch.cuda.Stream(dev)   # (the null stream's handle 0 would mean "the context's own stream")

        def render():
            r.render_into(frames_dev.data_ptr(), n, True, rgb.data_ptr(), inst.data_ptr(), depth.data_ptr(),
                          stats=stats.data_ptr(), obj_coords=coords.data_ptr(), stream=stream.cuda_stream)

        def crops():
            r.crop_objects(n, size=S, per_frame=K, instance=inst.data_ptr(), rgb=rgb.data_ptr(),
                           obj_coords=coords.data_ptr(), stats=stats.data_ptr(), eligible=elig.data_ptr(),
                           crop_rgb=crop_rgb.data_ptr(), crop_mask=crop_mask.data_ptr(),
                           crop_coords=crop_coords.data_ptr(), info=info.data_ptr(), stream=stream.cuda_stream)

        def points():
            r.sample_points(n, samples=N, per_frame=K, seed=0, instance=inst.data_ptr(), info=info.data_ptr(),
                            depth=depth.data_ptr(), intrinsics=intr.data_ptr(), rgb=rgb.data_ptr(),
                            obj_coords=coords.data_ptr(), frame_keys=keys.data_ptr(), pt_count=pt_count.data_ptr(),
                            pt_choose=pt_choose.data_ptr(), pt_xyz=pt_xyz.data_ptr(), pt_rgb=pt_rgb.data_ptr(),
                            pt_coords=pt_coords.data_ptr(), stream=stream.cuda_stream)

        def span_pass():
            r.mask_spans(n, instance=inst.data_ptr(), spans=spans.data_ptr(), span_offsets=offs.data_ptr(),
                         capacity=cap, stream=stream.cuda_stream)

        variants = {"render": (render,), "render_crops": (render, crops), "render_crops_points": (render, crops, points),
                    "points_only": (points,), "spans_only": (span_pass,)}

        def once(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for s in steps:
                s()
            e1.record(stream)
            e1.synchronize()
            r.synchronize()
            return e0.elapsed_time(e1) / 1e3

        for steps in variants.values():   # warm-up of every variant
            once(steps)
        times = {k: [] for k in variants}
        for _ in range(a.reps):           # alternating
            for k, steps in variants.items():
                times[k].append(once(steps))
        cnt = pt_count.cpu().numpy().view(np.uint32).astype(np.int64)
        slots = info.cpu().numpy().view(CROP_INFO_DTYPE).reshape(n, K)
        live = slots["label"] >= 0
        agree = bool(np.array_equal(cnt, np.where(live, slots["pixels"], 0)))   # M is the plan's own pixel count
        choose = pt_choose.cpu().numpy().view(np.uint32)
        ids = inst[:8].cpu().numpy().reshape(8, -1)
        on_label = all((ids[f][choose[f, k]] == slots["label"][f, k]).all()
                       for f in range(min(n, 8)) for k in range(K) if cnt[f, k])
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    behind, direct = med["render_crops_points"] - med["render_crops"], med["points_only"]
    read_bytes = 2 * n * H * W * 4
    res = {"workload": "C3", "width": W, "height": H, "frames": n, "n_labels": L, "per_frame": K, "samples": N,
           "crop_size": S,
           "method": f"HIP events around the enqueue on the caller's stream, device frame records and outputs, "
                     f"variants alternated, median of {a.reps} after one warm-up each",
           **{f"{k}_s": round(v, 6) for k, v in med.items()},
           "runs_s": {k: [round(t, 6) for t in v] for k, v in times.items()},
           "points_behind_crops_us_per_frame": round(behind / n * 1e6, 2),
           "points_only_us_per_frame": round(direct / n * 1e6, 2),
           "spans_only_us_per_frame": round(med["spans_only"] / n * 1e6, 2),
           "points_over_spans": round(direct / med["spans_only"], 3),
           "extra_fraction_of_render": round(behind / med["render"], 4),
           "id_bytes_read": read_bytes,
           "read_tb_per_s_points_only": round(read_bytes / direct / 1e12, 3) if direct > 0 else None,
           "hbm_copy_tb_per_s": HBM_COPY_TBS,
           "sample_bytes_per_frame": K * (4 + N * 25),
           "dense_bytes_per_frame": {"ids_and_depth": H * W * 8, "ids_depth_rgb_coords": H * W * 17},
           "slots": {"live": int(live.sum()), "of": int(live.size), "more_pixels_than_samples": int((cnt > N).sum()),
                     "pixels_mean": round(float(cnt[live].mean()), 1) if live.any() else 0.0,
                     "pixels_max": int(cnt.max())},
           "pt_count_equals_planned_pixels": agree, "chosen_pixels_carry_the_label": bool(on_label)}
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
