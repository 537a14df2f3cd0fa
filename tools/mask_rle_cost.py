"""Cost of the mask spans (csg_mask_spans: k_span_count + k_span_scan +
k_span_emit) and the span counts of C3 frames.

C3 at 1080p, device-resident batches of F frames (device frame records, device
outputs, Renderer.render_into on the caller's stream), timed with HIP events
around the enqueue, variants alternated, median of --reps after one warm-up of
each (the method of tools/crop_cost.py):

  render       rgb + instance + depth + stats
  with_spans   ... + csg_mask_spans on the same stream
  spans_only   csg_mask_spans alone on the ids the last render left

`with_spans - render` is the pass behind a render, `spans_only` the same kernels
timed directly.  The kernels read the id image three times (k_span_count once,
k_span_emit twice: 12 B per pixel) and write 8 B per span; the implied rate
stands next to the ~6.3 TB/s a copy kernel reaches in HBM.  The span totals of
the frames (mean, p99, max) are what the generator's capacity is set from.
Writes one JSON file.

    python tools/mask_rle_cost.py --frames 480 --out profiles/mask_rle/cost.json
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
    ap.add_argument("--capacity", type=int, default=0, help="span records per frame (0: the renderer's default)")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--out", default=os.path.join("profiles", "mask_rle", "cost.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from constructionsceneposeestimation_amd.renderer import DEFAULT_SPAN_CAPACITY, Renderer, make_frames
    from constructionsceneposeestimation_amd.workload import Workload
    if not torch.cuda.is_available():
        raise SystemExit("mask_rle_cost: needs the GPU (no CPU timing stands in for it)")
    wl = Workload("C3", seed=0, width=a.width, height=a.height)
    n, H, W = a.frames, wl.height, wl.width
    cap = a.capacity or DEFAULT_SPAN_CAPACITY
    fids = list(range(n))
    epochs = sorted({f // 10 for f in fids})
    dev = torch.device("cuda", 0)
    with Renderer(wl.scene, W, H, max_frames=n) as r:
        L = r.n_labels
        for k, e in enumerate(epochs):
            r.set_instance_transforms(k, wl.epoch(e).models)
        V, P = wl.frame_params(fids)
        fr = make_frames(V, P, [epochs.index(f // 10) for f in fids], fids)
        frames_dev = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
        r.size_work(frames_dev.data_ptr(), n, on_device=True)   # work buffers sized for these frames, as bench.py
        rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        inst = torch.empty((n, H, W), dtype=torch.int32, device=dev)
        depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        stats = torch.empty((n, L, 5), dtype=torch.int32, device=dev)
        spans = torch.empty((n, cap, 2), dtype=torch.int32, device=dev)
        offs = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(dev)   # (the null stream's handle 0 would mean "the context's own stream")

        def render():
            r.render_into(frames_dev.data_ptr(), n, True, rgb.data_ptr(), inst.data_ptr(), depth.data_ptr(),
                          stats=stats.data_ptr(), stream=stream.cuda_stream)

        def span_pass():
            r.mask_spans(n, instance=inst.data_ptr(), spans=spans.data_ptr(), span_offsets=offs.data_ptr(),
                         capacity=cap, stream=stream.cuda_stream)

        variants = {"render": (render,), "with_spans": (render, span_pass), "spans_only": (span_pass,)}

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
        off = offs.cpu().numpy().view(np.uint32)
        totals = off[:, L].astype(np.int64)
        px = stats.cpu().numpy().view(np.uint32)[:, :, 0].astype(np.int64)
        # the spans agree with the render's own label statistics (frames that fit)
        sp = spans.cpu().numpy().view(np.uint32)
        fits = totals <= cap
        agree = all(int(sp[f, :totals[f], 1].sum()) == int(px[f].sum()) for f in np.nonzero(fits)[0][:32])
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    behind, direct = med["with_spans"] - med["render"], med["spans_only"]
    read_bytes = 3 * n * H * W * 4
    own_bytes = read_bytes + int(np.minimum(totals, cap).sum()) * 8 + n * (L + 1) * 4
    res = {"workload": "C3", "width": W, "height": H, "frames": n, "n_labels": L, "capacity": cap,
           "method": f"HIP events around the enqueue on the caller's stream, device frame records and outputs, "
                     f"variants alternated, median of {a.reps} after one warm-up each",
           "render_s": round(med["render"], 6), "with_spans_s": round(med["with_spans"], 6),
           "spans_only_s": round(direct, 6), "runs_s": {k: [round(t, 6) for t in v] for k, v in times.items()},
           "spans_behind_render_us_per_frame": round(behind / n * 1e6, 2),
           "spans_only_us_per_frame": round(direct / n * 1e6, 2),
           "extra_fraction_of_render": round(behind / med["render"], 4),
           "id_bytes_read": read_bytes, "own_bytes": own_bytes,
           "read_tb_per_s_spans_only": round(read_bytes / direct / 1e12, 3) if direct > 0 else None,
           "read_tb_per_s_behind_render": round(read_bytes / behind / 1e12, 3) if behind > 0 else None,
           "hbm_copy_tb_per_s": HBM_COPY_TBS,
           "spans_per_frame": {"mean": round(float(totals.mean()), 1), "p50": int(np.percentile(totals, 50)),
                               "p99": int(np.percentile(totals, 99)), "max": int(totals.max()),
                               "min": int(totals.min())},
           "frames_over_capacity": int((~fits).sum()),
           "span_bytes_per_frame_mean": round(float(totals.mean()) * 8 + (L + 1) * 4, 1),
           "dense_id_bytes_per_frame": {"one_byte_wire": H * W, "int32_npy": H * W * 4},
           "span_lengths_sum_to_inst_stats_pixels": bool(agree)}
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
