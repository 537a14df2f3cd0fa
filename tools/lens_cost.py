"""Cost of the lens-distortion pass (csg_lens_remap: k_ln_init + k_ln_remap) behind a render.

C3 at 1080p, device-resident batches of F frames (device frame records, device outputs,
Renderer.render_into on the caller's stream), timed with HIP events around the enqueue, variants
alternated, median of --reps after one warm-up of each (the method of tools/sensor_depth_cost.py).
The run's frames are the source camera; the output camera has the same size, the coefficients of
--preset and the widest view the source holds (lens.fit_output, or --focal to skip the search).

  render         rgb + instance + depth + obj_coords (the render code is the parent commit's, unchanged)
  render_lens    ... + csg_lens_remap with every output
  lens_only      csg_lens_remap alone on what the last render left, every output
  lens_rgb_ids   csg_lens_remap with lens_rgb, lens_instance and lens_stats only
  torch          a torch restatement on the device of --torch-frames frames: index gathers for ids, depth,
                 coordinates and validity, integer bilinear for the RGB (no statistics), checked against
                 the pass to the bit

`render_lens - render` is the pass behind the render, `lens_only` the same kernels timed directly.  The
bytes per output pixel are counted from the layouts: the map entry, one source element per nearest
output (the four RGB taps counted once: neighbours share them), and every output.  Writes one JSON file.

    python tools/lens_cost.py --frames 480 --out profiles/lens/cost.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES_IN = {"map": 8, "rgb": 3, "instance": 4, "depth": 4, "obj_coords": 6}
BYTES_OUT = {"lens_rgb": 3, "lens_instance": 4, "lens_depth": 4, "lens_coords": 6, "lens_valid": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-frames", type=int, default=16)
    ap.add_argument("--preset", default="wide")
    ap.add_argument("--focal", type=float, default=0.0, help="output focal length in pixels (0: lens.fit_output)")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--out", default=os.path.join("profiles", "lens", "cost.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from constructionsceneposeestimation_amd import lens
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from constructionsceneposeestimation_amd.workload import Workload
    if not torch.cuda.is_available():
        raise SystemExit("lens_cost: needs the GPU (no CPU timing stands in for it)")
    wl = Workload("C3", seed=0, width=a.width, height=a.height)
    n, H, W = a.frames, wl.height, wl.width
    source = (W, H, wl.intr.fx, wl.intr.fy, wl.intr.cx, wl.intr.cy)
    model = lens.output_camera(lens.PRESETS[a.preset], W, H, a.focal or 1.0).with_source(*source)
    if not a.focal:
        model = lens.fit_output(model)
    host_map, map_counts = lens.build_map(model)
    fids = list(range(n))
    epochs = sorted({f // 10 for f in fids})
    dev = torch.device("cuda", 0)
    bpp = sum(BYTES_IN.values()) + sum(BYTES_OUT.values())
    res = {"workload": "C3", "width": W, "height": H, "frames": n, "preset": a.preset, "model": model.as_dict(),
           "map_counts": dict(zip(lens.cause_names, (int(v) for v in map_counts))),
           "method": f"HIP events around the enqueue on the caller's stream, device frame records and outputs, "
                     f"variants alternated, median of {a.reps} after one warm-up each",
           "bytes_per_output_pixel": {"read": BYTES_IN, "written": BYTES_OUT, "total": bpp}}
    with Renderer(wl.scene, W, H, max_frames=n) as r:
        for k, e in enumerate(epochs):
            r.set_instance_transforms(k, wl.epoch(e).models)
            r.set_object_frames(k, wl.epoch(e).object_frames)
        V, P = wl.frame_params(fids)
        fr = make_frames(V, P, [epochs.index(f // 10) for f in fids], fids)
        frames_dev = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
        r.size_work(frames_dev.data_ptr(), n, on_device=True)   # work buffers sized for these frames, as bench.py
        nl = r.n_labels

        def buf(shape, dt):
            return torch.empty(shape, dtype=dt, device=dev)

        rgb, inst, dep = buf((n, H, W, 3), torch.uint8), buf((n, H, W), torch.int32), buf((n, H, W), torch.float32)
        crd = buf((n, H, W, 3), torch.int16)
        o_rgb, o_inst, o_dep = buf((n, H, W, 3), torch.uint8), buf((n, H, W), torch.int32), buf((n, H, W), torch.float32)
        o_crd, o_val = buf((n, H, W, 3), torch.int16), buf((n, H, W), torch.uint8)
        o_st, o_cnt = buf((n, nl, 5), torch.int32), buf((n, 3), torch.int32)
        d_map = r.lens_map(model, host_map)
        stream = torch.cuda.Stream(dev)   # (the null stream's handle 0 would mean "the context's own stream")
        torch.cuda.synchronize()

        def render():
            r.render_into(frames_dev.data_ptr(), n, True, rgb.data_ptr(), inst.data_ptr(), depth=dep.data_ptr(),
                          obj_coords=crd.data_ptr(), stream=stream.cuda_stream)

        def remap(every=True):
            r.lens_remap(n, map=d_map.data_ptr(), width=W, height=H, rgb=rgb.data_ptr(), instance=inst.data_ptr(),
                         depth=dep.data_ptr() if every else 0, obj_coords=crd.data_ptr() if every else 0,
                         lens_rgb=o_rgb.data_ptr(), lens_instance=o_inst.data_ptr(),
                         lens_depth=o_dep.data_ptr() if every else 0, lens_coords=o_crd.data_ptr() if every else 0,
                         lens_valid=o_val.data_ptr() if every else 0, lens_stats=o_st.data_ptr(),
                         lens_count=o_cnt.data_ptr() if every else 0, stream=stream.cuda_stream)

        def once(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for s in steps:
                s()
            e1.record(stream)
            e1.synchronize()
            r.synchronize()
            return e0.elapsed_time(e1) / 1e3

        variants = {"render": (render,), "render_lens": (render, remap), "lens_only": (remap,),
                    "lens_rgb_ids": (lambda: remap(False),)}
        for steps in variants.values():   # warm-up of every variant (the first renders what the others read)
            once(steps)
        times = {k: [] for k in variants}
        for _ in range(a.reps):           # alternating
            for k, steps in variants.items():
                times[k].append(once(steps))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        print(med, file=sys.stderr, flush=True)
        once((remap,))
        behind = med["render_lens"] - med["render"]
        res.update({
            "runs_s": {k: [round(t, 6) for t in v] for k, v in times.items()},
            "render_us_per_frame": round(med["render"] / n * 1e6, 2),
            "render_frames_per_s": round(n / med["render"], 1),
            "lens_behind_render_us_per_frame": round(behind / n * 1e6, 2),
            "lens_only_us_per_frame": round(med["lens_only"] / n * 1e6, 2),
            "lens_rgb_ids_us_per_frame": round(med["lens_rgb_ids"] / n * 1e6, 2),
            "extra_fraction_of_render": round(behind / med["render"], 4),
            "tb_per_s_of_the_counted_bytes_lens_only": round(n * H * W * bpp / med["lens_only"] / 1e12, 3)})
        # the torch restatement on the device, on the first --torch-frames frames
        m = min(a.torch_frames, n)
        mp = d_map.to(torch.int64)
        qx, qy = mp[..., 0], mp[..., 1]
        tagged = qx == -2 ** 31
        px, py = qx >> 8, qy >> 8
        ok = ~tagged & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        idx = torch.where(ok, py * W + px, torch.zeros_like(px)).reshape(-1)
        tx, ty = torch.where(ok, qx, torch.full_like(qx, 128)) - 128, torch.where(ok, qy, torch.full_like(qy, 128)) - 128
        x0, y0, fx, fy = tx >> 8, ty >> 8, (tx & 255).to(torch.int32), (ty & 255).to(torch.int32)
        xl, xr, yt, yb = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1), y0.clamp(0, H - 1), (y0 + 1).clamp(0, H - 1)
        taps = [((yy * W + xx).reshape(-1), (wx * wy).reshape(1, -1, 1)) for yy, wy in ((yt, 256 - fy), (yb, fy))
                for xx, wx in ((xl, 256 - fx), (xr, fx))]
        okf = ok.reshape(1, -1)

        def torch_remap():
            with torch.cuda.stream(stream):
                t_inst = torch.where(okf, inst[:m].reshape(m, -1)[:, idx], torch.full((), -1, dtype=torch.int32, device=dev))
                t_dep = torch.where(okf, dep[:m].reshape(m, -1)[:, idx], torch.full((), float("inf"), device=dev))
                t_crd = torch.where(okf[..., None], crd[:m].reshape(m, -1, 3)[:, idx], torch.zeros((), dtype=torch.int16, device=dev))
                src = rgb[:m].reshape(m, -1, 3)
                acc = torch.full((m, H * W, 3), 32768, dtype=torch.int32, device=dev)
                for i, w in taps:
                    acc += src[:, i].to(torch.int32) * w
                t_rgb = torch.where(okf[..., None], (acc >> 16).to(torch.uint8), torch.zeros((), dtype=torch.uint8, device=dev))
                return t_rgb, t_inst, t_dep, t_crd

        outs = [None]
        once((lambda: outs.__setitem__(0, torch_remap()),))
        t_torch = sorted(once((lambda: outs.__setitem__(0, torch_remap()),)) for _ in range(a.reps))[a.reps // 2]
        t_rgb, t_inst, t_dep, t_crd = outs[0]
        agree = bool(torch.equal(t_rgb.reshape(m, H, W, 3), o_rgb[:m]) and torch.equal(t_inst.reshape(m, H, W), o_inst[:m])
                     and torch.equal(t_dep.reshape(m, H, W).view(torch.int32), o_dep[:m].view(torch.int32))
                     and torch.equal(t_crd.reshape(m, H, W, 3), o_crd[:m]))
        res["torch_restatement"] = {"frames": m, "us_per_frame": round(t_torch / m * 1e6, 2), "agrees_with_the_pass": agree,
                                    "times_the_pass": round((t_torch / m) / (med["lens_only"] / n), 2),
                                    "note": "no label statistics, no validity image, no counts"}
        cnt = o_cnt.cpu().numpy().view(np.uint32)
        res["pixels_per_cause_per_frame"] = dict(zip(lens.cause_names, (int(v) for v in cnt[0])))
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
