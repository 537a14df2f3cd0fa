"""Cost of the JPEG RGB files made on the GPU (csg_encode_jpeg: k_jpg_blocks +
k_jpg_emit + k_jpg_layout + k_jpg_offsets + k_jpg_pack) on C3 frames.

C3 at 1080p, device-resident batches of F frames (device outputs,
Renderer.render_into and the pass on one stream), timed with HIP events around
the enqueue, variants alternated, median of --reps after one warm-up of each
(the method of tools/bop_mask_cost.py):

  render        rgb + instance + depth + stats
  jpeg_420      ... + csg_encode_jpeg at --quality in 4:2:0
  jpeg_444      ... + csg_encode_jpeg at --quality in 4:4:4
  alone_420/444 the pass on an RGB image already in place

The bytes per frame stand against the RGB PNG (csg_encode_files) and Pillow's
files of the same --host-frames frames of the batch, and the comparison is the
host route measured in the same process on those frames: the raw RGB into page-locked
memory, then Pillow (libjpeg, the same quality, sampling and restart rows) in
--host-threads threads; where Pillow is absent, the copy alone.

    python tools/jpeg_cost.py --frames 480 --out profiles/jpeg/cost.json
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--host-frames", type=int, default=48)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "jpeg", "cost.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from constructionsceneposeestimation_amd.workload import Workload
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_cost: needs the GPU (no CPU timing stands in for it)")
    wl = Workload("C3", seed=0, width=a.width, height=a.height)
    n = a.frames
    fids = list(range(n))
    epochs = sorted({f // 10 for f in fids})
    r = Renderer(wl.scene, wl.width, wl.height, max_frames=n)
    for k, e in enumerate(epochs):
        r.set_instance_transforms(k, wl.epoch(e).models)
    V, P = wl.frame_params(fids)
    fr = make_frames(V, P, [epochs.index(f // 10) for f in fids], fids)
    H, W, L = wl.height, wl.width, r._n_inst_labels
    dev = torch.device("cuda", 0)
    frames_dev = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
    r.size_work(frames_dev.data_ptr(), n, on_device=True)   # work buffers sized for these frames, as bench.py
    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    inst = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    stats = torch.empty((n, L, 5), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)   # (the null stream's handle 0 would mean "the context's own stream")
    out_cap = n * (H * W // 2 + 4096)
    out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    fo = {ss: torch.empty(n + 1, dtype=torch.int64, device=dev) for ss in ("420", "444")}

    def render():
        r.render_into(frames_dev.data_ptr(), n, True, rgb.data_ptr(), inst.data_ptr(), depth.data_ptr(),
                      stats=stats.data_ptr(), stream=stream.cuda_stream)

    def jpeg(ss):
        return lambda: r.encode_jpeg(n, rgb=rgb.data_ptr(), out=out.data_ptr(), out_capacity=out_cap,
                                     file_offsets=fo[ss].data_ptr(), quality=a.quality, subsampling=ss,
                                     stream=stream.cuda_stream)

    variants = {"render": (render,), "jpeg_420": (render, jpeg("420")), "jpeg_444": (render, jpeg("444")),
                "alone_420": (jpeg("420"),), "alone_444": (jpeg("444"),)}

    def once(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for s in steps:
            s()
        e1.record(stream)
        e1.synchronize()
        r.synchronize()
        return e0.elapsed_time(e1) / 1e3

    for steps in variants.values():     # warm-up of every variant
        once(steps)
    offs = {ss: t.cpu().numpy() for ss, t in fo.items()}
    totals = {ss: int(o[n]) for ss, o in offs.items()}
    assert max(totals.values()) <= out_cap, "the JPEG files overflow the output"
    times = {k: [] for k in variants}
    for _ in range(a.reps):             # alternating
        for k, steps in variants.items():
            times[k].append(once(steps))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}

    # the RGB PNG of a sample of the same frames (the GPU's RLE deflate)
    hn = min(a.host_frames, n)
    _, png_need = r.encode_files(hn, W, H, ("rgb_png",), None, rgb=rgb.data_ptr())
    # the host route on the same sample: raw RGB to page-locked memory, then Pillow in threads
    pin = torch.empty((hn, H, W, 3), dtype=torch.uint8, pin_memory=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    pin.copy_(rgb[:hn], non_blocking=True)
    torch.cuda.synchronize(dev)
    t_copy = time.perf_counter() - t0
    host = {"frames": hn, "threads": a.host_threads, "rgb_copy_us_per_frame": round(t_copy / hn * 1e6, 2)}
    try:
        from PIL import Image
    except ImportError:
        Image = None
        host["pillow"] = None
    if Image is not None:
        rgb_h = pin.numpy()
        for ss, code in (("420", 2), ("444", 0)):
            def host_one(f):
                b = io.BytesIO()
                Image.fromarray(rgb_h[f]).save(b, "JPEG", quality=a.quality, subsampling=code, restart_marker_rows=1)
                return b.tell()
            with ThreadPoolExecutor(a.host_threads) as ex:
                list(ex.map(host_one, range(min(hn, a.host_threads))))     # warm-up
                t0 = time.perf_counter()
                nbytes = sum(ex.map(host_one, range(hn)))
                t_enc = time.perf_counter() - t0
            behind = (med[f"jpeg_{ss}"] - med["render"]) / n
            host[ss] = {"pillow_us_per_frame": round(t_enc / hn * 1e6, 2), "pillow_bytes_per_frame": round(nbytes / hn),
                        "us_per_frame": round((t_copy + t_enc) / hn * 1e6, 2),
                        "over_encode_behind": round((t_copy + t_enc) / hn / behind, 1) if behind > 0 else None}
    r.close()
    res = {"workload": "C3", "width": W, "height": H, "frames": n, "quality": a.quality,
           "method": f"HIP events around the enqueue on one stream, device outputs, variants alternated, median of "
                     f"{a.reps} after one warm-up each",
           "bytes_per_frame": {"raw_rgb": 3 * W * H, "jpeg_420": round(totals["420"] / n),
                               "jpeg_444": round(totals["444"] / n)},
           "bytes_per_frame_of_the_host_sample": {"frames": hn, "rgb_png": round(png_need / hn),
                                                  "jpeg_420": round(int(offs["420"][hn]) / hn),
                                                  "jpeg_444": round(int(offs["444"][hn]) / hn)},
           "runs_s": {k: [round(t, 6) for t in v] for k, v in times.items()},
           "us_per_frame": {k: round(v / n * 1e6, 2) for k, v in med.items()},
           "encode_behind_render": {ss: {"us_per_frame": round((med[f"jpeg_{ss}"] - med["render"]) / n * 1e6, 2),
                                         "fraction_of_one_render": round((med[f"jpeg_{ss}"] - med["render"])
                                                                         / med["render"], 4)}
                                    for ss in ("420", "444")},
           "host_route": host}
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
