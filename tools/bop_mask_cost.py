"""Cost of the per-object mask PNGs made on the GPU (csg_encode_span_masks:
k_mp_paint + k_mp_rows + k_mp_layout + k_mp_offsets + k_mp_zero + k_mp_emit +
k_mp_pack), for BOP's mask_visib and mask folders, on C3 frames.

C3 at 1080p, device-resident batches of F frames (device outputs,
Renderer.render_into and the passes on one stream), timed with HIP events around
the enqueue, variants alternated, median of --reps after one warm-up of each
(the method of tools/amodal_rle_cost.py):

  render        rgb + instance + depth + stats
  spans         ... + csg_mask_spans + csg_amodal_spans for the dynamic kinds
  masks         ... + csg_encode_span_masks twice: the visible and the amodal
                mask of every dynamic object with amodal pixels
  masks_alone   the two encode passes on spans already in place

The comparison is the only route the parent commit had to the same files: the
dense ids to the host, then zlib at level 1 per object mask in 16 threads
(zlib releases the GIL).  The tool measures that route on --host-frames frames
of the same batch: the copy of one-byte ids into page-locked memory, and the
threads' wall time for both masks of every listed object.

    python tools/bop_mask_cost.py --frames 480 --out profiles/bop_masks/cost.json
"""
import argparse
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--host-frames", type=int, default=48)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "bop_masks", "cost.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from constructionsceneposeestimation_amd import masks
    from constructionsceneposeestimation_amd.crops import eligible_labels
    from constructionsceneposeestimation_amd.renderer import DEFAULT_SPAN_CAPACITY, Renderer, make_frames
    from constructionsceneposeestimation_amd.workload import Workload
    if not torch.cuda.is_available():
        raise SystemExit("bop_mask_cost: needs the GPU (no CPU timing stands in for it)")
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
    el = eligible_labels(wl.scene)
    frames_dev = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
    r.size_work(frames_dev.data_ptr(), n, on_device=True)   # work buffers sized for these frames, as bench.py
    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    inst = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    stats = torch.empty((n, L, 5), dtype=torch.int32, device=dev)
    v_off = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
    a_off = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
    a_stats = torch.empty((n, L, 5), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)   # (the null stream's handle 0 would mean "the context's own stream")
    v_cap = a_cap = DEFAULT_SPAN_CAPACITY
    v_sp = torch.empty((n, v_cap, 2), dtype=torch.int32, device=dev)
    a_sp = torch.empty((n, a_cap, 2), dtype=torch.int32, device=dev)

    def render():
        r.render_into(frames_dev.data_ptr(), n, True, rgb.data_ptr(), inst.data_ptr(), depth.data_ptr(),
                      stats=stats.data_ptr(), stream=stream.cuda_stream)

    def spans():
        r.mask_spans(n, instance=inst.data_ptr(), spans=v_sp.data_ptr(), span_offsets=v_off.data_ptr(),
                     capacity=v_cap, n_labels=L, stream=stream.cuda_stream)
        r.amodal_spans(fr, spans=a_sp.data_ptr(), span_offsets=a_off.data_ptr(), capacity=a_cap,
                       amodal_stats=a_stats.data_ptr(), eligible=el, stream=stream.cuda_stream)

    # the items: every dynamic object with amodal pixels (what generate --outputs bop lists)
    render()
    spans()
    stream.synchronize()
    r.synchronize()
    assert int(v_off.cpu().numpy().view(np.uint32)[:, L].max()) <= v_cap, "visible spans overflow the capacity"
    assert int(a_off.cpu().numpy().view(np.uint32)[:, L].max()) <= a_cap, "amodal spans overflow the capacity"
    px = a_stats.cpu().numpy().view(np.uint32)[:, :, 0]
    items = np.array([(f, l) for f in range(n) for l in range(L) if el[l] and px[f, l] > 0], np.uint32).reshape(-1, 2)
    ni = len(items)
    fo = [torch.empty(ni + 1, dtype=torch.int64, device=dev) for _ in range(2)]
    out_cap = ni * (H * (24 + W // 64) + 256)
    outs = [torch.empty(out_cap, dtype=torch.uint8, device=dev) for _ in range(2)]

    def encode():
        for k, (sp, off, cap) in enumerate(((v_sp, v_off, v_cap), (a_sp, a_off, a_cap))):
            r.encode_span_masks(items, spans=sp.data_ptr(), span_offsets=off.data_ptr(), capacity=cap,
                                out=outs[k].data_ptr(), out_capacity=out_cap, file_offsets=fo[k].data_ptr(),
                                n_frames=n, n_labels=L, height=H, width=W, stream=stream.cuda_stream)

    variants = {"render": (render,), "spans": (render, spans), "masks": (render, spans, encode),
                "masks_alone": (encode,)}

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
    totals = [int(t.cpu().numpy()[ni]) for t in fo]
    assert max(totals) <= out_cap, "the mask files overflow the output"
    times = {k: [] for k in variants}
    for _ in range(a.reps):             # alternating
        for k, steps in variants.items():
            times[k].append(once(steps))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}

    # the parent's route on a sample: ids to the host, zlib level 1 per object mask in threads
    hn = min(a.host_frames, n)
    ids8 = (inst[:hn] + 1).to(torch.uint8)          # the one-byte wire of host-output batches
    pin = torch.empty((hn, H, W), dtype=torch.uint8, pin_memory=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    pin.copy_(ids8, non_blocking=True)
    torch.cuda.synchronize(dev)
    t_copy = time.perf_counter() - t0
    ids_h = pin.numpy()
    ao, asp = a_off[:hn].cpu().numpy().view(np.uint32), a_sp[:hn].cpu().numpy().view(np.uint32)
    host_items = [(int(f), int(l)) for f, l in items if f < hn]
    amodal = {(f, l): masks.spans_to_mask((H, W), masks.label_spans(asp[f], ao[f], l)) for f, l in host_items}

    def host_one(fl):
        f, l = fl
        nb = 0
        for m in (ids_h[f] == l + 1, amodal[fl]):
            raw = np.zeros((H, W + 1), np.uint8)
            raw[:, 1:] = m * np.uint8(255)
            nb += len(zlib.compress(raw, 1))
        return nb
    with ThreadPoolExecutor(a.host_threads) as ex:
        list(ex.map(host_one, host_items[:a.host_threads]))     # warm-up
        t0 = time.perf_counter()
        host_bytes = sum(ex.map(host_one, host_items))
        t_zlib = time.perf_counter() - t0
    r.close()
    enc = med["masks"] - med["spans"]
    res = {"workload": "C3", "width": W, "height": H, "frames": n, "n_labels": L,
           "method": f"HIP events around the enqueue on one stream, device outputs, variants alternated, median of "
                     f"{a.reps} after one warm-up each",
           "items": {"per_kind": ni, "objects_per_frame": round(ni / n, 2)},
           "mask_file_bytes_per_frame": {"mask_visib": round(totals[0] / n), "mask": round(totals[1] / n),
                                         "both": round(sum(totals) / n)},
           "mean_file_bytes": round(sum(totals) / (2 * max(ni, 1))),
           "runs_s": {k: [round(t, 6) for t in v] for k, v in times.items()},
           "us_per_frame": {k: round(v / n * 1e6, 2) for k, v in med.items()},
           "encode_behind_render_and_spans": {"us_per_frame": round(enc / n * 1e6, 2),
                                              "fraction_of_one_render": round(enc / med["render"], 4)},
           "encode_alone": {"us_per_frame": round(med["masks_alone"] / n * 1e6, 2),
                            "fraction_of_one_render": round(med["masks_alone"] / med["render"], 4)},
           "host_route": {"frames": hn, "threads": a.host_threads, "items": len(host_items),
                          "ids_copy_us_per_frame": round(t_copy / hn * 1e6, 2),
                          "zlib_level1_us_per_frame": round(t_zlib / hn * 1e6, 2),
                          "zlib_bytes_per_frame": round(host_bytes / hn),
                          "us_per_frame": round((t_copy + t_zlib) / hn * 1e6, 2),
                          "over_encode_behind": round((t_copy + t_zlib) / hn / (enc / n), 1) if enc > 0 else None}}
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
