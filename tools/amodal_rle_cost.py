"""Cost of the full-frame amodal spans (csg_amodal_spans: k_amodal_plane +
k_aplane_count + k_span_scan + k_aplane_emit) and their span counts on C3 frames.

C3 at 1080p, device-resident batches of F frames (device outputs,
Renderer.render_into and the passes on one stream), timed with HIP events around
the enqueue, variants alternated, median of --reps after one warm-up of each
(the method of tools/mask_rle_cost.py):

  render           rgb + instance + depth + stats
  visible_spans    ... + csg_mask_spans
  amodal_dynamic   render + csg_amodal_spans for the crops' dynamic kinds
  amodal_all       render + csg_amodal_spans for every label

`variant - render` is a pass behind a render.  The comparison that matters is the
only way the parent commit had to the same data: one more render of the frame per
eligible object present, with every other instance zeroed; the tool counts those
objects and prices them at the measured render.  The span totals (mean, p99, max)
are what a default capacity is set from (mask_spans_host's rule: the largest seen
plus three eighths); the scratch bytes and frame ranges are the pass's own
arithmetic restated.

The number of atomicOr per frame comes from a debug build with a device counter
(-DCSG_AMODAL_COUNT_ATOMICS=1), in a run of its own, in a child process:

    python tools/amodal_rle_cost.py --build-count-lib build/libcsg_count.so   # no GPU needed
    python tools/amodal_rle_cost.py --frames 480 --count-lib build/libcsg_count.so \\
        --out profiles/amodal_rle/cost.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANE_CAP = 64 << 20   # csg_amodal_spans' default scratch bound (csg_passes.cpp)


def build_count_lib(path):
    from constructionsceneposeestimation_amd.build import FLAGS, SOURCES, hipcc
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    cmd = [hipcc(), *FLAGS, "-DCSG_AMODAL_COUNT_ATOMICS=1", "-o", path, *SOURCES]
    print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)


def setup(a):
    import numpy as np
    import torch
    from constructionsceneposeestimation_amd.renderer import Renderer, make_frames
    from constructionsceneposeestimation_amd.workload import Workload
    if not torch.cuda.is_available():
        raise SystemExit("amodal_rle_cost: needs the GPU (no CPU timing stands in for it)")
    wl = Workload("C3", seed=0, width=a.width, height=a.height)
    n = a.frames
    fids = list(range(n))
    epochs = sorted({f // 10 for f in fids})
    r = Renderer(wl.scene, wl.width, wl.height, max_frames=n)
    for k, e in enumerate(epochs):
        r.set_instance_transforms(k, wl.epoch(e).models)
    V, P = wl.frame_params(fids)
    fr = make_frames(V, P, [epochs.index(f // 10) for f in fids], fids)
    return wl, r, fr, np, torch


def count_atomics(a):
    """Child process, CSG_LIB = the counting build: plane atomics per frame for both label sets."""
    import ctypes as C
    from constructionsceneposeestimation_amd.crops import eligible_labels
    wl, r, fr, np, torch = setup(a)
    fn = r.lib.csg_debug_amodal_atomics
    fn.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    n, L, cap = a.frames, r._n_inst_labels, 8
    dev = torch.device("cuda", 0)
    spans = torch.empty((n, cap, 2), dtype=torch.int32, device=dev)   # (overflows: only the planes matter here)
    offs = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
    st = torch.empty((n, L, 5), dtype=torch.int32, device=dev)
    out = {}
    for name, el in (("dynamic", eligible_labels(wl.scene)), ("all", None)):
        v = C.c_ulonglong()
        assert fn(None, 1) == 0
        r.amodal_spans(fr, spans=spans.data_ptr(), span_offsets=offs.data_ptr(), capacity=cap,
                       amodal_stats=st.data_ptr(), eligible=el)
        r.synchronize()
        assert fn(C.byref(v), 0) == 0
        px = st.cpu().numpy().view(np.uint32)[:, :, 0].astype(np.int64)
        out[name] = {"atomic_or_per_frame": round(v.value / n, 1), "set_pixels_per_frame": round(float(px.sum()) / n, 1),
                     "set_pixels_per_atomic": round(float(px.sum()) / max(v.value, 1), 2)}
    r.close()
    print("ATOMICS " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--out", default=os.path.join("profiles", "amodal_rle", "cost.json"))
    ap.add_argument("--build-count-lib", metavar="PATH", help="only build the counting library there (no GPU)")
    ap.add_argument("--count-lib", metavar="PATH", help="the counting library: adds the atomics per frame")
    ap.add_argument("--count-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.build_count_lib:
        build_count_lib(a.build_count_lib)
        return
    if a.count_child:
        count_atomics(a)
        return
    from constructionsceneposeestimation_amd.crops import eligible_labels
    from constructionsceneposeestimation_amd.renderer import DEFAULT_SPAN_CAPACITY
    wl, r, fr, np, torch = setup(a)
    n, H, W, L = a.frames, wl.height, wl.width, r._n_inst_labels
    dev = torch.device("cuda", 0)
    el_dyn = eligible_labels(wl.scene)
    frames_dev = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
    r.size_work(frames_dev.data_ptr(), n, on_device=True)   # work buffers sized for these frames, as bench.py
    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    inst = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    stats = torch.empty((n, L, 5), dtype=torch.int32, device=dev)
    offs = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
    a_offs = torch.empty((n, L + 1), dtype=torch.int32, device=dev)
    a_stats = torch.empty((n, L, 5), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)   # (the null stream's handle 0 would mean "the context's own stream")
    cap = DEFAULT_SPAN_CAPACITY
    spans = torch.empty((n, cap, 2), dtype=torch.int32, device=dev)

    def amodal(el, c, sp):
        r.amodal_spans(fr, spans=sp.data_ptr(), span_offsets=a_offs.data_ptr(), capacity=c,
                       amodal_stats=a_stats.data_ptr(), eligible=el, stream=stream.cuda_stream)

    # a capacity every frame fits, found by one pass with every label (offsets are exact on overflow)
    a_cap = 8
    a_spans = torch.empty((n, a_cap, 2), dtype=torch.int32, device=dev)
    amodal(None, a_cap, a_spans)
    stream.synchronize()
    r.synchronize()
    tot_all = a_offs.cpu().numpy().view(np.uint32)[:, L].astype(np.int64)
    a_cap = int(tot_all.max()) + 3 * int(tot_all.max()) // 8
    a_spans = torch.empty((n, a_cap, 2), dtype=torch.int32, device=dev)

    def render():
        r.render_into(frames_dev.data_ptr(), n, True, rgb.data_ptr(), inst.data_ptr(), depth.data_ptr(),
                      stats=stats.data_ptr(), stream=stream.cuda_stream)

    def visible():
        r.mask_spans(n, instance=inst.data_ptr(), spans=spans.data_ptr(), span_offsets=offs.data_ptr(),
                     capacity=cap, stream=stream.cuda_stream)

    variants = {"render": (render,), "visible_spans": (render, visible),
                "amodal_dynamic": (render, lambda: amodal(el_dyn, a_cap, a_spans)),
                "amodal_all": (render, lambda: amodal(None, a_cap, a_spans))}

    def once(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for s in steps:
            s()
        e1.record(stream)
        e1.synchronize()
        r.synchronize()
        return e0.elapsed_time(e1) / 1e3

    info = {}
    for k, steps in variants.items():   # warm-up of every variant; the amodal ones leave their totals
        once(steps)
        if k.startswith("amodal"):
            t = a_offs.cpu().numpy().view(np.uint32)[:, L].astype(np.int64)
            px = a_stats.cpu().numpy().view(np.uint32)[:, :, 0].astype(np.int64)
            vis = stats.cpu().numpy().view(np.uint32)[:, :, 0].astype(np.int64)
            el = el_dyn.astype(bool)[:L] if k == "amodal_dynamic" else np.ones(L, bool)
            present = (px > 0).sum(1)
            P = int(el.sum())
            per_frame = P * ((H + 31) // 32) * W * 4
            bound = int(os.environ.get("CSG_AMODAL_PLANE_CAP", PLANE_CAP))
            per_range = min(n, 65535, max(1, bound // per_frame)) if per_frame else n
            sp = a_spans.cpu().numpy().view(np.uint32)
            agree = all(int(sp[f, :t[f], 1].sum()) == int(px[f].sum()) for f in range(min(n, 32)))
            info[k] = {"eligible_labels": P,
                       "spans_per_frame": {"mean": round(float(t.mean()), 1), "p50": int(np.percentile(t, 50)),
                                           "p99": int(np.percentile(t, 99)), "max": int(t.max()), "min": int(t.min())},
                       "largest_plus_three_eighths": int(t.max()) + 3 * int(t.max()) // 8,
                       "objects_present_per_frame": {"mean": round(float(present.mean()), 2), "max": int(present.max())},
                       "amodal_pixels_per_frame": round(float(px.sum()) / n, 1),
                       "visible_pixels_of_those_labels_per_frame": round(float(vis[:, el].sum()) / n, 1),
                       "labels_with_amodal_larger_than_visible_per_frame":
                           round(float(((px > vis) & (px > 0)).sum()) / n, 2),
                       "scratch_bytes_per_frame": per_frame, "scratch_bound_bytes": bound,
                       "scratch_bytes": per_frame * per_range, "frames_per_range": per_range,
                       "ranges": -(-n // per_range), "span_lengths_sum_to_amodal_stats_pixels": bool(agree)}
    times = {k: [] for k in variants}
    for _ in range(a.reps):             # alternating
        for k, steps in variants.items():
            times[k].append(once(steps))
    r.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    res = {"workload": "C3", "width": W, "height": H, "frames": n, "n_labels": L, "amodal_capacity": a_cap,
           "method": f"HIP events around the enqueue on one stream, device outputs, variants alternated, median of "
                     f"{a.reps} after one warm-up each",
           "runs_s": {k: [round(t, 6) for t in v] for k, v in times.items()},
           "us_per_frame": {k: round(v / n * 1e6, 2) for k, v in med.items()},
           "ratio_to_one_render": {k: round(v / med["render"], 4) for k, v in med.items()}}
    for k in ("visible_spans", "amodal_dynamic", "amodal_all"):
        extra = med[k] - med["render"]
        d = {"pass_behind_render_us_per_frame": round(extra / n * 1e6, 2),
             "pass_as_fraction_of_one_render": round(extra / med["render"], 4)}
        if k in info:
            d.update(info[k])
            # the parent's only way: one more render of the frame per eligible object present
            m = info[k]["objects_present_per_frame"]["mean"]
            d["parent_way_us_per_frame"] = round(m * med["render"] / n * 1e6, 2)
            d["parent_way_over_this_pass"] = round(m * med["render"] / extra, 1) if extra > 0 else None
        res[k] = d
    if a.count_lib:
        env = dict(os.environ, CSG_LIB=os.path.abspath(a.count_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--count-child", "--frames", str(min(n, 60))]
        for name, v in (("--width", a.width), ("--height", a.height)):
            if v:
                cmd += [name, str(v)]
        out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout
        line = [x for x in out.splitlines() if x.startswith("ATOMICS ")][-1]
        res["atomics"] = dict(json.loads(line[len("ATOMICS "):]), frames=min(n, 60),
                              note="debug build with a device counter, a run of its own")
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
