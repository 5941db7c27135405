#!/usr/bin/env python3
"""What the field pose (k_field, at_set_field_layout) costs, measured in one process on one GPU.

Legs, alternated, `--repeats` times each (the median of the repeats and their range are kept):

  latency     one 640 x 480 GRAY8 frame resident in HBM (five tags of the test layout on two
              walls, tests/field_pose_cases.py), max_batch = 1: at_detect_device, the p50 of
              `--calls` calls on the host clock (every call ends in the wait for the batch),
              with the layout off and on;
  throughput  192 frames of 1280 x 720 YUYV (the stream of synth.stream_frame, 15 tags each)
              resident in HBM, max_batch = 192, ONE detector, enqueue + collect of `--batches`
              batches: frames per second with the layout off and on.  (bench.py's figure is
              higher: it keeps several detectors' batches in flight; this is one detector, the
              same for both legs.)  The layout puts every id of the family somewhere on one
              wall: the positions are not those of the picture, which costs k_field the same
              12 iterations -- they are fixed -- over up to 16 tags per frame.

Then, in a run of its own with at_set_profiling on (direct launches, HIP events around
k_field): its own time at B = 1 and at B = 192, from at_field_stats.

The off legs are the baseline.  `--lib PATH` loads another build of the library (e.g. the parent
commit's, which has no field pose: only the off legs run) for the comparison across commits; run
it as a process of its own and merge with `--merge-baseline FILE`.

Writes one JSON file (default profiles/field_pose_bench.json) and prints it.

  python tools/field_pose_bench.py [--calls 1000] [--batches 200] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAT_W, LAT_H = 640, 480
THR_W, THR_H, THR_B = 1280, 720, 192


def spread(v, digits=4):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--merge-baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_pose_bench.json"))
    args = ap.parse_args()
    if args.lib:
        os.environ["AT_HIP_LIB"] = os.path.abspath(args.lib)
    import torch
    import ros_vision_amd as rva
    from ros_vision_amd import synth
    import field_pose_cases as fc
    import tag_scenes as ts
    if not torch.cuda.is_available():
        raise SystemExit("field_pose_bench needs the GPU: nothing is measured without it")
    have_field = hasattr(rva.load_library(), "at_set_field_layout")
    legs = ("off", "on") if have_field else ("off",)
    result = {"gpu": torch.cuda.get_device_name(0), "library": args.lib or "this tree's", "field_pose": have_field,
              "calls": args.calls, "batches": args.batches, "repeats": args.repeats}

    # ---- latency: B = 1, one HBM frame ----
    g = fc.GPU_CAM
    cam = rva.CameraMatrix(fx=g.fx, cx=g.cx, fy=g.fy, cy=g.cy)
    img = fc.render_scene("five", ts.draw_tag, dict(rva.family_entries()), ts.blank)[0]
    frame = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    det = rva.GpuDetector(LAT_W, LAT_H, cam, rva.DistCoeffs(0, 0, 0, 0, 0), max_batch=1)

    def set_layout(d, layout, on):
        if have_field:
            d.set_field_layout(layout if on else None)

    def lat_leg(on):
        set_layout(det, fc.GPU_LAYOUT, on)
        for _ in range(20):
            det.detect_device(frame.data_ptr(), LAT_W * LAT_H, 1, rva.AT_FMT_GRAY8, counts_only=True)
        us = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            n = det.detect_device(frame.data_ptr(), LAT_W * LAT_H, 1, rva.AT_FMT_GRAY8, counts_only=True)
            us.append((time.perf_counter() - t0) * 1e6)
        assert n == [5]
        if on:
            assert det.field_poses()[0].n_tags == 5
        return float(np.percentile(us, 50))

    lat = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k in legs:
            lat[k].append(lat_leg(k == "on"))
    result["latency_b1_p50_us"] = {k: spread(v, 2) for k, v in lat.items()}
    kern = {}
    if have_field:
        set_layout(det, fc.GPU_LAYOUT, True)
        det.set_profiling(True)
        ns = []
        for _ in range(args.calls):
            det.detect_device(frame.data_ptr(), LAT_W * LAT_H, 1, rva.AT_FMT_GRAY8, counts_only=True)
            ns.append(det.field_stats()["kernel_ns"])
        det.set_profiling(False)
        kern["b1_5_tags_us"] = spread([x / 1e3 for x in ns[10:]], 2)
    det.close()

    # ---- throughput: 720p, batch 192, one detector ----
    distinct = [synth.stream_frame(THR_W, THR_H, f)[0] for f in range(8)]
    batch = torch.from_numpy(np.stack([distinct[f % 8] for f in range(THR_B)])).cuda()
    torch.cuda.synchronize()
    stride = THR_W * THR_H * 2
    wall = [(tid, np.eye(3), np.array([0.3 * (tid % 30), 0.3 * (tid // 30), 0.0])) for tid in range(587)]
    det = rva.GpuDetector(THR_W, THR_H, max_batch=THR_B)

    def batch_once():
        det.enqueue_device(batch.data_ptr(), stride, THR_B, rva.AT_FMT_YUYV)
        return det.collect(counts_only=True)

    def thr_leg(on):
        set_layout(det, wall, on)
        for _ in range(3):
            counts = batch_once()
        t0 = time.perf_counter()
        for _ in range(args.batches):
            counts = batch_once()
        dt = time.perf_counter() - t0
        assert min(counts) >= 10
        return THR_B * args.batches / dt

    fps = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k in legs:
            fps[k].append(thr_leg(k == "on"))
    result["throughput_720p_b192_frames_per_s"] = {k: spread(v, 0) for k, v in fps.items()}
    if have_field:
        set_layout(det, wall, True)
        batch_once()
        st = det.field_stats()
        result["throughput_tags_used_per_frame"] = round(st["tags_used"] / THR_B, 2)
        det.set_profiling(True)
        ns = []
        for _ in range(12):
            batch_once()
            ns.append(det.field_stats()["kernel_ns"])
        det.set_profiling(False)
        kern["b192_us"] = spread([x / 1e3 for x in ns[2:]], 2)
        result["k_field_kernel_time"] = kern
    det.close()

    if args.merge_baseline and os.path.exists(args.merge_baseline):
        with open(args.merge_baseline) as f:
            base = json.load(f)
        result["parent_commit_off"] = {k: base[k] for k in ("latency_b1_p50_us", "throughput_720p_b192_frames_per_s")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
