#!/usr/bin/env python3
"""What the ideal corners (at_set_undistort) cost, measured in one process on one GPU.

Legs, alternated, `--repeats` times each (the median of the repeats and their range are kept):

  latency     one 640 x 480 GRAY8 frame resident in HBM (five tags of the test layout seen
              through the barrel lens of tests/undistort_cases.py), max_batch = 1:
              at_detect_device, the p50 of `--calls` calls on the host clock, mode off and on
              (the pose-fused k_decode: both of its waves carry the stage);
  k_pose      192 frames of 1280 x 720 YUYV (synth.stream_frame, 15 tags each) resident in HBM,
              max_batch = 192, at_set_profiling on (direct launches, HIP events around every
              stage): k_pose's mean time per batch, mode off and on (four lanes per detection);
  throughput  the same batch without profiling, ONE detector, enqueue + collect of `--batches`
              batches: frames per second, mode off and on.  The detector has the reference test
              camera's lens, so with the mode on every corner is inverted.

`--bench-lines FILE` merges the means and spreads of bench.py's own line run alternately with
this tree's library and the parent commit's (the mode is off there: the two should not differ
beyond either side's spread); the job that produces FILE runs bench.py as processes of their own.

Writes one JSON file (default profiles/undistort_bench.json) and prints it.

  python tools/undistort_bench.py [--calls 1000] [--batches 100] [--repeats 3] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

LAT_W, LAT_H = 640, 480
THR_W, THR_H, THR_B = 1280, 720, 192
LEGS = ("off", "on")


def spread(v, digits=4):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--profiled-batches", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_bench.json"))
    args = ap.parse_args()
    import torch
    import ros_vision_amd as rva
    from ros_vision_amd import synth
    import field_pose_cases as fc
    import tag_scenes as ts
    import undistort_cases as uc
    if not torch.cuda.is_available():
        raise SystemExit("undistort_bench needs the GPU: nothing is measured without it")
    result = {"gpu": torch.cuda.get_device_name(0), "calls": args.calls, "batches": args.batches, "repeats": args.repeats}

    # ---- latency: B = 1, one HBM frame ----
    cam, dist = uc.camera_of(rva, uc.GPU_LENS)
    img = uc.warp(fc.render_scene("five", ts.draw_tag, dict(rva.family_entries()), ts.blank)[0], uc.GPU_LENS)
    frame = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    det = rva.GpuDetector(LAT_W, LAT_H, cam, dist, max_batch=1)

    def lat_leg(on):
        det.set_undistort(on)
        for _ in range(20):
            det.detect_device(frame.data_ptr(), LAT_W * LAT_H, 1, rva.AT_FMT_GRAY8, counts_only=True)
        us = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            n = det.detect_device(frame.data_ptr(), LAT_W * LAT_H, 1, rva.AT_FMT_GRAY8, counts_only=True)
            us.append((time.perf_counter() - t0) * 1e6)
        assert n == [5]
        assert det.undistort_stats()["ideal"] == (5 if on else 0)
        return float(np.percentile(us, 50))

    lat = {k: [] for k in LEGS}
    for _ in range(args.repeats):
        for k in LEGS:
            lat[k].append(lat_leg(k == "on"))
    result["latency_b1_p50_us"] = {k: spread(v, 2) for k, v in lat.items()}
    det.close()

    # ---- 720p, batch 192, one detector ----
    distinct = [synth.stream_frame(THR_W, THR_H, f)[0] for f in range(8)]
    batch = torch.from_numpy(np.stack([distinct[f % 8] for f in range(THR_B)])).cuda()
    torch.cuda.synchronize()
    stride = THR_W * THR_H * 2
    det = rva.GpuDetector(THR_W, THR_H, max_batch=THR_B)

    def batch_once():
        det.enqueue_device(batch.data_ptr(), stride, THR_B, rva.AT_FMT_YUYV)
        return det.collect(counts_only=True)

    def thr_leg(on):
        det.set_undistort(on)
        for _ in range(3):
            counts = batch_once()
        t0 = time.perf_counter()
        for _ in range(args.batches):
            counts = batch_once()
        dt = time.perf_counter() - t0
        assert min(counts) >= 10
        return THR_B * args.batches / dt

    def pose_leg(on):
        det.set_undistort(on)
        batch_once()
        det.set_profiling(True)
        for _ in range(args.profiled_batches):
            batch_once()
        names, batches = det.stage_times()
        det.set_profiling(False)
        assert batches == args.profiled_batches
        return names["k_pose"] * 1e3

    fps, pose = {k: [] for k in LEGS}, {k: [] for k in LEGS}
    for _ in range(args.repeats):
        for k in LEGS:
            fps[k].append(thr_leg(k == "on"))
        for k in LEGS:
            pose[k].append(pose_leg(k == "on"))
    result["throughput_720p_b192_frames_per_s"] = {k: spread(v, 0) for k, v in fps.items()}
    result["k_pose_b192_us"] = {k: spread(v, 2) for k, v in pose.items()}
    det.set_undistort(True)
    batch_once()
    st = det.undistort_stats()
    result["detections_per_batch"] = {"ideal": st["ideal"], "not_invertible": st["not_invertible"]}
    det.close()

    if args.bench_lines and os.path.exists(args.bench_lines):
        with open(args.bench_lines) as f:
            result["bench_py_line"] = json.load(f)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
