#!/usr/bin/env python3
"""What the rig pose (k_rig, at_rig_solve) costs, measured in one process on one GPU.

Every camera is a detector of its own given one 640 x 480 GRAY8 view of tests/rig_pose_cases.py
(front, right, left, wall_a in turn: 3, 3, 4 and 3 layout tags).  Legs, alternated, `--repeats`
times each (the median of the repeats and their range are kept):

  b1    max_batch = 1, rigs of 2, 4 and 8 cameras, the members' batches collected;
  b32   8 cameras, max_batch = 32, every frame of a member's batch its view: 32 instants.

Per leg:
  solve_call_us   at_rig_solve on the host clock, p50 of `--calls` calls (stream wait on the
                  members' events, launch, synchronise, copy from the mapped records);
  k_rig_us        k_rig between its own HIP events (at_rig_stats, profiling on for a member);
  host_us         at_rig_pose_host for every instant on one host core, from the members'
                  collected detections and poses (arguments built once), p50;
  k_field_us      the members' own k_field (at_field_stats, the same layout set, profiling on):
                  per member and summed -- what one field pose per camera costs on the device.

Writes one JSON file (default profiles/rig_pose_bench.json) and prints it.

  python tools/rig_pose_bench.py [--calls 300] [--repeats 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 640, 480
VIEWS = ["front", "right", "left", "wall_a"]


def spread(v, digits=2):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_pose_bench.json"))
    args = ap.parse_args()
    import torch
    import ros_vision_amd as rva
    from ros_vision_amd import detector as D
    import rig_pose_cases as rc
    import tag_scenes as ts
    if not torch.cuda.is_available():
        raise SystemExit("rig_pose_bench needs the GPU: nothing is measured without it")
    L = rva.load_library()
    codes = dict(rva.family_entries())
    frames = {v: rc.render_view(v, ts.draw_tag, codes, ts.blank) for v in VIEWS}
    no_dist = rva.DistCoeffs(0, 0, 0, 0, 0)

    class Rig:
        def __init__(self, n_cams, batch):
            self.views = [VIEWS[i % len(VIEWS)] for i in range(n_cams)]
            self.batch = batch
            self.dets = []
            for v in self.views:
                g = rc.VIEWS[v][5]
                cm = rva.CameraMatrix(fx=g.fx, cx=g.cx, fy=g.fy, cy=g.cy)
                self.dets.append(rva.GpuDetector(W, H, cm, no_dist, max_batch=batch))
            self.detect()
            self.rig = rva.RigSolver(self.dets, [rc.view_mount(v) for v in self.views], rc.RIG_LAYOUT)
            self.buf = (D.AtRigPose * batch)()
            self.tags = sum(len(rc.VIEWS[v][0]) for v in self.views)

        def detect(self):
            for d, v in zip(self.dets, self.views):
                d.detect_batch([frames[v]] * self.batch, rva.AT_FMT_GRAY8)

        def solve_call_us(self):
            us = []
            for _ in range(args.calls + 20):
                t0 = time.perf_counter()
                n = L.at_rig_solve(self.rig._h, self.buf, self.batch)
                us.append((time.perf_counter() - t0) * 1e6)
            assert n == self.batch and all(self.buf[f].n_tags == self.tags for f in range(self.batch))
            return float(np.percentile(us[20:], 50))

        def k_rig_us(self):
            self.dets[0].set_profiling(True)
            ns = []
            for _ in range(60):
                L.at_rig_solve(self.rig._h, self.buf, self.batch)
                ns.append(self.rig.stats()["kernel_ns"])
            self.dets[0].set_profiling(False)
            return float(np.median(ns[10:])) / 1e3

        def host_us(self):
            tarr, nt = D._field_tags(rc.RIG_LAYOUT)
            ext, _n = D._rig_extrinsics([rc.view_mount(v) for v in self.views], len(self.views))
            calls, keep = [], []
            for f in range(self.batch):
                arr = (D.AtRigHostCam * len(self.dets))()
                for i, (d, v) in enumerate(zip(self.dets, self.views)):
                    darr, n = D._detection_records(d.detections(f))
                    poses = d.poses(f)
                    parr = (D.AtPose * max(1, n))()
                    for k, p in enumerate(poses):
                        parr[k].id = int(p.id)
                        parr[k].R[:] = [float(x) for x in np.asarray(p.R).reshape(9)]
                        parr[k].t[:] = [float(x) for x in np.asarray(p.t).reshape(3)]
                    g = rc.VIEWS[v][5]
                    c = D.AtCamera(fx=g.fx, fy=g.fy, cx=g.cx, cy=g.cy)
                    keep.append((darr, parr, c))
                    arr[i].dets, arr[i].poses, arr[i].n, arr[i].cam, arr[i].extr = darr, parr, n, C.pointer(c), ext[i]
                calls.append(arr)
            out = D.AtRigPose()
            us = []
            for _ in range(max(20, args.calls // max(1, self.batch // 4))):
                t0 = time.perf_counter()
                for arr in calls:
                    L.at_rig_pose_host(arr, len(self.dets), tarr, nt, 0, rva.TAG_SIZE, C.byref(out))
                us.append((time.perf_counter() - t0) * 1e6)
            assert out.n_tags == self.tags and bytes(out) == bytes(self.buf[self.batch - 1])   # the twin, bit for bit
            return float(np.percentile(us[5:], 50))

        def k_field_us(self):
            per = []
            for d, v in zip(self.dets, self.views):
                d.set_field_layout(rc.RIG_LAYOUT)
                d.set_profiling(True)
                ns = []
                for _ in range(30):
                    d.detect_batch([frames[v]] * self.batch, rva.AT_FMT_GRAY8)
                    ns.append(d.field_stats()["kernel_ns"])
                d.set_profiling(False)
                d.set_field_layout(None)
                per.append(float(np.median(ns[5:])) / 1e3)
            self.detect()          # the members' last batches as the other legs expect them
            return per

        def close(self):
            self.rig.close()
            for d in self.dets:
                d.close()

    result = {"gpu": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats, "legs": {}}
    rigs = {"b1_2_cams": Rig(2, 1), "b1_4_cams": Rig(4, 1), "b1_8_cams": Rig(8, 1), "b32_8_cams": Rig(8, 32)}
    cols = {k: {"solve_call_us": [], "k_rig_us": [], "host_us": [], "k_field_sum_us": [], "k_field_per_member_us": []}
            for k in rigs}
    for _ in range(args.repeats):
        for name, r in rigs.items():
            c = cols[name]
            r.solve_call_us()                                     # (warm)
            c["solve_call_us"].append(r.solve_call_us())
            c["k_rig_us"].append(r.k_rig_us())
            c["host_us"].append(r.host_us())
            per = r.k_field_us()
            c["k_field_sum_us"].append(sum(per))
            c["k_field_per_member_us"].append(float(np.median(per)))
    for name, r in rigs.items():
        leg = {k: spread(v) for k, v in cols[name].items()}
        leg.update(cameras=len(r.dets), instants=r.batch, tags_per_instant=r.tags)
        result["legs"][name] = leg
        r.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
