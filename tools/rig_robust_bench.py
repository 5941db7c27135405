#!/usr/bin/env python3
"""What the robust rig pose (k_rig_robust, at_rig_solve_robust) costs beside the plain one (k_rig,
at_rig_solve) on the same batches, measured in one process on one GPU.

Every camera is a detector of its own given one 640 x 480 GRAY8 view of tests/rig_pose_cases.py
(front, right, left, wall_a in turn).  Rigs of 2, 4 and 8 cameras, 1 instant (max_batch = 1) and
32 instants (max_batch = 32, every frame of a member's batch its view).  Per rig three layouts:

  clean   the true layout: the robust solve drops nothing (one fit);
  one     layout tag 4 displaced by (0.25, 0.10, 0) m;
  two     layout tags 4 and 7 displaced (rigs of 2 cameras do not see tag 7).

What the robust solve dropped and how many rounds it ran is recorded with every leg.  Per leg, the
median of `--repeats` repeats and their range:

  k_rig_us          k_rig between its own HIP events (at_rig_stats, profiling on for a member):
                    the yardstick -- k_rig is the parent commit's kernel, unchanged;
  k_rig_robust_us   k_rig_robust likewise (at_rig_robust_stats);
  solve_call_us / solve_robust_call_us   the two calls on the host clock, p50 of `--calls`;
  host_us / host_robust_us   at_rig_pose_host / at_rig_pose_robust_host for every instant on one
                    host core, from the members' collected detections and poses, p50.

Writes one JSON file (default profiles/rig_robust_bench.json) and prints it.

  python tools/rig_robust_bench.py [--calls 200] [--repeats 3] [--out FILE]
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_robust_bench.json"))
    args = ap.parse_args()
    import torch
    import ros_vision_amd as rva
    from ros_vision_amd import detector as D
    import rig_pose_cases as rc
    import rig_robust_cases as rr
    import tag_scenes as ts
    if not torch.cuda.is_available():
        raise SystemExit("rig_robust_bench needs the GPU: nothing is measured without it")
    L = rva.load_library()
    codes = dict(rva.family_entries())
    frames = {v: rc.render_view(v, ts.draw_tag, codes, ts.blank) for v in VIEWS}
    no_dist = rva.DistCoeffs(0, 0, 0, 0, 0)
    layouts = {"clean": rc.RIG_LAYOUT, "one": rr.displaced(rc.RIG_LAYOUT, {4}), "two": rr.displaced(rc.RIG_LAYOUT, {4, 7})}
    cfg = D.AtRigRobustConfig(huber_px=2.0, reject_px=6.0, max_rounds=3, min_keep=2)

    class Rig:
        def __init__(self, n_cams, batch):
            self.views = [VIEWS[i % len(VIEWS)] for i in range(n_cams)]
            self.batch = batch
            self.dets = []
            for v in self.views:
                g = rc.VIEWS[v][5]
                cm = rva.CameraMatrix(fx=g.fx, cx=g.cx, fy=g.fy, cy=g.cy)
                self.dets.append(rva.GpuDetector(W, H, cm, no_dist, max_batch=batch))
            for d, v in zip(self.dets, self.views):
                d.detect_batch([frames[v]] * batch, rva.AT_FMT_GRAY8)
            mounts = [rc.view_mount(v) for v in self.views]
            self.rigs = {k: rva.RigSolver(self.dets, mounts, lay) for k, lay in layouts.items()}
            self.buf = (D.AtRigPose * batch)()
            self.info = (D.AtRigRobustInfo * batch)()
            self.host_args = self._host_args()

        def _host_args(self):
            calls, keep = [], []
            for f in range(self.batch):
                arr, _n, k = D._rig_host_cams([(d.detections(f), d.poses(f), rc.VIEWS[v][5], rc.view_mount(v))
                                               for d, v in zip(self.dets, self.views)])
                keep.append(k)
                calls.append(arr)
            self._keep = keep
            return calls

        def solve(self, which, robust):
            h = self.rigs[which]._h
            if robust:
                return L.at_rig_solve_robust(h, C.byref(cfg), self.buf, self.info, self.batch)
            return L.at_rig_solve(h, self.buf, self.batch)

        def call_us(self, which, robust):
            us = []
            for _ in range(args.calls + 20):
                t0 = time.perf_counter()
                n = self.solve(which, robust)
                us.append((time.perf_counter() - t0) * 1e6)
            assert n == self.batch
            return float(np.percentile(us[20:], 50))

        def kernel_us(self, which, robust):
            self.dets[0].set_profiling(True)
            ns = []
            for _ in range(60):
                self.solve(which, robust)
                st = self.rigs[which].robust_stats() if robust else self.rigs[which].stats()
                ns.append(st["kernel_ns"])
            self.dets[0].set_profiling(False)
            return float(np.median(ns[10:])) / 1e3

        def host_us(self, which, robust):
            tarr, nt = D._field_tags(layouts[which])
            out, info = D.AtRigPose(), D.AtRigRobustInfo()
            n = len(self.dets)
            us = []
            for _ in range(max(20, args.calls // max(1, self.batch // 4))):
                t0 = time.perf_counter()
                for arr in self.host_args:
                    if robust:
                        L.at_rig_pose_robust_host(arr, n, tarr, nt, 0, rva.TAG_SIZE, C.byref(cfg), C.byref(out),
                                                  C.byref(info))
                    else:
                        L.at_rig_pose_host(arr, n, tarr, nt, 0, rva.TAG_SIZE, C.byref(out))
                us.append((time.perf_counter() - t0) * 1e6)
            self.solve(which, robust)                                # the twin, bit for bit
            assert bytes(out) == bytes(self.buf[self.batch - 1])
            assert not robust or bytes(info) == bytes(self.info[self.batch - 1])
            return float(np.percentile(us[5:], 50))

        def close(self):
            for r in self.rigs.values():
                r.close()
            for d in self.dets:
                d.close()

    result = {"gpu": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats,
              "config": {"huber_px": 2.0, "reject_px": 6.0, "max_rounds": 3, "min_keep": 2}, "legs": {}}
    names = ("k_rig_us", "k_rig_robust_us", "solve_call_us", "solve_robust_call_us", "host_us", "host_robust_us")
    for batch in (1, 32):
        for n_cams in (2, 4, 8):
            r = Rig(n_cams, batch)
            for which in layouts:
                cols = {k: [] for k in names}
                for _ in range(args.repeats):
                    for robust in (False, True):
                        tag = "_robust" if robust else ""
                        cols["k_rig%s_us" % tag].append(r.kernel_us(which, robust))
                        cols["solve%s_call_us" % tag].append(r.call_us(which, robust))
                        cols["host%s_us" % tag].append(r.host_us(which, robust))
                leg = {k: spread(v) for k, v in cols.items()}
                r.solve(which, True)
                leg.update(cameras=n_cams, instants=batch, tags_per_instant=int(r.buf[0].n_tags),
                           tags_dropped_per_instant=int(r.info[0].n_rejected), rounds=int(r.info[0].rounds),
                           starved=int(r.info[0].starved))
                result["legs"]["b%d_%d_cams_%s" % (batch, n_cams, which)] = leg
            r.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
