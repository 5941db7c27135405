#!/usr/bin/env python3
"""Cost of the rig calibration: at_rigcal_solve (the k_cal_* kernels) against at_rigcal_solve_host
(the CPU twin, one core) over the same stored instants, at 64, 512 and 4096 instants of 2, 4 and 8
cameras.  The legs are alternated within a repeat; every GPU result is checked bit for bit against
the twin's.  Writes profiles/rig_calib_bench.json.

The instants are 64 distinct synthetic ones (tests/rig_calib_cases.py: 0.3 px corner noise, 3-4
tags a camera) stored again and again up to the count; the solve's work does not depend on whether
instants repeat."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rig_calib_cases as cc  # noqa: E402
import rig_pose_cases as rc  # noqa: E402

import ros_vision_amd as rva  # noqa: E402


def med(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def one(n_cams, n_instants, repeats):
    rng = np.random.default_rng(100 * n_cams + 7)
    mounts = [0, 1, 2, 3, 0, 1, 2, 3][:n_cams]
    true = [cc.true_camera(k) for k in mounts]
    start = [cc.fixed(true[0])] + [cc.perturbed(c, rng) for c in true[1:]]
    distinct = cc.make_instants(mounts, cc.robot_poses(64, rng), rng, noise_px=0.3)
    cal = rva.RigCalibrator(cc.as_create_args(start), rc.RIG_LAYOUT)
    L = rva.load_library()
    frames = [cal._frames(cc.as_add_args(inst)) for inst in distinct]
    for i in range(n_instants):
        assert L.at_rigcal_add(cal._h, frames[i % 64][0]) == 1
    cal.set_profiling(True)
    cal.solve()                                            # allocation and the first launches
    call, kern, host = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = cal.solve()
        call.append((time.perf_counter() - t0) * 1e3)
        kern.append(cal.stats()["kernel_ns"] / 1e6)
        t0 = time.perf_counter()
        want = cal.solve_host()
        host.append((time.perf_counter() - t0) * 1e3)
        assert cc.same_result(got, want)
    cal.close()
    return {"cameras": n_cams, "instants": n_instants, "call_ms": med(call), "kernels_ms": med(kern),
            "host_ms": med(host), "rms_before": got.rms_before, "rms_after": got.rms_after,
            "accepted": got.accepted, "rejected": got.rejected}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_calib_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--instants", type=int, nargs="*", default=[64, 512, 4096])
    ap.add_argument("--cameras", type=int, nargs="*", default=[2, 4, 8])
    args = ap.parse_args()
    rows = []
    for n in args.instants:
        for c in args.cameras:
            r = one(c, n, args.repeats if n < 4096 else 1)
            rows.append(r)
            print("%d cameras x %4d instants: call %.2f ms, kernels %.2f ms, host twin %.2f ms" % (
                c, n, r["call_ms"]["median"], r["kernels_ms"]["median"], r["host_ms"]["median"]), flush=True)
    with open(args.out, "w") as f:
        json.dump({"what": "at_rigcal_solve against at_rigcal_solve_host, milliseconds", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
