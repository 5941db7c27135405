#!/usr/bin/env python3
"""Cost of the camera calibration: at_camcal_solve (the k_cc_* kernels) against at_camcal_solve_host
(the CPU twin, one core) over the same stored views, at 32, 512 and 4096 views of 4 and 16 tags, all
nine parameters free.  The legs are alternated within a repeat; every GPU result is checked bit for
bit against the twin's; minimum and maximum are kept.  Writes profiles/camera_calib_bench.json.

The views are 20 distinct synthetic ones (tests/camera_calib_cases.py: the cam13 poses, 0.3 px
corner noise) stored again and again up to the count; the solve's work does not depend on whether
views repeat."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import camera_calib_cases as cc  # noqa: E402

import ros_vision_amd as rva  # noqa: E402
from ros_vision_amd.detector import _detection_records  # noqa: E402


def med(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def one(n_tags, n_views, repeats):
    rng = np.random.default_rng(100 * n_tags + 7)
    ids = None if n_tags == 16 else {5, 6, 9, 10}
    cam, board, tag_size, distinct = cc.cam13_case(rng=rng, noise_px=0.3, ids=ids)
    cal = rva.CameraCalibrator(*cc.CAM13_SIZE, board, tag_size, free=cc.ALL, init=cc.off_start(cam))
    L = rva.load_library()
    recs = [_detection_records(v) for v in distinct]
    for i in range(n_views):
        assert L.at_camcal_add(cal._h, *recs[i % len(recs)]) == 1
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
    return {"tags": n_tags, "views": n_views, "corners": got.corners, "call_ms": med(call), "kernels_ms": med(kern),
            "host_ms": med(host), "rms_before": got.rms_before, "rms_after": got.rms_after,
            "accepted": got.accepted, "rejected": got.rejected}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_calib_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--views", type=int, nargs="*", default=[32, 512, 4096])
    ap.add_argument("--tags", type=int, nargs="*", default=[4, 16])
    args = ap.parse_args()
    rows = []
    for n in args.views:
        for t in args.tags:
            r = one(t, n, args.repeats if n < 4096 else 2)
            rows.append(r)
            print("%2d tags x %4d views: call %.2f ms, kernels %.2f ms, host twin %.2f ms" % (
                t, n, r["call_ms"]["median"], r["kernels_ms"]["median"], r["host_ms"]["median"]), flush=True)
    with open(args.out, "w") as f:
        json.dump({"what": "at_camcal_solve against at_camcal_solve_host, milliseconds", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
