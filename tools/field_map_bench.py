#!/usr/bin/env python3
"""Cost of the field map: at_fieldmap_solve (the k_fm_* kernels) against at_fieldmap_solve_host (the
CPU twin, one core) over the same stored views, at 64 views x 8 tags, 512 x 22 and 4096 x 32.  The
legs are alternated within a repeat, three repeats each; every GPU result is checked byte for byte
against the twin's; minimum and maximum are kept.  Writes profiles/field_map_bench.json.

The views are 64 distinct synthetic ones (tests/field_map_cases.py: random cameras 2-4 m from the
walls, 0.3 px corner noise; a view sees a window of up to 16 consecutive tags of the map) stored
again and again up to the count; the solve's work does not depend on whether views repeat.  --e2e
adds the figures of the end-to-end GPU test (a JSON file it wrote) under "end_to_end"."""
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

import field_map_cases as fm  # noqa: E402

import ros_vision_amd as rva  # noqa: E402
from ros_vision_amd.detector import AtCamera, _detection_records, _pose_records  # noqa: E402


def med(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def one(n_tags, n_views, repeats):
    rng = np.random.default_rng(100 * n_tags + 7)
    truth = fm.field(n_tags)
    per = min(16, n_tags)
    subsets = [tuple(range(s, s + per)) for s in range(0, n_tags - per + 1, max(1, (n_tags - per) // 4 or 1))]
    distinct = fm.make_views(truth, 64, rng, noise_px=0.3, subsets=subsets)
    m = rva.FieldMapper(fm.map_tags(truth, rng))
    L = rva.load_library()
    recs = []
    for dets, poses, cam in distinct:
        darr, n = _detection_records(dets)
        recs.append((darr, _pose_records(poses, n), n, AtCamera(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)))
    for i in range(n_views):
        darr, parr, n, c = recs[i % len(recs)]
        assert L.at_fieldmap_add(m._h, darr, parr, n, C.byref(c)) == 1
    m.set_profiling(True)
    m.solve()                                              # allocation and the first launches
    call, kern, host = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = m.solve()
        call.append((time.perf_counter() - t0) * 1e3)
        kern.append(m.stats()["kernel_ns"] / 1e6)
        snap = fm.snapshot(m)
        t0 = time.perf_counter()
        m.solve_host()
        host.append((time.perf_counter() - t0) * 1e3)
        assert fm.snapshot(m) == snap
    m.close()
    return {"tags": n_tags, "views": n_views, "tags_per_view": per, "corners": got.corners, "call_ms": med(call),
            "kernels_ms": med(kern), "host_ms": med(host), "rms_before": got.rms_before, "rms_after": got.rms_after,
            "accepted": got.accepted, "rejected": got.rejected, "cov_valid": got.cov_valid}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_map_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 8, 512, 22, 4096, 32], help="views tags views tags ...")
    ap.add_argument("--e2e", help="the JSON the end-to-end GPU test wrote (AT_FIELDMAP_E2E_OUT)")
    args = ap.parse_args()
    rows = []
    for n, t in zip(args.sizes[0::2], args.sizes[1::2]):
        r = one(t, n, args.repeats)
        rows.append(r)
        print("%2d tags x %4d views: call %.2f ms, kernels %.2f ms, host twin %.2f ms" % (
            t, n, r["call_ms"]["median"], r["kernels_ms"]["median"], r["host_ms"]["median"]), flush=True)
    data = {"what": "at_fieldmap_solve against at_fieldmap_solve_host, milliseconds", "rows": rows}
    if args.e2e:
        with open(args.e2e) as f:
            data["end_to_end"] = json.load(f)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
