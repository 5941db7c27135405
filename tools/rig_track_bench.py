#!/usr/bin/env python3
"""Cost of the rig track: at_rigtrack_solve (the k_trk_* kernels) against at_rigtrack_solve_host (the
CPU twin, one core) over the same window, at N = 8 / 32 / 64 instants x 2 / 8 cameras, iters = 6.
Both sides are warmed: every instant's own start is already kept (on the device and in the twin), as
it is for all but the newest instant when a window slides at camera rate.  The legs are alternated
within a repeat, three repeats each; every GPU result is checked byte for byte against the twin's;
minimum and maximum are kept.  The call is timed with profiling off; one more solve per repeat with
profiling on gives the kernels' times from HIP events (at_rigtrack_stats), the serial solve kernel
per launch among them.  Writes profiles/rig_track_bench.json.

The windows are tests/rig_track_cases.py's: a walk near rig_pose_cases.ROBOT, mounts 0..3 (twice for
8 cameras), 0.3 px corner noise, noisy odometry, every eighth instant without a tag."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rig_track_cases as tc  # noqa: E402

import ros_vision_amd as rva  # noqa: E402

ITERS = 6


def med(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def one(n, n_cams, repeats):
    rng = np.random.default_rng(100 * n + n_cams)
    mounts = [0, 1, 2, 3, 0, 1, 2, 3][:n_cams]
    win = tc.make_window(mounts, tc.walk(n, rng), rng, noise_px=0.3, tagless=tuple(range(3, n, 8)), noisy_odom=True)
    trk = tc.tracker(rva, tc.cameras(mounts), win, iters=ITERS)
    trk.solve()                                            # allocation, the own starts, the first launches
    trk.solve_host()
    call, host, kern, accum, solve = [], [], [], [], []
    for _ in range(repeats):
        trk.set_profiling(False)
        t0 = time.perf_counter()
        got = trk.solve()
        call.append((time.perf_counter() - t0) * 1e6)
        snap = (bytes(trk.record), trk.instant_records())
        t0 = time.perf_counter()
        trk.solve_host()
        host.append((time.perf_counter() - t0) * 1e6)
        assert (bytes(trk.record), trk.instant_records()) == snap
        trk.set_profiling(True)
        trk.solve()
        st = trk.stats()
        kern.append(st["kernel_ns"] / 1e3)
        accum.append(st["accum_ns"] / 1e3 / (ITERS + 1))
        solve.append(st["solve_ns"] / 1e3 / (ITERS + 1))
    tags = int(sum(i.n_tags for i in trk.instants()))
    trk.close()
    return {"instants": n, "cameras": n_cams, "tags": tags,
            "call_us": med(call), "host_us": med(host), "kernels_us": med(kern), "accum_per_launch_us": med(accum),
            "solve_per_launch_us": med(solve), "launches": 2 + 2 * (ITERS + 1) - 1, "accepted": got.accepted,
            "rejected": got.rejected, "rms_after": got.rms_after, "cov_valid": got.cov_valid}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_track_bench.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[8, 2, 8, 8, 32, 2, 32, 8, 64, 2, 64, 8],
                    help="instants cameras instants cameras ...")
    args = ap.parse_args()
    rows = []
    for n, c in zip(args.sizes[0::2], args.sizes[1::2]):
        r = one(n, c, args.repeats)
        rows.append(r)
        print("%2d instants x %d cameras: call %.0f us, kernels %.0f us (accumulate %.1f, solve %.1f per launch), "
              "host twin %.0f us" % (n, c, r["call_us"]["median"], r["kernels_us"]["median"],
                                     r["accum_per_launch_us"]["median"], r["solve_per_launch_us"]["median"],
                                     r["host_us"]["median"]), flush=True)
    data = {"what": "at_rigtrack_solve against at_rigtrack_solve_host, iters = %d, microseconds" % ITERS, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
