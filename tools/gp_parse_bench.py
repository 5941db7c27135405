#!/usr/bin/env python3
"""Game-piece output parse: the GPU route (at_gp_parse_device) against the route a user
has without it -- an async device-to-host copy of the tensors into page-locked memory, a
sync, then at_gp_parse_host on one core.

Per shape (P, C, B): both routes interleaved in one loop, wall time of each call (each ends
in a device synchronise), the median of `--calls` calls after `--warmup`.  The outputs of
the two routes are compared before anything is timed.  Writes one JSON file (default
profiles/gp_parse/bench.json).  The two kernels' time (at_gp_parse_stats[3], with
at_set_profiling on) is measured in a run of its own: `--kernels-only` times nothing else
and adds `gpu_kernels_us` to the rows of the file the first run wrote.

  python tools/gp_parse_bench.py [--calls 300] [--warmup 30] [--out FILE] [--short]
  python tools/gp_parse_bench.py --kernels-only [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(8400, 1, 1, 20), (8400, 80, 8, 40), (33600, 2, 8, 60)]   # P, C, B, objects per frame
W, H = 1280, 800                                                      # the deployed camera


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_parse", "bench.json"))
    ap.add_argument("--short", action="store_true", help="few calls, no file (for a kernel trace)")
    ap.add_argument("--kernels-only", action="store_true",
                    help="a run of its own: only the kernels' time, added to the rows of --out")
    a = ap.parse_args()
    if a.short:
        a.calls, a.warmup = 50, 5
    import torch

    import gp_parse_cases as gc
    import ros_vision_amd as rva
    if not torch.cuda.is_available():
        raise SystemExit("gp_parse_bench: no GPU")
    L = rva.load_library()
    det = rva.GpuDetector(W, H, max_batch=8, tag_size=0.0)
    res = {"device": torch.cuda.get_device_name(0), "geometry": [W, H], "calls": a.calls, "warmup": a.warmup,
           "conf_thr": 0.25, "iou_thr": 0.45, "shapes": []}
    us = lambda t: round(t * 1e6, 2)  # noqa: E731
    q = lambda v: us(statistics.quantiles(v, n=10)[8])  # noqa: E731
    if a.kernels_only:
        with open(a.out) as f:
            res = json.load(f)
    for P, nc, B, G in SHAPES:
        frames = np.stack([gc.generate(P, nc, G, seed=1000 * f + P + nc) for f in range(B)])
        dev = torch.from_numpy(frames).cuda()
        pinned = torch.empty(frames.shape, dtype=torch.float32).pin_memory()
        host = pinned.numpy()
        stride = (4 + nc) * P
        out_g, out_h = np.zeros((B, 4096), rva.GP_BOX_DTYPE), np.zeros((B, 4096), rva.GP_BOX_DTYPE)
        n_g, n_h, n1 = (C.c_int * B)(), [0] * B, C.c_int()
        stream = torch.cuda.current_stream()

        def gpu_route():
            rc = L.at_gp_parse_device(det._h, C.c_void_p(dev.data_ptr()), stride, B, P, nc, 0.25, 0.45, 640, 640,
                                      C.c_void_p(stream.cuda_stream), out_g.ctypes.data, 4096, n_g, None)
            assert rc == 0, rc

        def host_route():
            pinned.copy_(dev, non_blocking=True)
            stream.synchronize()
            for f in range(B):
                rc = L.at_gp_parse_host(host[f].ctypes.data, P, nc, 0.25, 0.45, 640, 640, W, H,
                                        out_h[f].ctypes.data, 4096, C.byref(n1))
                assert rc == 0, rc
                n_h[f] = n1.value

        if a.kernels_only:
            det.set_profiling(True)
            tk = []
            for i in range(a.warmup + a.calls):
                gpu_route()
                if i >= a.warmup:
                    tk.append(det.game_piece_parse_stats()["kernels_ns"] / 1e9)
            det.set_profiling(False)
            row = next(r for r in res["shapes"] if (r["P"], r["C"], r["B"]) == (P, nc, B))
            row["gpu_kernels_us"] = {"median": us(statistics.median(tk)), "p90": q(tk), "min": us(min(tk))}
            print(json.dumps(row), flush=True)
            continue
        gpu_route()
        host_route()
        assert list(n_g) == n_h and all(
            np.array_equal(out_g[f, :n_h[f]].view(np.uint32), out_h[f, :n_h[f]].view(np.uint32)) for f in range(B))
        tg, th = [], []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            gpu_route()
            t1 = time.perf_counter()
            host_route()
            t2 = time.perf_counter()
            if i >= a.warmup:
                tg.append(t1 - t0)
                th.append(t2 - t1)
        # the copy alone (part of the host route)
        tc = []
        for i in range(a.warmup + a.calls):
            t0 = time.perf_counter()
            pinned.copy_(dev, non_blocking=True)
            stream.synchronize()
            if i >= a.warmup:
                tc.append(time.perf_counter() - t0)
        st = det.game_piece_parse_stats()
        row = {"P": P, "C": nc, "B": B, "tensor_bytes": int(frames.nbytes), "candidates": st["candidates"],
               "boxes": st["boxes"],
               "gpu_route_us": {"median": us(statistics.median(tg)), "p90": q(tg), "min": us(min(tg))},
               "host_route_us": {"median": us(statistics.median(th)), "p90": q(th), "min": us(min(th))},
               "host_route_copy_us": {"median": us(statistics.median(tc))}}
        row["host_over_gpu"] = round(row["host_route_us"]["median"] / row["gpu_route_us"]["median"], 3)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    det.close()
    if not a.short:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
