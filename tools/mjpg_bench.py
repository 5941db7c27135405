#!/usr/bin/env python3
"""Host-fed MJPG against host-fed YUYV, measured in one process on one GPU.

The frames are the bench's synthetic 1280x720 boards (ros_vision_amd.stream), once
packed as YUYV in page-locked memory (at_enqueue_host, what bench.py's host-ingest
leg times) and once JPEG-encoded at quality 80, 4:2:2 (at_enqueue_mjpg).  Both go
through the same round-robin loop over the same detector instances, so the two
rates differ only by the input path.  Also reported: the host decode time per frame,
k_mjpg_idct's time per batch and the bytes per frame that cross the link.

A colour leg follows (at_mjpg_set_color): the same boards tinted, so that the chroma
planes carry coefficients, through the same loop once with colour off and once with it
on -- frames/s, link bytes per frame, and the time of the two colour kernels
(k_mjpg_idct_chroma + k_mjpg_bgr) per batch.

Writes one JSON file (default profiles/mjpg_bench.json) and prints it.

  python tools/mjpg_bench.py [--batch 32] [--instances 4] [--steps 24] [--threads 1,4,16]

--entropy measures the entropy decode on the GPU (at_mjpg_set_device_entropy) instead: after a
plane check of a whole batch, legs with the switch on (1 host thread) alternate with the
host-decode legs (1, 4, 16 threads) in this process, each repeated; then the same pair with
colour on, k_mjpg_entropy's time and the synchronisation rounds per piece size S, and the
latency of single frames with the switch on and off.  Writes profiles/mjpg_entropy_bench.json.
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_mjpg(dets, jpgs, batch, nsteps):
    """StreamRunner's loop with at_enqueue_mjpg: batch k on instance k mod n, collected
    n-1 enqueues later (the host decodes batch k while the batches before it compute)."""
    ni, inflight, ndet = len(dets), [], 0
    for s in range(nsteps):
        d = dets[s % ni]
        off = (s * batch) % len(jpgs)
        d.enqueue_mjpg([jpgs[(off + j) % len(jpgs)] for j in range(batch)])
        inflight.append(d)
        if len(inflight) == ni:
            ndet += sum(inflight.pop(0).collect(counts_only=True))
    while inflight:
        ndet += sum(inflight.pop(0).collect(counts_only=True))
    return ndet


def tinted_pool(yuyv, W, H, quality):
    """The pool's frames with real chroma (so the chroma planes carry coefficients), 4:2:2."""
    from PIL import Image
    tinted = []
    yy, xx = np.mgrid[0:H, 0:W]
    for f in yuyv:
        g = np.ascontiguousarray(f[:, 0::2]).astype(np.int32)
        rgb = np.stack([np.clip(g + 40 * np.sin(xx / 9.0), 0, 255), g, np.clip(g - 35 * np.cos(yy / 7.0), 0, 255)], -1)
        b = io.BytesIO()
        Image.fromarray(rgb.astype(np.uint8)).save(b, "JPEG", quality=quality, subsampling=1)
        tinted.append(b.getvalue())
    return tinted


def _timed(dets, jpgs, batch, steps):
    import torch
    run_mjpg(dets, jpgs, batch, len(dets))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_mjpg(dets, jpgs, batch, steps)
    torch.cuda.synchronize()
    return steps * batch / (time.perf_counter() - t0)


def _spread(v):
    v = sorted(v)
    return {"frames_per_s": [round(x, 1) for x in v], "median": round(v[len(v) // 2], 1), "min": round(v[0], 1),
            "max": round(v[-1], 1)}


def entropy_bench(args, rva, jpgs, tinted, res):
    """The entropy decode on the GPU (at_mjpg_set_device_entropy) against the host decode:
    the same frames through the same loop and detectors, the legs alternated and repeated so
    that the spread of identical legs is in the file beside the differences."""
    import torch
    W, H, B = args.width, args.height, args.batch
    # self-check before anything is timed: a whole batch, switch on against off and Pillow
    on, off = (rva.GpuDetector(W, H, max_batch=B, debug_taps=True) for _ in range(2))
    on.set_mjpg_device_entropy(True)
    batch = [jpgs[j % len(jpgs)] for j in range(B)]
    n_on = sum(len(x) for x in on.detect_mjpg_batch(batch))
    n_off = sum(len(x) for x in off.detect_mjpg_batch(batch))
    from PIL import Image
    im = Image.open(io.BytesIO(batch[B - 1]))
    im.draft("L", im.size)
    res["self_check"] = {
        "frames": B, "planes_equal_switch_off": all(np.array_equal(on.copy_gray(f), off.copy_gray(f)) for f in range(B)),
        "last_plane_equals_pillow": bool(np.array_equal(on.copy_gray(B - 1), np.asarray(im.convert("L")))),
        "detections": {"on": n_on, "off": n_off}, "sync_rounds": on.mjpg_stats()["sync_rounds"]}
    on.close()
    off.close()
    if not (res["self_check"]["planes_equal_switch_off"] and res["self_check"]["last_plane_equals_pillow"]):
        raise SystemExit("self-check failed: " + json.dumps(res["self_check"]))

    dets = [rva.GpuDetector(W, H, max_batch=B) for _ in range(args.instances)]

    def setup(dev, threads, color=False, subseq=128):
        for d in dets:
            d.set_mjpg_device_entropy(dev)
            d.set_mjpg_threads(threads)
            d.set_mjpg_color(color)
            d.set_mjpg_subseq(subseq)

    legs = [("device_entropy_1_thread", True, 1)] + [("host_decode_%d_threads" % t, False, t)
                                                       for t in (int(v) for v in args.threads.split(","))]
    fps = {name: [] for name, _, _ in legs}
    link = {}
    for _ in range(args.repeats):
        for name, dev, nt in legs:
            setup(dev, nt)
            fps[name].append(_timed(dets, jpgs, B, args.steps))
            s = dets[0].mjpg_stats()
            link[name] = {"link_bytes_per_frame": round(s["device_bytes"] / B, 1),
                          "compressed_bytes_per_frame": round(s["compressed_bytes"] / B, 1),
                          "host_ms_per_frame_wall": round(s["host_decode_us"] / 1e3 / B, 4)}
    res["legs"] = {name: dict(_spread(v), **link[name]) for name, v in fps.items()}

    cfps = {"device_entropy_1_thread": [], "host_decode_1_threads": []}
    for _ in range(args.repeats):
        for name, dev in (("device_entropy_1_thread", True), ("host_decode_1_threads", False)):
            setup(dev, 1, color=True)
            cfps[name].append(_timed(dets, tinted, B, args.steps))
            s = dets[0].mjpg_stats()
            link[name] = {"link_bytes_per_frame": round(s["device_bytes"] / B, 1)}
    res["legs_color_on"] = {name: dict(_spread(v), **link[name]) for name, v in cfps.items()}

    # k_mjpg_entropy alone (HIP events while stage profiling is on), per piece size S
    d = dets[0]
    d.set_profiling(True)
    sweep = []
    for S in (16, 32, 64, 128, 256):
        setup(True, 1, subseq=S)
        ns, rounds = [], 0
        for i in range(12):
            d.enqueue_mjpg([jpgs[(i + j) % len(jpgs)] for j in range(B)])
            d.collect(counts_only=True)
            st = d.mjpg_stats()
            ns.append(st["entropy_kernel_ns"])
            rounds = max(rounds, st["sync_rounds"])
        ns = sorted(ns[2:])
        sweep.append({"subseq_bytes": S, "k_mjpg_entropy_ms_per_batch_median": round(ns[len(ns) // 2] / 1e6, 4),
                      "min": round(ns[0] / 1e6, 4), "most_sync_rounds": rounds})
    d.set_profiling(False)
    for e in sweep:
        setup(True, 1, subseq=e["subseq_bytes"])
        e["frames_per_s"] = round(_timed(dets, jpgs, B, args.steps), 1)
    res["subseq_sweep"] = {"frames": B, "how": "hipEventElapsedTime around the launch, 10 batches each", "points": sweep}
    for d in dets:
        d.close()

    # latency: one frame at a time, switch off and on in alternating blocks
    lat = {"on": [], "off": []}
    one = {k: rva.GpuDetector(W, H) for k in lat}
    one["on"].set_mjpg_device_entropy(True)
    for blk in range(6):
        for k in ("off", "on"):
            for i in range(60):
                t0 = time.perf_counter()
                one[k].detect_mjpg(jpgs[i % len(jpgs)])
                if blk and i >= 10:
                    lat[k].append((time.perf_counter() - t0) * 1e3)
    for v in one.values():
        v.close()
    res["latency_batch_1_ms"] = {k: {"p50": round(float(np.percentile(v, 50)), 4), "p90": round(float(np.percentile(v, 90)), 4),
                                     "n": len(v)} for k, v in lat.items()}
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--pool", type=int, default=16, help="distinct frames")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--instances", type=int, default=4)
    ap.add_argument("--steps", type=int, default=24, help="timed batches per leg")
    ap.add_argument("--threads", default="1,4,16", help="host decode thread counts to measure")
    ap.add_argument("--quality", type=int, default=80)
    ap.add_argument("--out", default=None)
    ap.add_argument("--entropy", action="store_true",
                    help="the device entropy decode against the host decode (profiles/mjpg_entropy_bench.json)")
    ap.add_argument("--repeats", type=int, default=3, help="--entropy: repetitions of every leg")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mjpg_entropy_bench.json" if args.entropy else "mjpg_bench.json")

    import torch
    from PIL import Image

    import ros_vision_amd as rva
    from ros_vision_amd.stream import StreamRunner, stream_pool

    W, H, B = args.width, args.height, args.batch
    yuyv = stream_pool(W, H, args.pool)
    jpgs = []
    for f in yuyv:
        g = np.ascontiguousarray(f[:, 0::2])
        b = io.BytesIO()
        Image.fromarray(np.stack([g] * 3, -1)).save(b, "JPEG", quality=args.quality, subsampling=1)
        jpgs.append(b.getvalue())

    if args.entropy:
        res = {"width": W, "height": H, "batch": B, "instances": args.instances, "steps": args.steps,
               "pool": args.pool, "repeats": args.repeats,
               "jpeg": {"quality": args.quality, "sampling": "4:2:2", "encoder": "Pillow (libjpeg-turbo)"},
               "device": torch.cuda.get_device_name(0)}
        entropy_bench(args, rva, jpgs, tinted_pool(yuyv, W, H, args.quality), res)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return

    dets = [rva.GpuDetector(W, H, max_batch=B) for _ in range(args.instances)]
    res = {"width": W, "height": H, "batch": B, "instances": args.instances, "steps": args.steps, "pool": args.pool,
           "jpeg": {"quality": args.quality, "sampling": "4:2:2", "encoder": "Pillow (libjpeg-turbo)"},
           "device": torch.cuda.get_device_name(0)}

    # the decoded plane is what Pillow decodes (one frame, before anything is timed)
    chk = rva.GpuDetector(W, H, debug_taps=True)
    n_mjpg = len(chk.detect_mjpg(jpgs[0]))
    im = Image.open(io.BytesIO(jpgs[0]))
    im.draft("L", im.size)
    res["plane_equals_pillow"] = bool(np.array_equal(chk.copy_gray(), np.asarray(im.convert("L"))))
    res["detections_frame0"] = {"mjpg": n_mjpg, "yuyv": len(chk.detect(yuyv[0]))}
    chk.close()

    # host-fed YUYV: the comparison figure, same process, same detectors
    pinned = torch.from_numpy(yuyv).pin_memory()
    hrun = StreamRunner(dets, pinned.data_ptr(), 2 * W * H, args.pool, B, host=True)
    hrun.run(len(dets))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hrun.run(args.steps)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    res["yuyv_host_fed"] = {"frames_per_s": round(args.steps * B / el, 1), "link_bytes_per_frame": 2 * W * H}

    res["mjpg_host_fed"] = []
    for nt in [int(v) for v in args.threads.split(",")]:
        for d in dets:
            d.set_mjpg_threads(nt)
        run_mjpg(dets, jpgs, B, len(dets))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_mjpg(dets, jpgs, B, args.steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        s = dets[0].mjpg_stats()
        res["mjpg_host_fed"].append({
            "threads": nt, "frames_per_s": round(args.steps * B / el, 1),
            "host_decode_ms_per_frame_wall": round(s["host_decode_us"] / 1e3 / B, 4),
            "host_decode_ms_per_frame_per_thread": round(s["host_decode_us"] / 1e3 / B * min(nt, B), 4)})
    s = dets[0].mjpg_stats()
    res["mjpg_link_bytes_per_frame"] = round(s["device_bytes"] / B, 1)
    res["mjpg_compressed_bytes_per_frame"] = round(s["compressed_bytes"] / B, 1)
    res["mjpg_dense_frames_per_batch"] = s["dense_frames"]

    # k_mjpg_idct alone: HIP events around it while stage profiling is on
    d = dets[0]
    d.set_profiling(True)
    ns = []
    for i in range(12):
        d.enqueue_mjpg([jpgs[(i + j) % len(jpgs)] for j in range(B)])
        d.collect(counts_only=True)
        ns.append(d.mjpg_stats()["idct_kernel_ns"])
    d.set_profiling(False)
    ns = sorted(ns[2:])
    res["k_mjpg_idct_ms_per_batch"] = {"median": round(ns[len(ns) // 2] / 1e6, 4), "min": round(ns[0] / 1e6, 4),
                                       "frames": B, "how": "hipEventElapsedTime around the launch, 10 batches"}
    # colour: tinted frames (real chroma), colour off and on through the same loop
    tinted = tinted_pool(yuyv, W, H, args.quality)
    chk = rva.GpuDetector(W, H)
    chk.set_mjpg_color(True)
    chk.detect_mjpg(tinted[0])
    want = np.asarray(Image.open(io.BytesIO(tinted[0])).convert("RGB"))[:, :, ::-1]
    res["mjpg_color"] = {"image_equals_pillow": bool(np.array_equal(chk.copy_bgr(), want)), "legs": []}
    chk.close()
    nt = max(int(v) for v in args.threads.split(","))
    for d in dets:
        d.set_mjpg_threads(nt)
    for color in (False, True):
        for d in dets:
            d.set_mjpg_color(color)
        run_mjpg(dets, tinted, B, len(dets))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_mjpg(dets, tinted, B, args.steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        s = dets[0].mjpg_stats()
        res["mjpg_color"]["legs"].append({
            "color": color, "threads": nt, "frames_per_s": round(args.steps * B / el, 1),
            "link_bytes_per_frame": round(s["device_bytes"] / B, 1),
            "compressed_bytes_per_frame": round(s["compressed_bytes"] / B, 1),
            "host_decode_ms_per_frame_wall": round(s["host_decode_us"] / 1e3 / B, 4)})
    d = dets[0]
    d.set_profiling(True)
    ns = []
    for i in range(12):
        d.enqueue_mjpg([tinted[(i + j) % len(tinted)] for j in range(B)])
        d.collect(counts_only=True)
        ns.append(d.mjpg_stats()["color_kernels_ns"])
    d.set_profiling(False)
    ns = sorted(ns[2:])
    res["mjpg_color"]["color_kernels_ms_per_batch"] = {
        "median": round(ns[len(ns) // 2] / 1e6, 4), "min": round(ns[0] / 1e6, 4), "frames": B,
        "how": "hipEventElapsedTime around k_mjpg_idct_chroma + k_mjpg_bgr, 10 batches"}
    for d in dets:
        d.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
