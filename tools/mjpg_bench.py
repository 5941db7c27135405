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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mjpg_bench.json"))
    args = ap.parse_args()

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
    tinted = []
    yy, xx = np.mgrid[0:H, 0:W]
    for f in yuyv:
        g = np.ascontiguousarray(f[:, 0::2]).astype(np.int32)
        rgb = np.stack([np.clip(g + 40 * np.sin(xx / 9.0), 0, 255), g, np.clip(g - 35 * np.cos(yy / 7.0), 0, 255)], -1)
        b = io.BytesIO()
        Image.fromarray(rgb.astype(np.uint8)).save(b, "JPEG", quality=args.quality, subsampling=1)
        tinted.append(b.getvalue())
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
