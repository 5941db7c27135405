#!/usr/bin/env python3
"""The annotated image's way out, raw against JPEG, measured in one process on one GPU.

Per size (1920x1080 and 1280x720) one detector and one annotated synthetic board (tinted, so
the chroma planes carry coefficients).  Every iteration detects the host BGR8 frame (not
timed: it stages the image) and then times one call, alternating between
  (a) at_annotate_staged into a page-locked buffer: W x H x 3 bytes over the link, and
  (b) at_annotate_jpeg (quality 95, 4:2:0) into a page-locked buffer: the stream's bytes,
each a host clock around a call that ends in a stream synchronise.  Reported: p50 / p99 of
both, the bytes per frame over the link, the encode kernels' time by HIP events
(at_jpeg_stats while profiling is on, median of 10), and for scale Pillow's encode of the same
annotated image on one host thread.  The stream is checked against the host encoder first.

Writes one JSON file (default profiles/jpeg_out_bench.json) and prints it.

  python tools/jpeg_out_bench.py [--iters 300] [--quality 95]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * (len(v) - 1) + 0.5))]


def measure(rva, W, H, iters, quality):
    import torch
    from PIL import Image
    from ros_vision_amd import synth
    L = rva.load_library()
    gray = synth.render_board(W, H, seed=766, ntags=6)[0].astype(np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    bgr = np.stack([np.clip(gray - 35 * np.cos(yy / 7.0), 0, 255), gray,
                    np.clip(gray + 40 * np.sin(xx / 9.0), 0, 255)], -1).astype(np.uint8)
    det = rva.GpuDetector(W, H)
    ndet = len(det.detect(bgr, rva.AT_FMT_BGR8))
    arr, n = det._records_array(0)
    raw = torch.empty(W * H * 3, dtype=torch.uint8).pin_memory()
    cap = rva.jpeg_max_bytes(W, H, "4:2:0")
    jbuf = torch.empty(cap, dtype=torch.uint8).pin_memory()
    jlen = C.c_size_t()
    nn = C.c_int()

    def detect():
        rc = L.at_detect(det._h, bgr.ctypes.data, rva.AT_FMT_BGR8, det._out, det._cap, C.byref(nn))
        assert rc == 0, rc

    def leg_raw():
        rc = L.at_annotate_staged(det._h, 0, arr, n, raw.data_ptr())
        assert rc == 0, rc

    def leg_jpeg():
        rc = L.at_annotate_jpeg(det._h, 0, arr, n, quality, 0, jbuf.data_ptr(), cap, C.byref(jlen))
        assert rc == 0, rc

    # the stream is the host encoder's of the raw annotated image
    detect()
    leg_raw()
    annotated = raw.numpy().reshape(H, W, 3).copy()
    detect()
    leg_jpeg()
    stream = bytes(jbuf.numpy()[:jlen.value])
    equal = stream == rva.jpeg_encode_host(annotated, quality, "4:2:0")
    t = {"raw": [], "jpeg": []}
    for it in range(-20, iters):   # 20 warm-up rounds
        for name, leg in (("raw", leg_raw), ("jpeg", leg_jpeg)):
            detect()
            t0 = time.perf_counter()
            leg()
            t1 = time.perf_counter()
            if it >= 0:
                t[name].append((t1 - t0) * 1e3)
    det.set_profiling(True)
    ns = []
    for _ in range(12):
        detect()
        leg_jpeg()
        ns.append(det.jpeg_stats()["encode_kernels_ns"])
    det.set_profiling(False)
    ns = sorted(ns[2:])
    rgb = np.ascontiguousarray(annotated[:, :, ::-1])
    pil = []
    for _ in range(12):
        b = io.BytesIO()
        t0 = time.perf_counter()
        Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=2)
        pil.append((time.perf_counter() - t0) * 1e3)
    pil = sorted(pil[2:])
    det.close()
    return {
        "width": W, "height": H, "detections": ndet, "iterations": iters,
        "stream_equals_host_encoder": bool(equal),
        "annotate_staged_ms": {"p50": round(pct(t["raw"], 0.5), 4), "p99": round(pct(t["raw"], 0.99), 4)},
        "annotate_jpeg_ms": {"p50": round(pct(t["jpeg"], 0.5), 4), "p99": round(pct(t["jpeg"], 0.99), 4)},
        "link_bytes_per_frame": {"raw": W * H * 3, "jpeg": jlen.value},
        "encode_kernels_ms": {"median": round(ns[len(ns) // 2] / 1e6, 4), "min": round(ns[0] / 1e6, 4),
                              "how": "hipEventElapsedTime around the six encode launches (k_jpg_fdct .. k_jpg_pack), 10 calls"},
        "pillow_encode_ms_one_thread": {"median": round(pil[len(pil) // 2], 3), "min": round(pil[0], 3),
                                        "bytes": len(b.getvalue())},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_out_bench.json"))
    args = ap.parse_args()
    import torch

    import ros_vision_amd as rva
    res = {"device": torch.cuda.get_device_name(0), "quality": args.quality, "sampling": "4:2:0",
           "how": "per call: host clock around at_annotate_staged / at_annotate_jpeg (each ends in a stream "
                  "synchronise), the two alternating, one at_detect of the BGR8 frame before each (not timed)",
           "sizes": [measure(rva, w, h, args.iters, args.quality) for w, h in ((1920, 1080), (1280, 720))]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
