#!/usr/bin/env python3
"""What the annotated image costs a consumer, full size against the preview stream, measured
in one process on one GPU.

Per shape (1920x1080 and 1280x800) one synthetic board, tinted, is staged as a host BGR8
frame (at_detect); then five legs run over that staged frame, alternated, `--repeats` times,
each leg `--calls` calls after a warm-up, timed with the host clock around the synchronous
call (every call ends in a stream synchronise):

  full_q95        at_annotate_jpeg, quality 95, 4:2:0, full size -- the only GPU route there
                  was before the preview
  preview_q50     at_preview_jpeg, s = 4, quality 50, no budget
  preview_budget  at_preview_jpeg, s = 4, quality 50, max_bytes = 20000 (with the number of
                  encodes the search took)
  preview_tight   the same with max_bytes = 6000, a budget quality 50 misses at these shapes: what
                  the search costs when it runs
  host_shrink     the host alternative: at_annotate_staged's full image copied out, a numpy
                  box reduce by 4, Pillow's JPEG encode at quality 50

ms per call (median of the repeats' means, and their spread) and bytes per frame.  Then, in a
run of its own with at_set_profiling on, the kernels' time from at_preview_stats[5] for the
two preview legs (k_preview + drawing + the encodes), and for a YUYV and a GRAY8 frame of
the same shape.

Writes one JSON file (default profiles/preview_bench.json) and prints it.

  python tools/preview_bench.py [--calls 50] [--repeats 3] [--out profiles/preview_bench.json]
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

SHAPES = [(1920, 1080), (1280, 800)]
SCALE, BUDGET, TIGHT = 4, 20000, 6000


def tinted_board(w, h):
    from ros_vision_amd import synth
    gray = synth.render_board(w, h, seed=766, ntags=6)[0].astype(np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    bgr = np.stack([np.clip(gray - 35 * np.cos(yy / 7.0), 0, 255), gray, np.clip(gray + 40 * np.sin(xx / 9.0), 0, 255)], -1)
    return np.ascontiguousarray(bgr.astype(np.uint8))


def host_shrink(det, s, quality):
    from PIL import Image
    img = det.annotate_staged(0)
    h, w = img.shape[:2]
    pw, ph = (w // s) & ~7, (h // s) & ~7
    ox, oy = (w - pw * s) // 2, (h - ph * s) // 2
    box = img[oy:oy + ph * s, ox:ox + pw * s].reshape(ph, s, pw, s, 3).astype(np.uint16).sum((1, 3))
    small = ((box + s * s // 2) // (s * s)).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(small[:, :, ::-1]).save(b, "JPEG", quality=quality, subsampling=2)
    return b.getvalue()


def timed(fn, calls):
    for _ in range(3):
        out = fn()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preview_bench.json"))
    args = ap.parse_args()
    import torch
    import ros_vision_amd as rva
    if not torch.cuda.is_available():
        raise SystemExit("preview_bench needs the GPU: nothing is measured without it")
    result = {"gpu": torch.cuda.get_device_name(0), "calls_per_leg": args.calls, "repeats": args.repeats,
              "scale": SCALE, "budget_bytes": BUDGET, "tight_budget_bytes": TIGHT, "shapes": []}
    for w, h in SHAPES:
        det = rva.GpuDetector(w, h)
        bgr = tinted_board(w, h)
        ntags = len(det.detect(bgr, rva.AT_FMT_BGR8))
        legs = {
            "full_q95": lambda: det.annotate_jpeg(0, 95, "4:2:0"),
            "preview_q50": lambda: det.preview_jpeg(0, SCALE, quality=50)[0],
            "preview_budget": lambda: det.preview_jpeg(0, SCALE, quality=50, max_bytes=BUDGET)[0],
            "preview_tight": lambda: det.preview_jpeg(0, SCALE, quality=50, max_bytes=TIGHT)[0],
            "host_shrink": lambda: host_shrink(det, SCALE, 50),
        }
        ms = {k: [] for k in legs}
        nbytes, extra = {}, {}
        legs_with_search = ("preview_budget", "preview_tight")
        for _ in range(args.repeats):
            for name, fn in legs.items():          # alternated: every repeat visits every leg
                t, out = timed(fn, args.calls)
                ms[name].append(t)
                nbytes[name] = len(out)
                if name in legs_with_search:
                    st = det.preview_stats()
                    extra[name] = {"encodes": st["encodes"], "quality_used": st["quality_used"]}
        rec = {"width": w, "height": h, "preview": list(det.preview_size(SCALE)[:2]), "tags": ntags, "legs": {}}
        for name in legs:
            v = sorted(ms[name])
            rec["legs"][name] = {"ms_per_call": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4),
                                 "ms_max": round(v[-1], 4), "bytes": nbytes[name]}
        for name in legs_with_search:
            rec["legs"][name].update(extra[name])
        # kernel times: a run of its own, profiling on
        det.set_profiling(True)
        kern = {}
        frames = {"bgr8": (bgr, rva.AT_FMT_BGR8), "gray8": (np.ascontiguousarray(bgr[:, :, 1]), rva.AT_FMT_GRAY8)}
        yuyv = np.empty((h, 2 * w), np.uint8)
        yuyv[:, 0::2] = bgr[:, :, 1]
        yuyv[:, 1::2] = np.random.RandomState(1).randint(96, 160, (h, w))
        frames["yuyv"] = (yuyv, rva.AT_FMT_YUYV)
        for key, (frame, fmt) in frames.items():
            det.detect(frame, fmt)
            for label, kw in (("q50", {}), ("budget", {"max_bytes": BUDGET})):
                ns = []
                for _ in range(args.calls):
                    det.preview_jpeg(0, SCALE, quality=50, **kw)
                    ns.append(det.preview_stats()["kernels_ns"])
                kern["%s_%s_kernels_us" % (key, label)] = round(sorted(ns)[len(ns) // 2] / 1e3, 2)
            ns = []
            for _ in range(args.calls):
                det.preview_bgr(0, SCALE)
                ns.append(det.preview_stats()["kernels_ns"])
            kern["%s_preview_and_draw_us" % key] = round(sorted(ns)[len(ns) // 2] / 1e3, 2)
        det.set_profiling(False)
        rec["kernels"] = kern
        result["shapes"].append(rec)
        det.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
