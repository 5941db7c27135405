#!/usr/bin/env python3
"""Calibrate one camera -- intrinsics and distortion -- from a directory of frames of a tag board.

The board is a layout file (--board: what node.load_field_layout reads, each tag's pose in the
board frame) or a printed grid (--grid ROWS COLS FIRST_ID TAG_SIZE PITCH, node.grid_board).  A
GpuDetector with zero distortion detects every frame (so the corners are raw pixels), a
CameraCalibrator collects the views and solves on the GPU; without one (or with --host) the solve
runs on the CPU twin, which gives the same result bit for bit.  Detections can be kept
(--save-detections) and used again without the frames or a GPU (--detections).

Prints the RMS before and after and every parameter with its standard deviation; --serial S writes
<calibration-dir>/calibrationmatrix_S.json, the file the detector node reads."""
import argparse
import glob
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp")


def read_gray(path):
    """An image file as gray uint8 [H, W] (Pillow)."""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("L"), np.uint8))


def detect_frames(rva, paths, family):
    """Per frame the detections of a zero-distortion detector, and the frame size."""
    zero = rva.DistCoeffs(0.0, 0.0, 0.0, 0.0, 0.0)
    det, size, out = None, None, []
    for path in paths:
        img = read_gray(path)
        if det is None:
            size = (img.shape[1], img.shape[0])
            det = rva.GpuDetector(size[0], size[1], rva.TEST_CAMERA, zero, family=family, max_batch=1)
        elif (img.shape[1], img.shape[0]) != size:
            raise SystemExit("%s is not %d x %d" % (path, size[0], size[1]))
        det.detect(img, rva.AT_FMT_GRAY8)
        out.append(list(det.detections(0)))
    if det is not None:
        det.close()
    return out, size


def to_json(views, size):
    return {"width": size[0], "height": size[1],
            "views": [[{"id": d.id, "hamming": d.hamming, "decision_margin": float(d.decision_margin),
                        "H": np.asarray(d.H).reshape(9).tolist(), "c": np.asarray(d.c).tolist(),
                        "p": np.asarray(d.p).reshape(8).tolist()} for d in v] for v in views]}


def from_json(data):
    views = [[SimpleNamespace(id=d["id"], hamming=d["hamming"], decision_margin=d["decision_margin"],
                              H=np.array(d["H"]).reshape(3, 3), c=np.array(d["c"]), p=np.array(d["p"]).reshape(4, 2))
              for d in v] for v in data["views"]]
    return views, (int(data["width"]), int(data["height"]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("frames", nargs="?", help="directory of image files, one view each")
    ap.add_argument("--detections", help="a file written by --save-detections, instead of frames")
    ap.add_argument("--save-detections", help="write the frames' detections here")
    ap.add_argument("--board", help="layout file of the board's tags (board frame)")
    ap.add_argument("--grid", nargs=5, metavar=("ROWS", "COLS", "ID0", "SIZE", "PITCH"),
                    help="a printed grid: rows, columns, first id, tag size, centre-to-centre pitch")
    ap.add_argument("--tag-size", type=float, default=None, help="with --board: the tags' size")
    ap.add_argument("--family", default="tag36h11")
    ap.add_argument("--free", default="fx,fy,cx,cy,k1,k2,p1,p2,k3", help="comma-separated parameters to solve for")
    ap.add_argument("--init", help="calibrationmatrix_<serial>.json to start from (default: guessed)")
    ap.add_argument("--max-hamming", type=int, default=0)
    ap.add_argument("--host", action="store_true", help="solve on the CPU twin")
    ap.add_argument("--calibration-dir", default=".")
    ap.add_argument("--serial", help="write calibrationmatrix_<serial>.json into --calibration-dir")
    args = ap.parse_args(argv)

    import ros_vision_amd as rva
    from ros_vision_amd import node

    if (args.board is None) == (args.grid is None):
        ap.error("give --board FILE or --grid ROWS COLS ID0 SIZE PITCH")
    if args.grid:
        rows, cols, id0 = (int(v) for v in args.grid[:3])
        tag_size, pitch = float(args.grid[3]), float(args.grid[4])
        board = node.grid_board(rows, cols, id0, tag_size, pitch)
    else:
        board = node.load_field_layout(args.board)
        tag_size = rva.TAG_SIZE if args.tag_size is None else args.tag_size
    free = 0
    for name in filter(None, args.free.split(",")):
        if name not in rva.CAMCAL_PARAMS:
            ap.error("--free: unknown parameter %s" % name)
        free |= 1 << rva.CAMCAL_PARAMS.index(name)

    if args.detections:
        with open(args.detections) as f:
            views, size = from_json(json.load(f))
    elif args.frames:
        paths = sorted(p for p in glob.glob(os.path.join(args.frames, "*")) if p.lower().endswith(EXTENSIONS))
        if not paths:
            ap.error("no image file in %s" % args.frames)
        views, size = detect_frames(rva, paths, args.family)
    else:
        ap.error("give a directory of frames or --detections FILE")
    if args.save_detections:
        with open(args.save_detections, "w") as f:
            json.dump(to_json(views, size), f)

    init = None
    if args.init:
        d, s = os.path.split(os.path.abspath(args.init))
        init = node.load_camera_calibration(d, s[len("calibrationmatrix_"):-len(".json")])
    cal = rva.CameraCalibrator(size[0], size[1], board, tag_size, free=free, init=init, max_hamming=args.max_hamming)
    stored = sum(bool(cal.add(v)) for v in views)
    print("%d of %d frames stored (a board tag in the frame)" % (stored, len(views)), file=sys.stderr)
    if not stored:
        return 1
    use_host = args.host
    if not use_host:
        try:
            import torch
            use_host = not torch.cuda.is_available()
        except ImportError:
            pass
        if use_host:
            print("no GPU: solving on the CPU twin", file=sys.stderr)
    res = cal.solve_host() if use_host else cal.solve()
    sigma = np.sqrt(np.diag(res.cov)) if res.cov_valid else [None] * 9
    print("rms %.4f -> %.4f px over %d corners of %d views (%d skipped); %d steps accepted, %d rejected"
          % (res.rms_before, res.rms_after, res.corners, res.views_used, res.views_skipped, res.accepted, res.rejected))
    for k, name in enumerate(rva.CAMCAL_PARAMS):
        if not (free >> k) & 1:
            print("%-3s %14.8g   (held)" % (name, res.params[k]))
        elif sigma[k] is None:
            print("%-3s %14.8g   +- ?" % (name, res.params[k]))
        else:
            print("%-3s %14.8g   +- %.3g" % (name, res.params[k], sigma[k]))
    if args.serial:
        path = node.save_camera_calibration(args.calibration_dir, args.serial, res.camera_matrix,
                                            res.distortion_coefficients, res.rms_after,
                                            extra={"views": res.views_used, "image_size": list(size)})
        print("wrote %s" % path, file=sys.stderr)
    cal.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
