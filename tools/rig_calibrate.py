#!/usr/bin/env python3
"""Calibrate the cameras' extrinsics from a directory of synchronised frames.

The frames are named <prefix>_<frame>_<camid>.png: frame <frame> of camera <camid>, all cameras of
one <frame> taken at one instant.  Per camera the intrinsics come from
<calibration_dir>/calibrationmatrix_<camid>.json and the initial extrinsics from the system config
(camera_mounted_positions.<camid> -> extrinsics.<location>), the tags' field poses from a layout
file (this project's format or a WPILib field layout).  One GpuDetector per camera detects every
frame, a RigCalibrator collects the instants and solves on the GPU.  The first camera (or --fixed)
is held fixed: the robot frame is defined by its mount.

Prints each camera's "extrinsics" entry as JSON and the RMS before and after; --write saves the
entries into the system config (the rest of the file stays as it was)."""
import argparse
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_RE = re.compile(r"^(?P<prefix>.+)_(?P<frame>\d+)_(?P<cam>[^_]+)\.png$")


def read_gray(path):
    """A PNG as gray uint8 [H, W]."""
    try:
        import cv2
        img = cv2.imread(path, cv2.IMREAD_GRAYSCALE)
        if img is None:
            raise OSError("cannot read %s" % path)
        return np.ascontiguousarray(img)
    except ImportError:
        from PIL import Image
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("L"), np.uint8))


def group_frames(directory, prefix=None):
    """{frame number: {camid: path}} of the directory's <prefix>_<frame>_<camid>.png files."""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.png"))):
        m = FRAME_RE.match(os.path.basename(path))
        if not m or (prefix is not None and m.group("prefix") != prefix):
            continue
        out.setdefault(int(m.group("frame")), {})[m.group("cam")] = path
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("frames", help="directory of <prefix>_<frame>_<camid>.png")
    ap.add_argument("--calibration-dir", required=True)
    ap.add_argument("--system-config", required=True)
    ap.add_argument("--layout", required=True)
    ap.add_argument("--prefix", default=None, help="use only the frames of this prefix")
    ap.add_argument("--cameras", nargs="*", default=None, help="camera ids, in order (default: all found, sorted)")
    ap.add_argument("--fixed", default=None, help="the camera held fixed (default: the first)")
    ap.add_argument("--rotation-only", nargs="*", default=[], help="cameras whose translation is held fixed")
    ap.add_argument("--translation-only", nargs="*", default=[], help="cameras whose rotation is held fixed")
    ap.add_argument("--max-hamming", type=int, default=0)
    ap.add_argument("--tag-size", type=float, default=None)
    ap.add_argument("--host", action="store_true", help="solve on the CPU twin instead of the GPU")
    ap.add_argument("--undistort", action="store_true",
                    help="calibrate from ideal corners: each camera's lens distortion undone on the GPU")
    ap.add_argument("--write", action="store_true", help="save the entries into the system config")
    args = ap.parse_args(argv)

    import ros_vision_amd as rva
    from ros_vision_amd import node

    groups = group_frames(args.frames, args.prefix)
    if not groups:
        ap.error("no <prefix>_<frame>_<camid>.png in %s" % args.frames)
    cam_ids = args.cameras or sorted({c for g in groups.values() for c in g})
    if len(cam_ids) < 2:
        ap.error("a calibration needs two cameras or more")
    fixed = args.fixed or cam_ids[0]
    if fixed not in cam_ids:
        ap.error("--fixed names no camera")
    tag_size = rva.TAG_SIZE if args.tag_size is None else args.tag_size
    layout = node.load_field_layout(args.layout)

    cams, locations, dets = [], [], {}
    for cid in cam_ids:
        cm, dist = node.load_camera_calibration(args.calibration_dir, cid)
        R, t, location = node.load_extrinsics(args.system_config, cid)
        if location is None:
            ap.error("camera %s has no location in %s" % (cid, args.system_config))
        locations.append(location)
        cams.append((cm, (R, t), cid != fixed and cid not in args.translation_only,
                     cid != fixed and cid not in args.rotation_only))
        dets[cid] = (cm, dist)
    cal = rva.RigCalibrator(cams, layout, max_hamming=args.max_hamming, tag_size=tag_size)

    detectors = {}
    stored = 0
    for frame in sorted(groups):
        per = []
        for cid in cam_ids:
            path = groups[frame].get(cid)
            if path is None:
                per.append(None)
                continue
            img = read_gray(path)
            if cid not in detectors:
                cm, dist = dets[cid]
                detectors[cid] = rva.GpuDetector(img.shape[1], img.shape[0], cm, dist, max_batch=1, tag_size=tag_size)
                if args.undistort:
                    detectors[cid].set_undistort(True)
            d = detectors[cid]
            d.detect(img, rva.AT_FMT_GRAY8)
            per.append((d.ideal_detections(0) if args.undistort else d.detections(0), d.poses(0)))
        stored += bool(cal.add(per))
    print("%d of %d instants stored (two cameras or more with a layout tag)" % (stored, len(groups)), file=sys.stderr)
    if not stored:
        return 1
    res = cal.solve_host() if args.host else cal.solve()
    entries = {loc: {"rotation": [[float(x) for x in row] for row in R], "offset": [float(x) for x in t]}
               for loc, R, t in zip(locations, res.R, res.t)}
    print(json.dumps({"extrinsics": entries, "rms_px_before": res.rms_before, "rms_px_after": res.rms_after,
                      "instants_used": res.instants_used, "instants_skipped": res.instants_skipped,
                      "accepted_steps": res.accepted, "rejected_steps": res.rejected,
                      "sigma": {loc: [float(x) for x in np.sqrt(np.diag(c))] for loc, c in zip(locations, res.cov)}
                      if res.cov_valid else None}, indent=2))
    if args.write:
        for loc, R, t in zip(locations, res.R, res.t):
            node.save_extrinsics(args.system_config, loc, R, t)
    for d in detectors.values():
        d.close()
    cal.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
