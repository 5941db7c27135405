#!/usr/bin/env python3
"""Map a field's tags -- where each really stands -- from a directory of frames of one calibrated
camera.

A GpuDetector with the camera's calibrationmatrix_<serial>.json detects every frame and gives each
tag's own pose; a FieldMapper collects the views and solves on the GPU (--host: on the CPU twin,
which gives the same result bit for bit).  The tags to map are those of the nominal layout
(--layout: what node.load_field_layout reads), each started where the layout puts it, plus any
further ids given with --ids, which have no start and are placed from views that see them together
with placed tags.  --anchor names the tag or tags held fixed at the layout's pose (at least one):
they fix where the field frame is.  At most 32 tags.

Writes the refined layout as WPILib layout JSON (--out, node.save_field_layout) and prints per tag
its shift from the nominal pose, its standard deviations and the number of views that saw it."""
import argparse
import glob
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp")


def read_gray(path):
    """An image file as gray uint8 [H, W] (Pillow)."""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("L"), np.uint8))


def report(tags, nominal, cov_valid, out=sys.stdout):
    """One line per tag: shift from nominal (mm, degrees), sigma of the position (mm) and of the
    turn (degrees), views."""
    where = {g[0]: g for g in nominal}
    print("%4s %6s %10s %10s %10s %10s %6s" % ("id", "placed", "shift mm", "turn deg", "sigma mm", "sigma deg", "views"), file=out)
    for q in tags:
        if not q.placed:
            print("%4d %6s %10s %10s %10s %10s %6d" % (q.id, "no", "-", "-", "-", "-", q.views), file=out)
            continue
        ref = where.get(q.id, (q.id, q.R0, q.t0))          # (a tag without a nominal pose: against its start)
        shift = 1e3 * float(np.linalg.norm(q.t - np.asarray(ref[2])))
        c = (float(np.trace(np.asarray(ref[1]).T @ q.R)) - 1.0) / 2.0
        turn = math.degrees(math.acos(max(-1.0, min(1.0, c))))
        if cov_valid and q.cov.any():
            d = np.diag(q.cov)
            s_mm, s_deg = "%10.2f" % (1e3 * math.sqrt(d[3:].sum())), "%10.3f" % math.degrees(math.sqrt(d[:3].sum()))
        else:
            s_mm, s_deg = "%10s" % ("held" if not q.cov.any() and cov_valid else "?"), "%10s" % ""
        print("%4d %6s %10.2f %10.3f %s %s %6d" % (q.id, "yes", shift, turn, s_mm, s_deg, q.views), file=out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("frames", help="directory of image files, one view each")
    ap.add_argument("--calibration", required=True, help="calibrationmatrix_<serial>.json of the camera")
    ap.add_argument("--layout", help="nominal layout file: the tags' starts")
    ap.add_argument("--ids", type=int, nargs="*", default=[], help="further tag ids to map, without a start")
    ap.add_argument("--anchor", type=int, nargs="+", required=True, help="id(s) held fixed at the layout's pose")
    ap.add_argument("--tag-size", type=float, default=None)
    ap.add_argument("--family", default="tag36h11")
    ap.add_argument("--max-hamming", type=int, default=0)
    ap.add_argument("--host", action="store_true", help="solve on the CPU twin")
    ap.add_argument("--undistort", action="store_true",
                    help="map from ideal corners: the calibration's lens distortion undone on the GPU")
    ap.add_argument("--out", default="field_layout_refined.json")
    args = ap.parse_args(argv)

    import ros_vision_amd as rva
    from ros_vision_amd import node

    nominal = node.load_field_layout(args.layout) if args.layout else []
    known = {g[0] for g in nominal}
    if not set(args.anchor) <= known:
        ap.error("--anchor: every anchor needs a pose in --layout")
    tags = [(tid, R, t, tid not in args.anchor, tid not in args.anchor) for tid, R, t in nominal]
    tags += [(tid, None, None, True, True) for tid in args.ids if tid not in known]
    tag_size = rva.TAG_SIZE if args.tag_size is None else args.tag_size
    d, s = os.path.split(os.path.abspath(args.calibration))
    cam, dist = node.load_camera_calibration(d, s[len("calibrationmatrix_"):-len(".json")])

    paths = sorted(p for p in glob.glob(os.path.join(args.frames, "*")) if p.lower().endswith(EXTENSIONS))
    if not paths:
        ap.error("no image file in %s" % args.frames)
    mapper = rva.FieldMapper(tags, max_hamming=args.max_hamming, tag_size=tag_size)
    det, size, stored = None, None, 0
    for path in paths:
        img = read_gray(path)
        if det is None:
            size = (img.shape[1], img.shape[0])
            det = rva.GpuDetector(img.shape[1], img.shape[0], cam, dist, family=args.family, max_batch=1, tag_size=tag_size)
            if args.undistort:
                det.set_undistort(True)
        elif (img.shape[1], img.shape[0]) != size:
            raise SystemExit("%s is not %d x %d" % (path, size[0], size[1]))
        det.detect(img, rva.AT_FMT_GRAY8)
        stored += bool(mapper.add(det.ideal_detections(0) if args.undistort else det.detections(0), det.poses(0), cam))
    det.close()
    print("%d of %d frames stored (two map tags or more in the frame)" % (stored, len(paths)), file=sys.stderr)
    if not stored:
        return 1
    res = mapper.solve_host() if args.host else mapper.solve()
    print("rms %.4f -> %.4f px over %d corners of %d views (%d skipped); %d of %d tags placed; %d steps accepted, "
          "%d rejected" % (res.rms_before, res.rms_after, res.corners, res.views_used, res.views_skipped, res.n_placed,
                           res.n_tags, res.accepted, res.rejected))
    recs = mapper.tags()
    report(recs, nominal, res.cov_valid)
    path = node.save_field_layout(args.out, [(q.id, q.R, q.t) for q in recs if q.placed])
    print("wrote %s" % path, file=sys.stderr)
    mapper.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
