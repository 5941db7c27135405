"""Lenses, the numpy restatement and the warped scenes for the ideal-corner tests
(tests/test_undistort_host.py, tests/test_undistort_gpu.py).

The forward model (include/at_api.h, csrc/at_undist.h) takes a normalised ideal point (x, y) to
  x'' = x lin + 2 p1 x y + p2 (r2 + 2 x^2),  y'' = y lin + p1 (r2 + 2 y^2) + 2 p2 x y,
  lin = 1 + k1 r2 + k2 r2^2 + k3 r2^3,       u = fx x'' + cx,  v = fy y'' + cy;
the ideal pixel of a raw one is its inverse image, found by eight Newton steps from the raw
normalised point.  Everything here is written in the library's operation order, in float64
without contraction, so values and flags are the library's bit for bit.  Nothing here needs the
library or a GPU.
"""
import json
import os
from types import SimpleNamespace

import numpy as np

ITERS = 8
TOL_PX = 1e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def lens(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, width=640, height=480):
    return SimpleNamespace(fx=fx, fy=fy, cx=cx, cy=cy, k1=k1, k2=k2, p1=p1, p2=p2, k3=k3, width=width, height=height)


def load_lenses():
    """name -> lens of tests/golden/lenses.json (matrix and five coefficients of the deployed
    cameras' calibration files, each at 1280 x 800)."""
    with open(os.path.join(GOLDEN, "lenses.json")) as f:
        raw = json.load(f)
    out = {}
    for name, j in raw.items():
        m, d = j["matrix"], j["disto"][0]
        out[name] = lens(m[0][0], m[1][1], m[0][2], m[1][2], d[0], d[1], d[2], d[3], d[4], j["width"], j["height"])
    return out


# lenses whose Jacobian determinant stays >= 0.5 over their whole frame; cam14 (k3 = -0.395) folds over
REGULAR = ("12", "199", "766", "UC762", "cam11", "cam13", "cam15")

# the 640 x 480 scenes' camera (field_pose_cases.GPU_CAM) behind a barrel lens: the corner of the
# frame (r2 = 0.42) moves by 18 px, a tag half way out by 3-5 px; the determinant stays above 0.8
GPU_LENS = lens(620.0, 620.0, 320.0, 240.0, k1=-0.12, k2=0.03, p1=0.002, p2=-0.001, k3=0.0)
NO_LENS = lens(620.0, 620.0, 320.0, 240.0)
# ... and behind one that folds over inside the frame (k1 = 2, k3 = -40: r lin(r) peaks at r = 0.445,
# 276 px from the centre, where the raw radius is 299 px).  Raw pixels 276-299 px out have an
# inverse image, but the Newton iteration starts at the raw point, beyond the fold, where the
# determinant is negative: they are flagged; further out there is no inverse image at all.  The
# detector's own edge fit still works 288 px out (checked with the CPU oracle: fold_frame()).
FOLD_LENS = lens(620.0, 620.0, 320.0, 240.0, k1=2.0, k3=-40.0)


def fold_frame(draw_tag, square, codes, blank):
    """A raw frame for FOLD_LENS (drawn as the camera sees it, no warp): tag 2 near the centre, tag 1
    with its outer corner 288 px from it.  The oracle returns both; tag 1 is not invertible."""
    img = blank()
    draw_tag(img, codes[1], square(320 + 245 * 0.8, 240 + 245 * 0.6, 80, 5))
    draw_tag(img, codes[2], square(300, 230, 110, -8))
    return img


def crowd_frame(draw_tag, square, codes, blank):
    """18 tags (ids 20-37) of 84 px on a 6 x 3 grid, tag k turned by 7 k degrees, without
    distortion: more detections than the 16 a wave of k_pose<false> holds."""
    img = blank()
    for k in range(18):
        draw_tag(img, codes[20 + k], square(56 + 106 * (k % 6), 82 + 158 * (k // 6), 84, 7 * k))
    return img


def grid(ln, step=4):
    xs, ys = np.meshgrid(np.arange(0, ln.width, step, dtype=np.float64), np.arange(0, ln.height, step, dtype=np.float64))
    return np.stack([xs.ravel(), ys.ravel()], 1)


# ---- the algorithm, restated ------------------------------------------------------------------
def _forward(c, x, y):
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    r4 = r2 * r2
    r6 = r4 * r2
    lin = ((1.0 + c.k1 * r2) + c.k2 * r4) + c.k3 * r6
    dl = (c.k1 + 2.0 * c.k2 * r2) + 3.0 * c.k3 * r4
    xd = (x * lin + 2.0 * c.p1 * xy) + c.p2 * (r2 + 2.0 * xx)
    yd = (y * lin + c.p1 * (r2 + 2.0 * yy)) + 2.0 * c.p2 * xy
    j0 = ((lin + 2.0 * xx * dl) + 2.0 * c.p1 * y) + 6.0 * c.p2 * x
    j1 = (2.0 * xy * dl + 2.0 * c.p1 * x) + 2.0 * c.p2 * y
    j2 = ((lin + 2.0 * yy * dl) + 6.0 * c.p1 * y) + 2.0 * c.p2 * x
    return xd, yd, j0, j1, j2


def forward_pixels(c, xy):
    """Raw pixels of ideal pixels [n, 2]."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    xd, yd, *_ = _forward(c, (xy[:, 0] - c.cx) / c.fx, (xy[:, 1] - c.cy) / c.fy)
    return np.stack([xd * c.fx + c.cx, yd * c.fy + c.cy], 1)


def min_determinant(c, xy):
    """The least Jacobian determinant over the ideal pixels xy."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    _xd, _yd, j0, j1, j2 = _forward(c, (xy[:, 0] - c.cx) / c.fx, (xy[:, 1] - c.cy) / c.fy)
    return float((j0 * j2 - j1 * j1).min())


def und_points_ref(c, xy):
    """([n, 2] ideal pixels, [n] bool ok) of raw pixels [n, 2]: und_point, vectorised."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    u, v = xy[:, 0].copy(), xy[:, 1].copy()
    with np.errstate(all="ignore"):
        x0, y0 = (u - c.cx) / c.fx, (v - c.cy) / c.fy
        x, y = x0.copy(), y0.copy()
        ok = np.ones(len(u), bool)
        for _ in range(ITERS):
            xd, yd, j0, j1, j2 = _forward(c, x, y)
            det = j0 * j2 - j1 * j1
            ok &= det > 0.0
            rx, ry = xd - x0, yd - y0
            x, y = x - (j2 * rx - j1 * ry) / det, y - (j0 * ry - j1 * rx) / det
        xd, yd, j0, j1, j2 = _forward(c, x, y)
        det = j0 * j2 - j1 * j1
        ok &= det > 0.0
        eu, ev = (xd * c.fx + c.cx) - u, (yd * c.fy + c.cy) - v
        ok &= (eu <= TOL_PX) & (eu >= -TOL_PX) & (ev <= TOL_PX) & (ev >= -TOL_PX)
        ou = np.where(ok, u + c.fx * (x - x0), u)
        ov = np.where(ok, v + c.fy * (y - y0), v)
    return np.stack([ou, ov], 1), ok


CORNER_T = ((-1.0, 1.0), (1.0, 1.0), (1.0, -1.0), (-1.0, -1.0))   # at_detection.p[i] = H (tx, ty)


def homography_ref(p):
    """H [9] with H (tx, ty)_i = p[i] by homography_compute2's elimination, or None (singular)."""
    A = []
    for (tx, ty), (px, py) in zip(CORNER_T, [(float(a), float(b)) for a, b in np.asarray(p, np.float64)]):
        A.append([tx, ty, 1.0, 0.0, 0.0, 0.0, -tx * px, -ty * px, px])
        A.append([0.0, 0.0, 0.0, tx, ty, 1.0, -tx * py, -ty * py, py])
    for col in range(8):
        max_val, max_idx = 0.0, -1
        for row in range(col, 8):
            v = abs(A[row][col])
            if v > max_val:
                max_val, max_idx = v, row
        if not max_val >= 1e-10:
            return None
        if max_idx != col:   # (the entries left of col are never read again: whole rows may swap)
            A[col], A[max_idx] = A[max_idx], A[col]
        for i in range(col + 1, 8):
            f = A[i][col] / A[col][col]
            for j in range(col + 1, 9):
                A[i][j] = A[i][j] - f * A[col][j]
    for col in range(7, -1, -1):
        s = 0.0
        for i in range(col + 1, 8):
            s = s + A[col][i] * A[i][8]
        A[col][8] = (A[col][8] - s) / A[col][col]
    return np.array([A[k][8] for k in range(8)] + [1.0])


def ideal_detection_ref(c, d):
    """The ideal record of detection d (id, hamming, decision_margin, H [3, 3], c, p): und_detection."""
    H, cc, p, tid = np.asarray(d.H, np.float64).reshape(9), np.asarray(d.c, np.float64), np.asarray(d.p, np.float64), d.id
    if any((c.k1, c.k2, c.p1, c.p2, c.k3)):
        q, ok = und_points_ref(c, p)
        Hi = homography_ref(q) if ok.all() else None
        if Hi is None:
            tid = -1
        else:
            H, cc, p = Hi, np.array([Hi[2] / Hi[8], Hi[5] / Hi[8]]), q
    return SimpleNamespace(id=int(tid), hamming=d.hamming, decision_margin=d.decision_margin, H=H.reshape(3, 3).copy(),
                           c=cc.copy(), p=p.copy())


def same_detection(a, b):
    """Bit for bit."""
    return (a.id == b.id and a.hamming == b.hamming
            and np.float32(a.decision_margin).tobytes() == np.float32(b.decision_margin).tobytes()
            and np.asarray(a.H, np.float64).tobytes() == np.asarray(b.H, np.float64).tobytes()
            and np.asarray(a.c, np.float64).tobytes() == np.asarray(b.c, np.float64).tobytes()
            and np.asarray(a.p, np.float64).tobytes() == np.asarray(b.p, np.float64).tobytes())


# ---- frames seen through a lens ---------------------------------------------------------------
def warp(img, c):
    """The frame a camera with lens c gives of the scene whose distortion-free picture is img
    (uint8 [h, w], pixel centres at +0.5): every raw pixel takes the bilinear sample of img at its
    ideal pixel (the restatement above); pixels without one, or whose ideal pixel lies outside img,
    take the nearest pixel of img."""
    h, w = img.shape
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64) + 0.5, np.arange(h, dtype=np.float64) + 0.5)
    q, _ok = und_points_ref(c, np.stack([xs.ravel(), ys.ravel()], 1))
    fx = np.clip(q[:, 0] - 0.5, 0.0, w - 1.0)
    fy = np.clip(q[:, 1] - 0.5, 0.0, h - 1.0)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = fx - x0, fy - y0
    f = img.astype(np.float64)
    val = (f[y0, x0] * (1 - ax) + f[y0, x1] * ax) * (1 - ay) + (f[y1, x0] * (1 - ax) + f[y1, x1] * ax) * ay
    return np.clip(np.rint(val), 0, 255).astype(np.uint8).reshape(h, w)


def camera_of(rva, c):
    """(CameraMatrix, DistCoeffs) of a lens, for GpuDetector."""
    return (rva.CameraMatrix(fx=c.fx, cx=c.cx, fy=c.fy, cy=c.cy),
            rva.DistCoeffs(k1=c.k1, k2=c.k2, p1=c.p1, p2=c.p2, k3=c.k3))
