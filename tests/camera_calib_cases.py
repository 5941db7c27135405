"""Scenes and the numpy restatement for the camera-calibration tests
(tests/test_camera_calib_host.py, tests/test_camera_calib_gpu.py).

A camera is the nine values (fx, fy, cx, cy, k1, k2, p1, p2, k3); a board the (id, R, t) triples of
node.grid_board; a view the list of one frame's detections (exact distorted corners, the exact
four-point homography of those corners).  tests/golden/camera_calib_cam13.json holds the matrix,
distortion and the 20 board poses of a real calibration: a real lens with all five coefficients
non-zero.  Nothing here needs the library or a GPU.
"""
import json
import math
import os
from types import SimpleNamespace

import numpy as np

import field_pose_cases as fc
import rig_calib_cases as rcc

ITERS = 30
CHUNK = 32
MAX_VIEWS = 4096
NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
FX, FY, CX, CY, K1, K2, P1, P2, K3 = (1 << i for i in range(9))
PINHOLE, ALL = 15, 511
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- scenes ---------------------------------------------------------------------------------------
def grid_board(rows, cols, first_id, tag_size, pitch):
    """node.grid_board, restated: tag (r, c) upright with its centre at (c pitch, r pitch, 0)."""
    return [(first_id + r * cols + c, np.eye(3), np.array([c * float(pitch), r * float(pitch), 0.0]))
            for r in range(rows) for c in range(cols)]


def rodrigues(v):
    v = np.asarray(v, np.float64).reshape(3)
    a = float(np.linalg.norm(v))
    if a == 0.0:
        return np.eye(3)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def distort(c, x, y):
    r2 = x * x + y * y
    lin = 1 + c[4] * r2 + c[5] * r2 ** 2 + c[8] * r2 ** 3
    return (x * lin + 2 * c[6] * x * y + c[7] * (r2 + 2 * x * x), y * lin + c[6] * (r2 + 2 * y * y) + 2 * c[7] * x * y)


def project(c, R, t, X):
    """Pixels [n, 2] of the board points X under the full forward model, and their depth."""
    P = np.asarray(X) @ np.asarray(R).T + np.asarray(t)
    xd, yd = distort(c, P[:, 0] / P[:, 2], P[:, 1] / P[:, 2])
    return np.stack([c[0] * xd + c[2], c[1] * yd + c[3]], 1), P[:, 2]


def homographies(px):
    """[n, 3, 3]: per tag the map of its (-1, 1), (1, 1), (1, -1), (-1, -1) onto its four corners px [n, 4, 2]."""
    px = np.asarray(px, np.float64).reshape(-1, 4, 2)
    A, b = np.zeros((len(px), 8, 8)), np.zeros((len(px), 8))
    for k, (x, y) in enumerate(fc.CORNER_SIGNS):
        u, v = px[:, k, 0], px[:, k, 1]
        A[:, 2 * k, :3] = A[:, 2 * k + 1, 3:6] = (x, y, 1)
        A[:, 2 * k, 6], A[:, 2 * k, 7] = -u * x, -u * y
        A[:, 2 * k + 1, 6], A[:, 2 * k + 1, 7] = -v * x, -v * y
        b[:, 2 * k], b[:, 2 * k + 1] = u, v
    h = np.linalg.solve(A, b[:, :, None])[:, :, 0]
    return np.concatenate([h, np.ones((len(px), 1))], 1).reshape(-1, 3, 3)


def homography(px):
    return homographies([px])[0]


def make_view(board, cam, R, t, tag_size, width, height, rng=None, noise_px=0.0, ids=None, clip=True):
    """The detections of the board tags (all, or `ids`) whose four corners lie inside the frame
    (clip) seen from x_cam = R x_board + t, in id order."""
    kept = []
    for tid, Rt, tt in sorted(board, key=lambda g: g[0]):
        if ids is not None and tid not in ids:
            continue
        px, z = project(cam, R, t, fc.tag_corners_field(Rt, tt, tag_size))
        if clip and not ((z > 0).all() and px.min() >= 0 and (px[:, 0] <= width - 1).all()
                         and (px[:, 1] <= height - 1).all()):
            continue
        if noise_px:
            px = px + rng.normal(scale=noise_px, size=px.shape)
        kept.append((int(tid), px))
    Hs = homographies([px for _tid, px in kept]) if kept else []
    return [SimpleNamespace(id=tid, hamming=0, decision_margin=60.0, H=H, c=px.mean(0), p=px)
            for (tid, px), H in zip(kept, Hs)]


def renoise(views, rng, noise_px):
    """views (exact) with fresh corner noise, the homographies those of the noisy corners."""
    out = []
    for dets in views:
        px = [d.p + rng.normal(scale=noise_px, size=d.p.shape) for d in dets]
        out.append([SimpleNamespace(id=d.id, hamming=0, decision_margin=60.0, H=H, c=q.mean(0), p=q)
                    for d, q, H in zip(dets, px, homographies(px))])
    return out


def cam13():
    """(true camera [9], [(R, t)] x 20) of the fixture."""
    with open(os.path.join(HERE, "golden", "camera_calib_cam13.json")) as f:
        d = json.load(f)
    m, k = d["matrix"], d["disto"][0]
    cam = np.array([m[0][0], m[1][1], m[0][2], m[1][2]] + list(k), np.float64)
    poses = [(rodrigues(np.array(r).reshape(3)), np.array(t, np.float64).reshape(3))
             for r, t in zip(d["rotvec"], d["travec"])]
    return cam, poses


# the cam13 case: a 1280 x 800 frame and a 4 x 4 grid of 3-unit tags 4 units apart, in the units of
# the file's translations (the boards stand 28 .. 51 units away: a tag is 50 .. 100 px across)
CAM13_SIZE = (1280, 800)
CAM13_TAG, CAM13_PITCH = 3.0, 4.0
CAM13_BOARD = grid_board(4, 4, 0, CAM13_TAG, CAM13_PITCH)


def cam13_case(rng=None, noise_px=0.0, n_views=None, ids=None):
    """(true camera, board, tag_size, views) -- every view keeps at least 4 whole tags in the frame
    when all ids are drawn."""
    cam, poses = cam13()
    views = []
    for R, t in poses[:n_views]:
        whole = make_view(CAM13_BOARD, cam, R, t, CAM13_TAG, *CAM13_SIZE)
        assert len(whole) >= 4, len(whole)
        views.append(make_view(CAM13_BOARD, cam, R, t, CAM13_TAG, *CAM13_SIZE, rng=rng, noise_px=noise_px, ids=ids))
    return cam, CAM13_BOARD, CAM13_TAG, views


def off_start(cam):
    """The start of the exact-corner checks: fx, fy 15 % off, cx, cy 20 px off, no distortion."""
    return np.array([cam[0] * 1.15, cam[1] * 0.85, cam[2] + 20.0, cam[3] - 20.0, 0, 0, 0, 0, 0], np.float64)


def many_views(n, rng, noise_px=0.0, ids=None):
    """n views of the cam13 board: the file's poses in turn, each turned and moved a little."""
    cam, poses = cam13()
    views = []
    for i in range(n):
        R, t = poses[i % len(poses)]
        R = fc.small_rotation(rng, 2.0) @ R
        t = t + rng.uniform(-0.5, 0.5, 3)
        views.append(make_view(CAM13_BOARD, cam, R, t, CAM13_TAG, *CAM13_SIZE, rng=rng, noise_px=noise_px, ids=ids))
    return cam, views


def behind_view(board, cam, tag_size, ids=(0, 3)):
    """A view with corners built behind the camera: the board is turned 80 degrees about y and
    stands astride the camera's plane, tag ids[0] in front of it and tag ids[1] behind, both put
    through the pinhole formula.  Under the pose of either tag's homography the other tag has its
    corners at Pz <= 0 (the pose of the tag behind comes out mirrored, P -> -P), so no candidate
    puts every corner in front and the view is skipped."""
    R, t = fc.rot_y(80.0), np.array([0.0, -2.0, 3.0])
    pin = np.array([cam[0], cam[1], cam[2], cam[3], 0, 0, 0, 0, 0], np.float64)
    dets = make_view(board, pin, R, t, tag_size, 0, 0, ids=set(ids), clip=False)
    z = [float((fc.tag_corners_field(Rt, tt, tag_size) @ R.T + t)[:, 2].max()) for tid, Rt, tt in board if tid == ids[1]]
    assert len(dets) == 2 and z[0] < 0
    return dets


def calibrator(rva, views, board, tag_size, size=CAM13_SIZE, **kw):
    """A CameraCalibrator holding the views it stores."""
    cal = rva.CameraCalibrator(size[0], size[1], board, tag_size, **kw)
    for v in views:
        cal.add(v)
    return cal


# ---- the algorithm, restated ------------------------------------------------------------------------
# Expression order is csrc/at_camcal.h's.  A sum over a view's corners is the 64-slot tree; a product
# sum runs over ascending k; a sum over the views runs ascending within chunks of 32, then over the
# chunks in order.
_TRI9 = [(i, j) for i in range(9) for j in range(i, 9)]
_chunked = rcc._chunked


def _model(c, R, t, X):
    Q, P = fc._points_cam(R, t, X)
    Pz = P[:, 2]
    x, y = P[:, 0] / Pz, P[:, 1] / Pz
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    r4 = r2 * r2
    r6 = r4 * r2
    lin = ((1.0 + c[4] * r2) + c[5] * r4) + c[8] * r6
    xd = (x * lin + 2.0 * c[6] * xy) + c[7] * (r2 + 2.0 * xx)
    yd = (y * lin + c[6] * (r2 + 2.0 * yy)) + 2.0 * c[7] * xy
    return SimpleNamespace(Q=Q, Pz=Pz, x=x, y=y, xx=xx, yy=yy, xy=xy, r2=r2, r4=r4, r6=r6, lin=lin, xd=xd, yd=yd)


def view_cost(c, R, t, X, uv):
    with np.errstate(all="ignore"):
        m = _model(c, R, t, X)
        ru = (c[0] * m.xd + c[2]) - uv[:, 0]
        rv = (c[1] * m.yd + c[3]) - uv[:, 1]
        return fc._tree(np.where(m.Pz > 0.0, ru * ru + rv * rv, math.inf))


def rows(c, mask, R, t, X, uv):
    """(jp [n, 6] x 2, ji [n, 9] x 2, ru, rv): the residual rows of the points X for the pose
    (w, dt) and for the nine intrinsics; columns that are not free are 0."""
    m = _model(c, R, t, X)
    x, y, Q, Pz = m.x, m.y, m.Q, m.Pz
    ru = (c[0] * m.xd + c[2]) - uv[:, 0]
    rv = (c[1] * m.yd + c[3]) - uv[:, 1]
    dl = (c[4] + 2.0 * c[5] * m.r2) + 3.0 * c[8] * m.r4
    dxx = ((m.lin + 2.0 * m.xx * dl) + 2.0 * c[6] * y) + 6.0 * c[7] * x
    dxy = (2.0 * m.xy * dl + 2.0 * c[6] * x) + 2.0 * c[7] * y
    dyy = ((m.lin + 2.0 * m.yy * dl) + 6.0 * c[6] * y) + 2.0 * c[7] * x
    A0, A1 = c[0] * dxx / Pz, c[0] * dxy / Pz
    A2 = -(A0 * x + A1 * y)
    B0, B1 = c[1] * dxy / Pz, c[1] * dyy / Pz
    B2 = -(B0 * x + B1 * y)
    jpu = [A2 * Q[:, 1] - A1 * Q[:, 2], A0 * Q[:, 2] - A2 * Q[:, 0], A1 * Q[:, 0] - A0 * Q[:, 1], A0, A1, A2]
    jpv = [B2 * Q[:, 1] - B1 * Q[:, 2], B0 * Q[:, 2] - B2 * Q[:, 0], B1 * Q[:, 0] - B0 * Q[:, 1], B0, B1, B2]
    zero, one = np.zeros(len(X)), np.ones(len(X))
    iu = [m.xd, zero, one, zero, c[0] * (x * m.r2), c[0] * (x * m.r4), c[0] * (2.0 * m.xy),
          c[0] * (m.r2 + 2.0 * m.xx), c[0] * (x * m.r6)]
    iv = [zero, m.yd, zero, one, c[1] * (y * m.r2), c[1] * (y * m.r4), c[1] * (m.r2 + 2.0 * m.yy),
          c[1] * (2.0 * m.xy), c[1] * (y * m.r6)]
    jiu = [iu[p] if (mask >> p) & 1 else zero for p in range(9)]
    jiv = [iv[p] if (mask >> p) & 1 else zero for p in range(9)]
    return np.stack(jpu, 1), np.stack(jpv, 1), np.stack(jiu, 1), np.stack(jiv, 1), ru, rv


def _accum(c, mask, R, t, X, uv, lam):
    """The view's part of the reduced system [99] and what the back substitution needs."""
    jpu, jpv, jiu, jiv, ru, rv = rows(c, mask, R, t, X, uv)
    U = {(i, j): fc._tree(jpu[:, i] * jpu[:, j] + jpv[:, i] * jpv[:, j]) for i, j in fc._TRI}
    g = [fc._tree(jpu[:, i] * ru + jpv[:, i] * rv) for i in range(6)]
    V = {(i, j): fc._tree(jiu[:, i] * jiu[:, j] + jiv[:, i] * jiv[:, j]) for i, j in _TRI9}
    h = [fc._tree(jiu[:, i] * ru + jiv[:, i] * rv) for i in range(9)]
    W = [[fc._tree(jpu[:, k] * jiu[:, b] + jpv[:, k] * jiv[:, b]) for b in range(9)] for k in range(6)]
    cols = [rcc._s6(U, [-W[k][b] for k in range(6)], lam) for b in range(9)]
    Y = [[cols[b][k] for b in range(9)] for k in range(6)]
    y = rcc._s6(U, [-g[k] for k in range(6)], lam)
    part = np.zeros(99)
    for r in range(9):
        for s in range(r, 9):
            acc = W[0][r] * Y[0][s]
            for k in range(1, 6):
                acc = acc + W[k][r] * Y[k][s]
            part[r * 9 + s] = V[(r, s)] - acc
        acc = W[0][r] * y[0]
        for k in range(1, 6):
            acc = acc + W[k][r] * y[k]
        part[81 + r] = h[r] - acc
        part[90 + r] = V[(r, r)]
    return part, (U, g, W)


def _apply_step(R, t, d):
    h = [0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]
    n = math.sqrt(1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]))
    Rn = fc._mul(fc._quat_to_R(1.0 / n, h[0] / n, h[1] / n, h[2] / n), R)
    return Rn, np.array([t[k] + d[3 + k] for k in range(3)])


def h_pose(H, c, hs):
    """cam_T_tag of a tag's homography under (fx, fy, cx, cy) = c[:4]."""
    H = [float(v) for v in np.asarray(H, np.float64).reshape(9)]
    a = [[(H[k] - c[2] * H[6 + k]) / c[0], (H[3 + k] - c[3] * H[6 + k]) / c[1], H[6 + k]] for k in range(3)]
    n1 = math.sqrt((a[0][0] * a[0][0] + a[0][1] * a[0][1]) + a[0][2] * a[0][2])
    n2 = math.sqrt((a[1][0] * a[1][0] + a[1][1] * a[1][1]) + a[1][2] * a[1][2])
    s = math.sqrt(n1 * n2)
    if a[2][2] < 0.0:
        s = -s
    r1 = [a[0][k] / s for k in range(3)]
    r2 = [a[1][k] / s for k in range(3)]
    t = np.array([(a[2][k] / s) * hs for k in range(3)])
    r3 = [r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]]
    return np.array([[r1[k], r2[k], r3[k]] for k in range(3)]), t


def focal_guess(stored, width, height):
    """(fx, fy) by Zhang's constraints with the principal point at the frame's centre, over the
    stored tags in view then id order; None when there is no positive solution."""
    cx, cy = float(width) / 2.0, float(height) / 2.0
    n00 = n01 = n11 = b0 = b1 = 0.0
    for dets in stored:
        for d in dets:
            H = [float(v) for v in np.asarray(d.H, np.float64).reshape(9)]
            x1, y1, z1 = H[0] - cx * H[6], H[3] - cy * H[6], H[6]
            x2, y2, z2 = H[1] - cx * H[7], H[4] - cy * H[7], H[7]
            q = math.sqrt(math.sqrt(x1 * x1 + y1 * y1) * math.sqrt(x2 * x2 + y2 * y2))
            x1, y1, z1, x2, y2, z2 = x1 / q, y1 / q, z1 / q, x2 / q, y2 / q, z2 / q
            for r in ((x1 * x2, y1 * y2, -(z1 * z2)), (x1 * x1 - x2 * x2, y1 * y1 - y2 * y2, -(z1 * z1 - z2 * z2))):
                n00 = n00 + r[0] * r[0]
                n01 = n01 + r[0] * r[1]
                n11 = n11 + r[1] * r[1]
                b0 = b0 + r[0] * r[2]
                b1 = b1 + r[1] * r[2]
    det = n00 * n11 - n01 * n01
    with np.errstate(all="ignore"):
        a = float(np.float64(b0 * n11 - b1 * n01) / np.float64(det))
        b = float(np.float64(n00 * b1 - n01 * b0) / np.float64(det))
    if not (a > 0.0 and b > 0.0 and math.isfinite(a) and math.isfinite(b)):
        return None
    return 1.0 / math.sqrt(a), 1.0 / math.sqrt(b)


def stored_views(views, board, max_hamming=0):
    """What at_camcal_add keeps of each view (ascending ids, at most 16); views without a board tag
    are not stored."""
    lay = {int(g[0]) for g in board}
    out = []
    for dets in views:
        sel = fc.select_ref(dets, lay, max_hamming)
        if sel:
            out.append([dets[i] for i in sel])
    return out


def solve_ref(views, board, tag_size, width, height, free=ALL, init=None, max_hamming=0, iters=ITERS):
    """The calibration as include/at_api.h defines it.  Returns a namespace with at_camcal_result's
    fields (params for cam), the per-view records and, for the tests, cost and start (the start
    intrinsics); None when the focal guess fails."""
    lay = {int(tid): (np.asarray(R, np.float64), np.asarray(t, np.float64)) for tid, R, t in board}
    stored = stored_views(views, board, max_hamming)
    N = len(stored)
    if init is None:
        f = focal_guess(stored, width, height)
        if f is None:
            return None
        cam = [f[0], f[1], float(width) / 2.0, float(height) / 2.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    else:
        cam = [float(v) for v in init]
    start_cam = list(cam)
    free_l = [bool((free >> p) & 1) for p in range(9)]
    hs = tag_size / 2.0
    pts, poses, ntags = [], [], []
    for dets in stored:
        X, uv = [], []
        for d in dets:
            Rt, tt = lay[d.id]
            for k, (sx, sy) in enumerate(fc.CORNER_SIGNS):
                X.append([(Rt[r, 0] * (sx * hs) + Rt[r, 1] * (sy * hs)) + tt[r] for r in range(3)])
                uv.append(np.asarray(d.p, np.float64)[k])
        X, uv = np.array(X), np.array(uv)
        pts.append((X, uv))
        cost, best = math.inf, None
        for d in dets:
            Rt, tt = lay[d.id]
            Rc, tc = h_pose(d.H, cam, hs)
            Rj = fc._mul(Rc, Rt.T)
            rt = np.array([(Rj[r, 0] * tt[0] + Rj[r, 1] * tt[1]) + Rj[r, 2] * tt[2] for r in range(3)])
            tj = tc - rt
            cj = view_cost(cam, Rj, tj, X, uv)
            if cj < cost:
                cost, best = cj, (Rj, tj)
        if best is None:
            poses.append((np.zeros((3, 3)), np.zeros(3)))
            ntags.append(0)
        else:
            poses.append((fc._project_rotation(best[0]), best[1]))
            ntags.append(len(dets))
    used = [n > 0 for n in ntags]

    def costs(ps, c):
        return [view_cost(c, *ps[i], *pts[i]) if used[i] else 0.0 for i in range(N)]

    cost0 = cost = _chunked(costs(poses, cam))
    lam, accepted, rejected = 1e-3, 0, 0
    for _ in range(iters):
        acc = [_accum(cam, free, *poses[i], *pts[i], lam) if used[i] else (np.zeros(99), None) for i in range(N)]
        tot = _chunked([a[0] for a in acc])
        L, ok = rcc._reduced(tot, free_l, lam, True)
        x = rcc._subst(L, [-float(tot[81 + p]) if free_l[p] else 0.0 for p in range(9)])
        dc = [x[p] if ok and free_l[p] else 0.0 for p in range(9)]
        cam_n = [cam[p] + dc[p] if free_l[p] else cam[p] for p in range(9)]
        poses_n = list(poses)
        for i in range(N):
            if not used[i]:
                continue
            U, g, W = acc[i][1]
            r = []
            for k in range(6):
                a = g[k]
                for q in range(9):
                    a = a + W[k][q] * dc[q]
                r.append(a)
            d = fc._solve6(U, r, lam)
            if d is None or not ok:
                d = [0.0] * 6
            poses_n[i] = _apply_step(*poses[i], d)
        cn = _chunked(costs(poses_n, cam_n))
        if ok and cn < cost:
            cam, poses, cost, accepted = cam_n, poses_n, cn, accepted + 1
            lam = max(lam / 10.0, 1e-9)
        else:
            rejected += 1
            lam = lam * 10.0
    acc = [_accum(cam, free, *poses[i], *pts[i], 0.0)[0] if used[i] else np.zeros(99) for i in range(N)]
    tot = _chunked(acc)
    L, ok = rcc._reduced(tot, free_l, 0.0, False)
    corners, n_used = 4 * sum(ntags), sum(used)
    den = 2 * corners - 6 * n_used - sum(free_l)
    valid = ok and den > 0
    cov = np.zeros((9, 9))
    if valid:
        s2 = cost / float(den)
        for p in range(9):
            w = rcc._subst(L, [1.0 if i == p else 0.0 for i in range(9)])
            for q in range(9):
                cov[p, q] = s2 * w[q] if free_l[p] and free_l[q] else 0.0
    final = costs(poses, cam)
    recs = [SimpleNamespace(R=poses[i][0], t=poses[i][1], rms_px=math.sqrt(final[i] / float(4 * ntags[i])),
                            n_tags=ntags[i], used=True) if used[i] else
            SimpleNamespace(R=np.zeros((3, 3)), t=np.zeros(3), rms_px=0.0, n_tags=0, used=False) for i in range(N)]
    return SimpleNamespace(params=np.array(cam), cov=cov, cov_valid=valid,
                           rms_before=math.sqrt(cost0 / corners) if corners else 0.0,
                           rms_after=math.sqrt(cost / corners) if corners else 0.0, views_used=n_used,
                           views_skipped=N - n_used, corners=corners, accepted=accepted, rejected=rejected,
                           views=recs, cost=cost, start=np.array(start_cam))


def same_result(a, b):
    """Every field of two calibration results (library or restatement) equal, the doubles bit for bit."""
    return (a.views_used == b.views_used and a.views_skipped == b.views_skipped and a.corners == b.corners
            and a.accepted == b.accepted and a.rejected == b.rejected and bool(a.cov_valid) == bool(b.cov_valid)
            and a.rms_before == b.rms_before and a.rms_after == b.rms_after
            and np.array_equal(a.params, b.params) and np.array_equal(a.cov, b.cov))


def same_views(a, b):
    return len(a) == len(b) and all(
        x.used == y.used and x.n_tags == y.n_tags and x.rms_px == y.rms_px and np.array_equal(x.R, y.R)
        and np.array_equal(x.t, y.t) for x, y in zip(a, b))


# ---- rendered views for the end-to-end GPU test ------------------------------------------------------
# A 2 x 3 grid of 0.1 m tags 0.14 m apart (the quiet zones, 0.125 m, stay apart) in front of
# field_pose_cases.GPU_CAM at 0.8 m: a tag is about 75 px across.  Every view is tilted, so the focal
# guess has its two constraints.  (rx, ry, rz in degrees, then where the board's centre stands.)
E2E_CAM = np.array([fc.GPU_CAM.fx, fc.GPU_CAM.fy, fc.GPU_CAM.cx, fc.GPU_CAM.cy, 0, 0, 0, 0, 0], np.float64)
E2E_TAG, E2E_PITCH = 0.1, 0.14
E2E_BOARD = grid_board(2, 3, 0, E2E_TAG, E2E_PITCH)
E2E_CENTRE = np.array([E2E_PITCH, E2E_PITCH / 2.0, 0.0])
E2E_VIEWS = [(25.0, 0.0, 3.0, (0.0, 0.0, 0.8)), (-25.0, 5.0, -4.0, (0.02, -0.01, 0.8)),
             (0.0, 28.0, 2.0, (-0.02, 0.02, 0.8)), (3.0, -28.0, -3.0, (0.01, 0.0, 0.8)),
             (18.0, 18.0, 10.0, (0.0, 0.01, 0.85)), (-15.0, -20.0, -8.0, (-0.01, -0.02, 0.85))]


def e2e_pose(k):
    rx, ry, rz, where = E2E_VIEWS[k]
    R = fc.rot_xyz(rx, ry, rz)
    return R, np.asarray(where, np.float64) - R @ E2E_CENTRE


def render_board_view(k, draw_tag, codes, blank):
    """gray uint8 [480, 640] of view k of the board, drawn as field_pose_cases.render_scene draws."""
    R, t = e2e_pose(k)
    img = blank()
    for tid, Rt, tt in E2E_BOARD:
        px, z = project(E2E_CAM, R, t, fc.tag_corners_field(Rt, tt, E2E_TAG, fc.QUIET))
        assert (z > 0).all() and px.min() >= 0 and (px[:, 0] <= 639).all() and (px[:, 1] <= 479).all(), (k, tid)
        draw_tag(img, codes[tid], px[[3, 2, 1, 0]])               # draw_tag takes TL, TR, BR, BL
    return img
