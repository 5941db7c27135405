"""Scenes and the numpy restatement for the field-pose tests (tests/test_field_pose_host.py,
tests/test_field_pose_gpu.py).

Conventions (include/at_api.h): a layout tag is (id, R, t) with x_field = R x_tag + t; the tag
frame is at_pose's -- x to the right and y down on the upright tag, z into it, the corners of
at_detection.p at (-s/2, s/2), (s/2, s/2), (s/2, -s/2), (-s/2, -s/2) with s the tag size (black
border edge to edge).  A field pose is x_cam = R x_field + t; pixels are fx X/Z + cx, fy Y/Z + cy.

The field used here: wall A is the plane z = 0 seen from z < 0 (tags with R = I), wall B is
turned about y by 50 degrees.  Nothing here needs the library or a GPU.
"""
import math
from types import SimpleNamespace

import numpy as np

TAG_SIZE = 0.1651
CAM = SimpleNamespace(fx=905.495617, fy=907.909470, cx=609.916016, cy=352.682645)   # detector.TEST_CAMERA
MAX_TAGS = 16
ITERS = 12


# ---- geometry ---------------------------------------------------------------------------------
def rot_y(deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_xyz(rx, ry, rz):
    """Rz Ry Rx, degrees."""
    ax, ay, az = (math.radians(v) for v in (rx, ry, rz))
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def wall_a(tid, x, y):
    return (tid, np.eye(3), np.array([x, y, 0.0]))


def wall_b(tid, x, y, z, deg=50.0):
    return (tid, rot_y(deg), np.array([x, y, z]))


LAYOUT_ONE = [wall_a(3, 0.0, 0.0)]
LAYOUT_COPLANAR = [wall_a(1, -0.6, 0.1), wall_a(4, 0.0, -0.2), wall_a(7, 0.6, 0.15)]
LAYOUT_TWO_WALLS = [wall_a(2, -0.5, 0.0), wall_a(5, 0.1, 0.2), wall_b(9, 0.9, -0.1, -0.4)]
LAYOUTS = {"one": LAYOUT_ONE, "coplanar": LAYOUT_COPLANAR, "two_walls": LAYOUT_TWO_WALLS}

CORNER_SIGNS = ((-1, 1), (1, 1), (1, -1), (-1, -1))   # at_detection.p order in the tag frame


def tag_corners_field(R, t, tag_size=TAG_SIZE, scale=1.0):
    """[4, 3] the corners (p order) of a layout tag in the field frame; scale > 1 widens the
    square about its centre (the quiet zone's corners for drawing)."""
    h = tag_size / 2.0 * scale
    return np.array([R @ np.array([sx * h, sy * h, 0.0]) + t for sx, sy in CORNER_SIGNS])


def project(cam, R, t, X):
    P = X @ R.T + t
    return np.stack([cam.fx * P[:, 0] / P[:, 2] + cam.cx, cam.fy * P[:, 1] / P[:, 2] + cam.cy], 1), P[:, 2]


def camera_pose(centre, rx, ry, rz):
    """(R, t) of x_cam = R x_field + t for a camera at `centre` (field frame) turned by the
    three angles (degrees) from looking along +z."""
    R = rot_xyz(rx, ry, rz)
    return R, -R @ np.asarray(centre, np.float64)


def random_camera(rng):
    """A camera 2-4 m in front of wall A, up to 15 degrees off on every axis."""
    c = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), -rng.uniform(2.0, 4.0)])
    return camera_pose(c, *rng.uniform(-15, 15, 3))


def small_rotation(rng, deg):
    v = rng.normal(size=3)
    v *= math.radians(deg) / np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    a = np.linalg.norm(v)
    return np.eye(3) + math.sin(a) / a * K + (1 - math.cos(a)) / (a * a) * K @ K


def make_frame(layout, R, t, rng, cam=CAM, noise_px=0.0, pose_rot_deg=3.0, pose_t_m=0.03, tag_size=TAG_SIZE):
    """What one frame of `layout` seen from (R, t) gives the solver: a detection (exact corners,
    plus noise_px of Gaussian noise) and a single-tag pose (the true one turned by pose_rot_deg
    and moved by pose_t_m: as far off as the two-minimum ambiguity leaves a coplanar pose) per tag,
    in id order.  Returns (detections, poses)."""
    dets, poses = [], []
    for tid, Rt, tt in sorted(layout, key=lambda g: g[0]):
        px, _z = project(cam, R, t, tag_corners_field(Rt, tt, tag_size))
        if noise_px:
            px = px + rng.normal(scale=noise_px, size=px.shape)
        dets.append(SimpleNamespace(id=int(tid), hamming=0, decision_margin=60.0, H=np.eye(3), c=px.mean(0), p=px))
        Rp = small_rotation(rng, pose_rot_deg) @ (R @ Rt) if pose_rot_deg else R @ Rt
        tp = R @ tt + t + (rng.normal(scale=pose_t_m, size=3) if pose_t_m else 0.0)
        poses.append(SimpleNamespace(id=int(tid), R=Rp, t=tp, err=0.0))
    return dets, poses


# ---- the algorithm, restated ------------------------------------------------------------------
# Every sum over the corners is the tree over 64 slots the library fixes ((i, i + 32), (i, i + 16),
# ...), every expression is written in the library's order, in float64 without contraction: the
# accept / reject decisions, hence steps_taken, are the library's.
def _tree(v):
    a = np.zeros(64)
    a[:len(v)] = v
    n = 32
    while n >= 1:
        a = a[:n] + a[n:2 * n]
        n //= 2
    return float(a[0])


def _quat_to_R(q0, q1, q2, q3):
    xx, yy, zz = q1 * q1, q2 * q2, q3 * q3
    xy, xz, yz = q1 * q2, q1 * q3, q2 * q3
    wx, wy, wz = q0 * q1, q0 * q2, q0 * q3
    return np.array([[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
                     [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
                     [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]])


def _project_rotation(M):
    R = [float(x) for x in M.reshape(9)]
    tr = (R[0] + R[4]) + R[8]
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0
        q = (0.25 * s, (R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s)
    elif R[0] > R[4] and R[0] > R[8]:
        s = math.sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0
        q = ((R[7] - R[5]) / s, 0.25 * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s)
    elif R[4] > R[8]:
        s = math.sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0
        q = ((R[2] - R[6]) / s, (R[1] + R[3]) / s, 0.25 * s, (R[5] + R[7]) / s)
    else:
        s = math.sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0
        q = ((R[3] - R[1]) / s, (R[2] + R[6]) / s, (R[5] + R[7]) / s, 0.25 * s)
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return _quat_to_R(q[0] / n, q[1] / n, q[2] / n, q[3] / n)


def _mul(a, b):
    """3x3 product, every entry (p + q) + r."""
    return np.array([[(a[r, 0] * b[0, k] + a[r, 1] * b[1, k]) + a[r, 2] * b[2, k] for k in range(3)]
                     for r in range(3)])


def _points_cam(R, t, X):
    Q = np.stack([(R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2] for r in range(3)], 1)
    return Q, Q + t


def _cost(cam, R, t, X, uv):
    _Q, P = _points_cam(R, t, X)
    ru = (cam.fx * (P[:, 0] / P[:, 2]) + cam.cx) - uv[:, 0]
    rv = (cam.fy * (P[:, 1] / P[:, 2]) + cam.cy) - uv[:, 1]
    return _tree(ru * ru + rv * rv), bool((~(P[:, 2] > 0.0)).any())


_TRI = [(i, j) for i in range(6) for j in range(i, 6)]


def _normal(cam, R, t, X, uv):
    Q, P = _points_cam(R, t, X)
    xn, yn = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    ru = (cam.fx * xn + cam.cx) - uv[:, 0]
    rv = (cam.fy * yn + cam.cy) - uv[:, 1]
    A, B = cam.fx / P[:, 2], -(cam.fx * xn) / P[:, 2]
    C, D = cam.fy / P[:, 2], -(cam.fy * yn) / P[:, 2]
    zero = np.zeros(len(X))
    ju = [B * Q[:, 1], A * Q[:, 2] - B * Q[:, 0], -(A * Q[:, 1]), A, zero, B]
    jv = [D * Q[:, 1] - C * Q[:, 2], -(D * Q[:, 0]), C * Q[:, 0], zero, C, D]
    a = {(i, j): _tree(ju[i] * ju[j] + jv[i] * jv[j]) for i, j in _TRI}
    g = [_tree(ju[i] * ru + jv[i] * rv) for i in range(6)]
    return a, g


def _solve6(a, g, lam):
    L = [[0.0] * 6 for _ in range(6)]
    ok = True
    for j in range(6):
        s = a[(j, j)] + lam * a[(j, j)]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            v = a[(j, i)]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        v = -g[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    return x if ok else None


def select_ref(dets, layout_ids, max_hamming):
    """Indices into dets of the tags used, ascending id: per id the lowest hamming, then the
    greatest margin, then the lowest index; the 16 lowest ids."""
    best = {}
    for i, d in enumerate(dets):
        if d.id not in layout_ids or not 0 <= d.hamming <= max_hamming:
            continue
        key = (d.hamming, -float(np.float32(d.decision_margin)), i)
        if d.id not in best or key < best[d.id][0]:
            best[d.id] = (key, i)
    return [best[tid][1] for tid in sorted(best)][:MAX_TAGS]


def solve_ref(dets, poses, layout, max_hamming=0, cam=CAM, tag_size=TAG_SIZE):
    """The field pose of one frame as include/at_api.h defines it.  Returns a namespace with
    n_tags, ids, R, t, rms_px, steps_taken and, for the tests, start_cost and cost."""
    lay = {int(tid): (np.asarray(R, np.float64), np.asarray(t, np.float64)) for tid, R, t in layout}
    sel = select_ref(dets, lay, max_hamming)
    none = SimpleNamespace(n_tags=0, ids=[], R=np.zeros((3, 3)), t=np.zeros(3), rms_px=0.0, steps_taken=0,
                           start_cost=math.inf, cost=math.inf)
    if not sel:
        return none
    hs = tag_size / 2.0
    X, uv = [], []
    for i in sel:
        Rt, tt = lay[dets[i].id]
        for c, (sx, sy) in enumerate(CORNER_SIGNS):
            X.append([(Rt[k, 0] * (sx * hs) + Rt[k, 1] * (sy * hs)) + tt[k] for k in range(3)])
            uv.append(np.asarray(dets[i].p, np.float64)[c])
    X, uv = np.array(X), np.array(uv)
    cost, R, t = math.inf, None, None
    for i in sel:
        Rt, tt = lay[dets[i].id]
        Rj = _mul(np.asarray(poses[i].R, np.float64), Rt.T)
        rt = np.array([(Rj[r, 0] * tt[0] + Rj[r, 1] * tt[1]) + Rj[r, 2] * tt[2] for r in range(3)])
        tj = np.asarray(poses[i].t, np.float64) - rt
        cj, behind = _cost(cam, Rj, tj, X, uv)
        if not behind and cj < cost:
            cost, R, t = cj, Rj, tj
    if R is None:
        return none
    start_cost = cost
    R = _project_rotation(R)
    c0, behind = _cost(cam, R, t, X, uv)
    if not behind and c0 == c0:
        cost = c0
    lam, steps = 1e-3, 0
    for _ in range(ITERS):
        a, g = _normal(cam, R, t, X, uv)
        d = _solve6(a, g, lam)
        take = d is not None
        if take:
            h = [0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]
            n = math.sqrt(1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]))
            Rn = _mul(_quat_to_R(1.0 / n, h[0] / n, h[1] / n, h[2] / n), R)
            tn = np.array([t[k] + d[3 + k] for k in range(3)])
            cn, behind = _cost(cam, Rn, tn, X, uv)
            take = not behind and cn < cost
        if take:
            R, t, cost, steps = Rn, tn, cn, steps + 1
            lam = max(lam / 10.0, 1e-9)
        else:
            lam = lam * 10.0
    return SimpleNamespace(n_tags=len(sel), ids=[int(dets[i].id) for i in sel], R=R, t=t,
                           rms_px=math.sqrt(cost / float(4 * len(sel))), steps_taken=steps, start_cost=start_cost,
                           cost=cost)


def cost_of(dets, layout, R, t, ids, cam=CAM, tag_size=TAG_SIZE):
    """Summed squared reprojection error of the tags `ids` (each one's first detection) under (R, t)."""
    lay = {int(tid): (np.asarray(Rt, np.float64), np.asarray(tt, np.float64)) for tid, Rt, tt in layout}
    total = 0.0
    for tid in ids:
        d = next(x for x in dets if x.id == tid)
        px, _z = project(cam, np.asarray(R), np.asarray(t), tag_corners_field(*lay[tid], tag_size))
        total += float(((px - np.asarray(d.p)) ** 2).sum())
    return total


# ---- rendered frames for the GPU tests -----------------------------------------------------------
# 640 x 480, a camera whose principal point is the image centre; every tag at least 48 px across.
GPU_CAM = SimpleNamespace(fx=620.0, fy=620.0, cx=320.0, cy=240.0)
QUIET = 10.0 / 8.0     # tag36h11: (d + 4) cells across the drawn bitmap over (d + 2) across the border

GPU_LAYOUT = [wall_a(0, -0.33, -0.12), wall_a(1, -0.05, 0.14), wall_a(2, 0.2, -0.15), wall_b(3, 0.5, 0.1, -0.12),
              wall_b(4, 0.58, -0.18, -0.2)]
# frame name -> (ids drawn, camera centre, rx, ry, rz); id 11 is in no layout
GPU_SCENES = {
    "one": ((1,), (0.0, 0.0, -1.2), 4.0, -3.0, 2.0),
    "two_coplanar": ((0, 2), (-0.05, -0.1, -1.3), -3.0, 2.0, -4.0),
    "three_coplanar": ((0, 1, 2), (-0.05, 0.0, -1.25), 5.0, 4.0, 3.0),
    "three_two_walls": ((0, 1, 3), (0.05, 0.0, -1.3), -4.0, -5.0, 2.0),
    "five": ((0, 1, 2, 3, 4), (0.1, 0.0, -1.35), 3.0, -4.0, -2.0),
    "none": ((), (0.0, 0.0, -1.2), 0.0, 0.0, 0.0),
    "foreign": ((1, 11), (0.0, 0.0, -1.2), 2.0, 3.0, -3.0),
    "only_foreign": ((11,), (0.0, 0.0, -1.2), 2.0, 3.0, -3.0),
}
FOREIGN = {11: wall_a(11, 0.25, 0.12)}   # where the id outside the layout is drawn


def render_scene(name, draw_tag, codes, blank):
    """(gray uint8 [480, 640], (R, t) of the camera, ids drawn) -- draw_tag, codes and blank are
    tests/tag_scenes.py's."""
    ids, centre, rx, ry, rz = GPU_SCENES[name]
    R, t = camera_pose(centre, rx, ry, rz)
    img = blank()
    where = {g[0]: g for g in GPU_LAYOUT}
    where.update(FOREIGN)
    for tid in ids:
        _tid, Rt, tt = where[tid]
        q = tag_corners_field(Rt, tt, TAG_SIZE, QUIET)           # p order: BL, BR, TR, TL of the upright tag
        px, z = project(GPU_CAM, R, t, q)
        assert (z > 0).all()
        draw_tag(img, codes[tid], px[[3, 2, 1, 0]])               # draw_tag takes TL, TR, BR, BL
    return img, (R, t), ids
