"""Scenes and the numpy restatement for the rig-pose tests (tests/test_rig_pose_host.py,
tests/test_rig_pose_gpu.py).

Conventions (include/at_api.h): a rig camera has intrinsics (fx, fy, cx, cy) and extrinsics
x_robot = E_R x_cam + E_t; the rig pose is the robot in the field, x_field = R x_robot + t.  A
field point X projects as Q = R^T (X - t), P = E_R^T (Q - E_t), u = fx Px / Pz + cx,
v = fy Py / Pz + cy.  Layout tags, tag frame and corner order are tests/field_pose_cases.py's.

The field here is field_pose_cases.GPU_LAYOUT (walls A and B) plus wall C, turned about y by
-50 degrees on the other side.  Nothing here needs the library or a GPU.
"""
import math
from types import SimpleNamespace

import numpy as np

import field_pose_cases as fc

TAG_SIZE = fc.TAG_SIZE
MAX_CAMS = 8
ITERS = fc.ITERS

RIG_LAYOUT = fc.GPU_LAYOUT + [fc.wall_b(5, -0.62, 0.1, -0.12, -50.0), fc.wall_b(6, -0.70, -0.18, -0.2, -50.0),
                              fc.wall_b(7, -0.82, 0.12, -0.36, -50.0)]
FOREIGN = fc.FOREIGN

CAM_A = fc.GPU_CAM
CAM_B = SimpleNamespace(fx=600.0, fy=605.0, cx=318.0, cy=243.0)
CAM_C = SimpleNamespace(fx=640.0, fy=636.0, cx=322.5, cy=238.0)


# ---- geometry ---------------------------------------------------------------------------------
def camera_in_field(Rr, tr, ER, Et):
    """(Rc, tc) of x_cam = Rc x_field + tc for the robot at (Rr, tr) and a camera mounted at (ER, Et)."""
    Rc = ER.T @ Rr.T
    return Rc, -ER.T @ (Rr.T @ tr + Et)


def mount_of(Rr, tr, Rc, tc):
    """The extrinsics (ER, Et) of a camera whose field pose is x_cam = Rc x_field + tc on the robot
    at (Rr, tr)."""
    return Rr.T @ Rc.T, Rr.T @ (-Rc.T @ tc - tr)


def rig_camera(dets, poses, cam, ER=None, Et=None):
    return SimpleNamespace(dets=list(dets), poses=list(poses), cam=cam,
                           ER=np.eye(3) if ER is None else np.asarray(ER, np.float64),
                           Et=np.zeros(3) if Et is None else np.asarray(Et, np.float64))


def as_host_args(cams):
    """The `cameras` argument of ros_vision_amd.rig_pose_host."""
    return [(c.dets, c.poses, c.cam, (c.ER, c.Et)) for c in cams]


# ---- the algorithm, restated ------------------------------------------------------------------
# Expression order is csrc/at_rigpose.h's; a sum over the corners is the 64-slot tree per camera
# (field_pose_cases._tree), then ((c0 + c1) + c2) + ... over the cameras in order.
def _across(parts):
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


def _rot(M, v):
    return np.array([(M[r, 0] * v[0] + M[r, 1] * v[1]) + M[r, 2] * v[2] for r in range(3)])


def points_cam(c, R, t, X):
    """(Q, P) [n, 3] of the field points X for camera c under the robot pose (R, t)."""
    d = X - t
    Q = np.stack([(R[0, k] * d[:, 0] + R[1, k] * d[:, 1]) + R[2, k] * d[:, 2] for k in range(3)], 1)
    e = Q - c.Et
    P = np.stack([(c.ER[0, k] * e[:, 0] + c.ER[1, k] * e[:, 1]) + c.ER[2, k] * e[:, 2] for k in range(3)], 1)
    return Q, P


def project_rig(c, R, t, X):
    """[n, 2] pixels of the field points X in camera c."""
    _Q, P = points_cam(c, R, t, X)
    return np.stack([c.cam.fx * (P[:, 0] / P[:, 2]) + c.cam.cx, c.cam.fy * (P[:, 1] / P[:, 2]) + c.cam.cy], 1)


def _cam_cost(c, R, t, X, uv):
    if not len(X):
        return 0.0
    with np.errstate(all="ignore"):
        _Q, P = points_cam(c, R, t, X)
        ru = (c.cam.fx * (P[:, 0] / P[:, 2]) + c.cam.cx) - uv[:, 0]
        rv = (c.cam.fy * (P[:, 1] / P[:, 2]) + c.cam.cy) - uv[:, 1]
        e = np.where(P[:, 2] > 0.0, ru * ru + rv * rv, math.inf)
    return fc._tree(e)


def _cost(cams, pts, R, t):
    return _across([_cam_cost(c, R, t, X, uv) for c, (X, uv) in zip(cams, pts)])


def jacobian_rows(c, R, t, X):
    """(ju, jv, P): the rows du/d(w, dt), dv/d(w, dt) [n, 6] of the points X in camera c, with
    R' = R dR(w), t' = t + dt."""
    Q, P = points_cam(c, R, t, X)
    xn, yn = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    A, B = c.cam.fx / P[:, 2], -(c.cam.fx * xn) / P[:, 2]
    Cc, D = c.cam.fy / P[:, 2], -(c.cam.fy * yn) / P[:, 2]
    zero = np.zeros(len(X))
    dQ = [[zero, -Q[:, 2], Q[:, 1], -R[0, 0], -R[1, 0], -R[2, 0]],
          [Q[:, 2], zero, -Q[:, 0], -R[0, 1], -R[1, 1], -R[2, 1]],
          [-Q[:, 1], Q[:, 0], zero, -R[0, 2], -R[1, 2], -R[2, 2]]]
    ju, jv = [], []
    for k in range(6):
        m = [(c.ER[0, r] * dQ[0][k] + c.ER[1, r] * dQ[1][k]) + c.ER[2, r] * dQ[2][k] for r in range(3)]
        ju.append(A * m[0] + B * m[2])
        jv.append(Cc * m[1] + D * m[2])
    return np.stack(ju, 1), np.stack(jv, 1), P


def _cam_normal(c, R, t, X, uv):
    if not len(X):
        return [0.0] * 27
    ju, jv, P = jacobian_rows(c, R, t, X)
    ru = (c.cam.fx * (P[:, 0] / P[:, 2]) + c.cam.cx) - uv[:, 0]
    rv = (c.cam.fy * (P[:, 1] / P[:, 2]) + c.cam.cy) - uv[:, 1]
    out = [fc._tree(ju[:, i] * ju[:, j] + jv[:, i] * jv[:, j]) for i, j in fc._TRI]
    return out + [fc._tree(ju[:, i] * ru + jv[:, i] * rv) for i in range(6)]


def _normal(cams, pts, R, t):
    per = [_cam_normal(c, R, t, X, uv) for c, (X, uv) in zip(cams, pts)]
    v = [_across([p[k] for p in per]) for k in range(27)]
    return {ij: v[k] for k, ij in enumerate(fc._TRI)}, v[21:]


def apply_step(R, t, d):
    """R' = R dR(w), t' = t + dt for d = (w, dt)."""
    h = [0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]
    n = math.sqrt(1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]))
    dR = fc._quat_to_R(1.0 / n, h[0] / n, h[1] / n, h[2] / n)
    return fc._mul(R, dR), np.array([t[k] + d[3 + k] for k in range(3)])


def solve_rig_ref(cams, layout, max_hamming=0, tag_size=TAG_SIZE):
    """The rig pose of one instant as include/at_api.h defines it.  Returns a namespace with the
    record's fields and, for the tests, cost."""
    lay = {int(tid): (np.asarray(R, np.float64), np.asarray(t, np.float64)) for tid, R, t in layout}
    n_cams = len(cams)
    sels = [fc.select_ref(c.dets, lay, max_hamming) for c in cams]
    tags_per_cam = [len(s) for s in sels] + [0] * (MAX_CAMS - n_cams)
    ids = [[int(c.dets[i].id) for i in s] for c, s in zip(cams, sels)] + [[] for _ in range(MAX_CAMS - n_cams)]
    n_tags = sum(tags_per_cam)
    none = SimpleNamespace(n_tags=0, n_cams_used=0, tags_per_cam=[0] * MAX_CAMS, ids=[[] for _ in range(MAX_CAMS)],
                           R=np.zeros((3, 3)), t=np.zeros(3), cov=np.zeros((6, 6)), cov_valid=False, rms_px=0.0,
                           steps_taken=0, rejected=0, cost=math.inf)
    hs = tag_size / 2.0
    pts = []
    for c, sel in zip(cams, sels):
        X, uv = [], []
        for i in sel:
            Rt, tt = lay[c.dets[i].id]
            for k, (sx, sy) in enumerate(fc.CORNER_SIGNS):
                X.append([(Rt[r, 0] * (sx * hs) + Rt[r, 1] * (sy * hs)) + tt[r] for r in range(3)])
                uv.append(np.asarray(c.dets[i].p, np.float64)[k])
        pts.append((np.array(X).reshape(-1, 3), np.array(uv).reshape(-1, 2)))
    cost, R, t = math.inf, None, None
    for c, sel in zip(cams, sels):
        for i in sel:
            Rt, tt = lay[c.dets[i].id]
            Rfc = fc._mul(Rt, np.asarray(c.poses[i].R, np.float64).T)
            tfc = tt - _rot(Rfc, np.asarray(c.poses[i].t, np.float64))
            Rj = fc._mul(Rfc, c.ER.T)
            tj = tfc - _rot(Rj, c.Et)
            cj = _cost(cams, pts, Rj, tj)
            if cj < cost:
                cost, R, t = cj, Rj, tj
    if R is None:
        return none
    R = fc._project_rotation(R)
    c0 = _cost(cams, pts, R, t)
    if c0 < math.inf:
        cost = c0
    lam, steps, rejected = 1e-3, 0, 0
    for _ in range(ITERS):
        a, g = _normal(cams, pts, R, t)
        d = fc._solve6(a, g, lam)
        take = d is not None
        if take:
            Rn, tn = apply_step(R, t, d)
            cn = _cost(cams, pts, Rn, tn)
            take = cn < cost
        if take:
            R, t, cost, steps = Rn, tn, cn, steps + 1
            lam = max(lam / 10.0, 1e-9)
        else:
            rejected += 1
            lam = lam * 10.0
    a, _g = _normal(cams, pts, R, t)
    s2 = cost / float(8 * n_tags - 6)
    cov, cov_valid = np.zeros((6, 6)), True
    for k in range(6):
        x = fc._solve6(a, [-1.0 if i == k else -0.0 for i in range(6)], 0.0)
        if x is None:
            cov_valid = False
            break
        cov[k] = [s2 * x[i] for i in range(6)]
    if not cov_valid:
        cov = np.zeros((6, 6))
    return SimpleNamespace(n_tags=n_tags, n_cams_used=sum(1 for m in tags_per_cam if m), tags_per_cam=tags_per_cam,
                           ids=ids, R=R, t=t, cov=cov, cov_valid=cov_valid, rms_px=math.sqrt(cost / float(4 * n_tags)),
                           steps_taken=steps, rejected=rejected, cost=cost)


def same_record(a, b):
    """Every field of two rig records (library or restatement) equal, the doubles bit for bit."""
    return (a.n_tags == b.n_tags and a.n_cams_used == b.n_cams_used and list(a.tags_per_cam) == list(b.tags_per_cam)
            and [list(x) for x in a.ids] == [list(x) for x in b.ids] and a.steps_taken == b.steps_taken
            and a.rejected == b.rejected and bool(a.cov_valid) == bool(b.cov_valid) and a.rms_px == b.rms_px
            and np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and np.array_equal(a.cov, b.cov))


# ---- synthetic instants for the CPU tests -----------------------------------------------------
# robot pose, and per camera (layout ids it sees, mount: camera centre in the robot frame and its
# turn rx, ry, rz from looking along the robot's +z, intrinsics)
ROBOT = (fc.rot_xyz(2.0, -3.0, 1.5), np.array([0.03, 0.02, -1.3]))
MOUNTS = [
    ((0, 1, 3), (0.02, -0.02, 0.0), -4.0, -2.0, 0.5, CAM_A),
    ((2, 3, 4), (0.14, 0.0, 0.03), 1.0, -14.0, -1.0, CAM_B),
    ((0, 5, 6, 7), (-0.16, 0.01, 0.02), 2.0, 17.0, 1.0, CAM_C),
    ((0, 1, 2), (0.0, 0.08, -0.05), 6.0, 1.0, -2.0, CAM_B),
]


def mount(k):
    """(ids, ER, Et, intrinsics) of MOUNTS[k]: the camera looks along its +z."""
    ids, centre, rx, ry, rz, cam = MOUNTS[k]
    return ids, fc.rot_xyz(rx, ry, rz).T, np.asarray(centre, np.float64), cam


def make_instant(mounts, rng, robot=ROBOT, noise_px=0.0, pose_rot_deg=3.0, pose_t_m=0.03, layout=None):
    """Rig cameras (rig_camera) for the robot at `robot`: MOUNTS[k] for every k of `mounts`; None
    is a camera that sees nothing, "foreign" one that sees only an id outside the layout."""
    where = {g[0]: g for g in (layout or RIG_LAYOUT)}
    Rr, tr = robot
    out = []
    for k in mounts:
        if k is None:
            out.append(rig_camera([], [], CAM_A))
            continue
        if k == "foreign":
            ids, ER, Et, cam = mount(0)
            seen = [FOREIGN[11]]
        else:
            ids, ER, Et, cam = mount(k)
            seen = [where[i] for i in ids]
        Rc, tc = camera_in_field(Rr, tr, ER, Et)
        dets, poses = fc.make_frame(seen, Rc, tc, rng, cam=cam, noise_px=noise_px, pose_rot_deg=pose_rot_deg,
                                    pose_t_m=pose_t_m)
        out.append(rig_camera(dets, poses, cam, ER, Et))
    return out


# ---- rendered frames for the GPU tests -----------------------------------------------------------
# 640 x 480; view name -> (ids drawn, camera centre in the field, rx, ry, rz, intrinsics); the
# robot of every rendered instant is RENDER_ROBOT, so a view's extrinsics are mount_of(...).
RENDER_ROBOT = (fc.rot_xyz(1.0, -2.0, 1.0), np.array([0.0, 0.03, -1.32]))
VIEWS = {
    "front": ((0, 1, 3), (0.05, 0.0, -1.3), -4.0, -5.0, 2.0, CAM_A),
    "right": ((2, 3, 4), (0.2, 0.02, -1.25), 2.0, -10.0, -2.0, CAM_B),
    "left": ((0, 5, 6, 7), (-0.2, 0.0, -1.3), 3.0, 14.0, 1.0, CAM_C),
    "wall_a": ((0, 1, 2), (-0.05, 0.0, -1.25), 5.0, 4.0, 3.0, CAM_A),
    "foreign": ((11,), (0.0, 0.0, -1.2), 2.0, 3.0, -3.0, CAM_A),
    "blank": ((), (0.0, 0.0, -1.2), 0.0, 0.0, 0.0, CAM_A),
}


def view_pose(name):
    _ids, centre, rx, ry, rz, _cam = VIEWS[name]
    return fc.camera_pose(centre, rx, ry, rz)


def view_mount(name):
    """(ER, Et) of the view on RENDER_ROBOT."""
    return mount_of(*RENDER_ROBOT, *view_pose(name))


def view_corners(name):
    """{id: [4, 2] the black border's corners in p order} of a view."""
    ids, _c, _rx, _ry, _rz, cam = VIEWS[name]
    R, t = view_pose(name)
    where = {g[0]: g for g in RIG_LAYOUT}
    where.update(FOREIGN)
    return {tid: fc.project(cam, R, t, fc.tag_corners_field(where[tid][1], where[tid][2]))[0] for tid in ids}


def render_view(name, draw_tag, codes, blank):
    """gray uint8 [480, 640] of a view -- draw_tag, codes and blank are tests/tag_scenes.py's."""
    ids, _c, _rx, _ry, _rz, cam = VIEWS[name]
    R, t = view_pose(name)
    img = blank()
    where = {g[0]: g for g in RIG_LAYOUT}
    where.update(FOREIGN)
    for tid in ids:
        _tid, Rt, tt = where[tid]
        px, z = fc.project(cam, R, t, fc.tag_corners_field(Rt, tt, TAG_SIZE, fc.QUIET))
        assert (z > 0).all() and px.min() >= 0 and (px[:, 0] <= 639).all() and (px[:, 1] <= 479).all(), (name, tid)
        draw_tag(img, codes[tid], px[[3, 2, 1, 0]])               # draw_tag takes TL, TR, BR, BL
    return img
