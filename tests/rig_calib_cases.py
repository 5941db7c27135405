"""Scenes and the numpy restatement for the rig-calibration tests (tests/test_rig_calib_host.py,
tests/test_rig_calib_gpu.py).

Built on tests/rig_pose_cases.py: its mounts, layout, make_instant and the restated rig pose (the
calibration's start).  A calibration camera is (intrinsics, ER, Et, free_rot, free_trans); an
instant is make_instant's list of rig cameras.  Nothing here needs the library or a GPU.
"""
import math
from types import SimpleNamespace

import numpy as np

import field_pose_cases as fc
import rig_pose_cases as rc

ITERS = 16
CHUNK = 32
MAX_INSTANTS = 4096
NAN6 = [math.nan] * 6


# ---- scenes ---------------------------------------------------------------------------------------
def robot_poses(n, rng, turn_deg=6.0, move_m=0.08):
    """n robot poses around rig_pose_cases.ROBOT: every mount still sees its tags in front."""
    return [(fc.small_rotation(rng, turn_deg) @ rc.ROBOT[0], rc.ROBOT[1] + rng.uniform(-move_m, move_m, 3))
            for _ in range(n)]


def true_camera(k, free_rot=True, free_trans=True):
    """The calibration camera of MOUNTS[k] at its true mount."""
    _ids, ER, Et, cam = rc.mount(k)
    return SimpleNamespace(cam=cam, ER=ER.copy(), Et=Et.copy(), free_rot=free_rot, free_trans=free_trans)


def perturbed(c, rng, rot_deg=3.0, move_m=0.03):
    """c with its mount turned by rot_deg and moved by move_m (make_instant's defaults for a pose)."""
    d = rng.normal(size=3)
    return SimpleNamespace(cam=c.cam, ER=c.ER @ fc.small_rotation(rng, rot_deg), Et=c.Et + move_m * d / np.linalg.norm(d),
                           free_rot=c.free_rot, free_trans=c.free_trans)


def fixed(c):
    return SimpleNamespace(cam=c.cam, ER=c.ER, Et=c.Et, free_rot=False, free_trans=False)


def make_instants(mounts, robots, rng, noise_px=0.0, blind=None):
    """One make_instant per robot pose; blind = {instant index: [camera indices that see nothing]}."""
    out = []
    for i, robot in enumerate(robots):
        ms = [None if c in (blind or {}).get(i, ()) else k for c, k in enumerate(mounts)]
        out.append(rc.make_instant(ms, rng, robot=robot, noise_px=noise_px))
    return out


def as_create_args(cams):
    """The `cameras` argument of ros_vision_amd.RigCalibrator."""
    return [(c.cam, (c.ER, c.Et), c.free_rot, c.free_trans) for c in cams]


def as_add_args(instant):
    return [(c.dets, c.poses) for c in instant]


def stored(instant, layout=rc.RIG_LAYOUT, max_hamming=0):
    """What at_rigcal_add says of the instant: two cameras or more have a selected tag."""
    lay = {int(g[0]) for g in layout}
    return sum(1 for c in instant if fc.select_ref(c.dets, lay, max_hamming)) >= 2


def calibrator(rva, cams, instants, **kw):
    """A RigCalibrator over cams holding the instants it stores, and those instants."""
    cal = rva.RigCalibrator(as_create_args(cams), rc.RIG_LAYOUT, **kw)
    kept = [inst for inst in instants if cal.add(as_add_args(inst))]
    assert len(cal) == len(kept) == sum(1 for inst in instants if stored(inst, max_hamming=kw.get("max_hamming", 0)))
    return cal, kept


# The cases both test files use: (true cameras, starting cameras, instants).  Camera 0 is held fixed
# at its true mount; the others start 3 degrees and 30 mm off in what they are free in.
def two_camera_case(rng, n, noise_px=0.0):
    true = [fixed(true_camera(0)), true_camera(1)]
    start = [true[0], perturbed(true[1], rng)]
    return true, start, make_instants([0, 1], robot_poses(n, rng), rng, noise_px=noise_px)


def three_camera_case(rng, n, noise_px=0.3, blind=None):
    """Camera 2 is free_rot only and sees nothing in instants 4, 17 and 32 (where there are such)."""
    true = [fixed(true_camera(0)), true_camera(1), true_camera(2, free_trans=False)]
    start = [true[0], perturbed(true[1], rng), perturbed(true[2], rng)]
    start[2].Et = true[2].Et
    blind = {4: [2], 17: [2], 32: [2]} if blind is None else blind
    return true, start, make_instants([0, 1, 2], robot_poses(n, rng), rng, noise_px=noise_px, blind=blind)


def eight_camera_case(rng, n, noise_px=0.0, blind=None):
    """Mounts 0..3 twice; camera 0 fixed, camera 5 free_rot only, camera 6 free_trans only (each
    starts at the truth in what it holds fixed)."""
    mounts = [0, 1, 2, 3, 0, 1, 2, 3]
    true = [true_camera(k) for k in mounts]
    true[0] = fixed(true[0])
    true[5].free_trans = False
    true[6].free_rot = False
    start = [true[0]] + [perturbed(c, rng) for c in true[1:]]
    start[5].Et = true[5].Et
    start[6].ER = true[6].ER
    return true, start, make_instants(mounts, robot_poses(n, rng), rng, noise_px=noise_px, blind=blind)


def never_shared_case():
    """Camera 2 is free and sees nothing in any instant."""
    rng = np.random.default_rng(31)
    true = [fixed(true_camera(0)), true_camera(1), true_camera(2)]
    start = [true[0], perturbed(true[1], rng), perturbed(true[2], rng)]
    return start, make_instants([0, 1, 2], robot_poses(4, rng), rng, blind={i: [2] for i in range(4)})


def accept_reject_case():
    """2 cameras x 6 noisy instants: the solve converges in a few accepted steps, after which the
    cost no longer falls and the remaining iterations are rejected (the twin alone shows both
    counts positive: tests/test_rig_calib_host.py)."""
    rng = np.random.default_rng(41)
    _true, start, instants = two_camera_case(rng, 6, noise_px=0.3)
    return start, instants


# ---- rendered instants for the end-to-end GPU test --------------------------------------------------
# The rig of rig_pose_cases' views "front", "right" and "left" (their mounts on RENDER_ROBOT) at
# robot poses near RENDER_ROBOT: every drawn tag stays inside the 640 x 480 frame (asserted).
E2E_VIEWS = ("front", "right", "left")
E2E_ROBOTS = [rc.RENDER_ROBOT,
              (fc.rot_xyz(1.06, -3.46, -0.03), rc.RENDER_ROBOT[1] + np.array([-0.036, -0.025, -0.019])),
              (fc.rot_xyz(2.42, -3.24, 1.45), rc.RENDER_ROBOT[1] + np.array([-0.012, -0.013, -0.035])),
              (fc.rot_xyz(0.19, -3.31, 1.12), rc.RENDER_ROBOT[1] + np.array([-0.005, -0.038, -0.028])),
              (fc.rot_xyz(2.36, -3.27, 1.21), rc.RENDER_ROBOT[1] + np.array([-0.04, -0.005, 0.017]))]


def render_mounted_view(name, robot, draw_tag, codes, blank):
    """gray uint8 [480, 640] of view `name`'s camera, mounted as on RENDER_ROBOT, with the robot at
    `robot` -- drawn as rig_pose_cases.render_view draws."""
    ids, _c, _rx, _ry, _rz, cam = rc.VIEWS[name]
    R, t = rc.camera_in_field(*robot, *rc.view_mount(name))
    img = blank()
    where = {g[0]: g for g in rc.RIG_LAYOUT}
    for tid in ids:
        _tid, Rt, tt = where[tid]
        px, z = fc.project(cam, R, t, fc.tag_corners_field(Rt, tt, rc.TAG_SIZE, fc.QUIET))
        assert (z > 0).all() and px.min() >= 0 and (px[:, 0] <= 639).all() and (px[:, 1] <= 479).all(), (name, tid)
        draw_tag(img, codes[tid], px[[3, 2, 1, 0]])               # draw_tag takes TL, TR, BR, BL
    return img


# ---- the algorithm, restated ------------------------------------------------------------------------
# Expression order is csrc/at_rigcal.h's.  A sum over a camera's corners is the 64-slot tree; U and
# g add the cameras in order; a product sum runs over ascending k; a sum over the instants runs
# ascending within chunks of 32, then over the chunks in order.
def _s6(a, g, lam):
    x = fc._solve6(a, g, lam)
    return NAN6 if x is None else x


def _chunked(vals):
    chunks = []
    for i0 in range(0, len(vals), CHUNK):
        acc = vals[i0]
        for v in vals[i0 + 1:i0 + CHUNK]:
            acc = acc + v
        chunks.append(acc)
    tot = chunks[0]
    for c in chunks[1:]:
        tot = tot + c
    return tot


def camera_rows(c, R, t, X):
    """(jpu, jpv, jcu, jcv, P): the rows of the points X of camera c for the pose (w, dt) and for
    the camera's own (we, de), E_R' = E_R dR(we), E_t' = E_t + de; columns that are not free are 0."""
    jpu, jpv, P = rc.jacobian_rows(c, R, t, X)
    xn, yn = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    A, B = c.cam.fx / P[:, 2], -(c.cam.fx * xn) / P[:, 2]
    Cc, D = c.cam.fy / P[:, 2], -(c.cam.fy * yn) / P[:, 2]
    zero = np.zeros(len(X))
    one = np.ones(len(X))
    dP = [[zero, -P[:, 2], P[:, 1], -c.ER[0, 0] * one, -c.ER[1, 0] * one, -c.ER[2, 0] * one],
          [P[:, 2], zero, -P[:, 0], -c.ER[0, 1] * one, -c.ER[1, 1] * one, -c.ER[2, 1] * one],
          [-P[:, 1], P[:, 0], zero, -c.ER[0, 2] * one, -c.ER[1, 2] * one, -c.ER[2, 2] * one]]
    jcu, jcv = [], []
    for k in range(6):
        free = c.free_rot if k < 3 else c.free_trans
        jcu.append(A * dP[0][k] + B * dP[2][k] if free else zero)
        jcv.append(Cc * dP[1][k] + D * dP[2][k] if free else zero)
    return jpu, jpv, np.stack(jcu, 1), np.stack(jcv, 1), P


def project_ext(c, R, t, X):
    return rc.project_rig(c, R, t, X)


def apply_ext(c, d):
    """The camera moved by d = (we, de); a part that is not free is copied."""
    Rn, tn = rc.apply_step(c.ER, c.Et, d)
    return SimpleNamespace(cam=c.cam, ER=Rn if c.free_rot else c.ER, Et=tn if c.free_trans else c.Et,
                           free_rot=c.free_rot, free_trans=c.free_trans)


def _cam_sums(c, R, t, X, uv):
    """U (21), g (6), V (21), h (6), W (36, row k of the pose, column b of the camera) of one camera."""
    if not len(X):
        return [0.0] * 27, [0.0] * 27, [0.0] * 36
    jpu, jpv, jcu, jcv, P = camera_rows(c, R, t, X)
    ru = (c.cam.fx * (P[:, 0] / P[:, 2]) + c.cam.cx) - uv[:, 0]
    rv = (c.cam.fy * (P[:, 1] / P[:, 2]) + c.cam.cy) - uv[:, 1]
    out = []
    for ju, jv in ((jpu, jpv), (jcu, jcv)):
        s = [fc._tree(ju[:, i] * ju[:, j] + jv[:, i] * jv[:, j]) for i, j in fc._TRI]
        out.append(s + [fc._tree(ju[:, i] * ru + jv[:, i] * rv) for i in range(6)])
    W = [fc._tree(jpu[:, k] * jcu[:, b] + jpv[:, k] * jcv[:, b]) for k in range(6) for b in range(6)]
    return out[0], out[1], W


def _tri(v):
    return {ij: v[k] for k, ij in enumerate(fc._TRI)}


def _accum(cams, pts, R, t, lam):
    """The instant's part of the reduced system [M M + 2 M] and what the back substitution needs."""
    nc, M = len(cams), 6 * len(cams)
    per = [_cam_sums(c, R, t, X, uv) for c, (X, uv) in zip(cams, pts)]
    Ug = [rc._across([p[0][k] for p in per]) for k in range(27)]
    U, g = _tri(Ug), Ug[21:]
    V = [_tri(p[1]) for p in per]
    h = [p[1][21:] for p in per]
    W = [p[2] for p in per]
    Y = []
    for c in range(nc):
        cols = [_s6(U, [-W[c][6 * k + b] for k in range(6)], lam) for b in range(6)]
        Y.append([[cols[b][k] for b in range(6)] for k in range(6)])          # Y[c][k][b]
    y = _s6(U, [-g[k] for k in range(6)], lam)
    part = np.zeros(M * M + 2 * M)
    for r in range(M):
        c, a = divmod(r, 6)
        for s in range(M):
            c2, b = divmod(s, 6)
            if c > c2:
                continue
            acc = W[c][a] * Y[c2][0][b]
            for k in range(1, 6):
                acc = acc + W[c][6 * k + a] * Y[c2][k][b]
            part[r * M + s] = (V[c][(min(a, b), max(a, b))] if c == c2 else 0.0) - acc
        acc = W[c][a] * y[0]
        for k in range(1, 6):
            acc = acc + W[c][6 * k + a] * y[k]
        part[M * M + r] = h[c][a] - acc
        part[M * M + M + r] = V[c][(a, a)]
    return part, (U, g, W)


def _reduced(tot, free, lam, damped):
    """(L, ok) of the reduced matrix; fixed parameters are identity rows."""
    M = len(free)
    A = [[0.0] * M for _ in range(M)]
    for r in range(M):
        for s in range(r, M):
            a = float(tot[r * M + s])
            if not free[r] or not free[s]:
                a = 1.0 if r == s else 0.0
            elif r == s and damped:
                a = a + lam * float(tot[M * M + M + r])
            A[r][s] = a
    L = [[0.0] * M for _ in range(M)]
    ok = True
    for j in range(M):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            ok = False
        L[j][j] = math.sqrt(s) if s >= 0.0 else math.nan
        for i in range(j + 1, M):
            v = A[j][i]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            with np.errstate(all="ignore"):
                L[i][j] = float(np.float64(v) / np.float64(L[j][j]))
    return L, ok


def _subst(L, rhs):
    M = len(rhs)
    y, x = [0.0] * M, [0.0] * M
    with np.errstate(all="ignore"):
        for i in range(M):
            v = rhs[i]
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = float(np.float64(v) / np.float64(L[i][i]))
        for i in range(M - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, M):
                v = v - L[k][i] * x[k]
            x[i] = float(np.float64(v) / np.float64(L[i][i]))
    return x


def solve_cal_ref(cams, instants, layout=rc.RIG_LAYOUT, max_hamming=0, tag_size=rc.TAG_SIZE, iters=ITERS):
    """The calibration of `cams` (initial mounts and flags) over `instants` as include/at_api.h
    defines it; instants that at_rigcal_add would not store must have been left out.  Returns a
    namespace with at_rigcal_result's fields, the per-instant records and, for the tests, cost."""
    lay = {int(tid): (np.asarray(R, np.float64), np.asarray(t, np.float64)) for tid, R, t in layout}
    nc, M, N = len(cams), 6 * len(cams), len(instants)
    free = [(c.free_rot if k < 3 else c.free_trans) for c in cams for k in range(6)]
    hs = tag_size / 2.0
    pts, poses, ntags = [], [], []
    for inst in instants:
        per = []
        for c in inst:
            X, uv = [], []
            for i in fc.select_ref(c.dets, lay, max_hamming):
                Rt, tt = lay[c.dets[i].id]
                for k, (sx, sy) in enumerate(fc.CORNER_SIGNS):
                    X.append([(Rt[r, 0] * (sx * hs) + Rt[r, 1] * (sy * hs)) + tt[r] for r in range(3)])
                    uv.append(np.asarray(c.dets[i].p, np.float64)[k])
            per.append((np.array(X).reshape(-1, 3), np.array(uv).reshape(-1, 2)))
        pts.append(per)
        start = rc.solve_rig_ref([rc.rig_camera(o.dets, o.poses, c.cam, c.ER, c.Et) for o, c in zip(inst, cams)],
                                 layout, max_hamming, tag_size)
        poses.append((start.R, start.t))
        ntags.append(start.n_tags)
    used = [n > 0 for n in ntags]

    def costs(ps, cs):
        return [rc._cost(cs, pts[i], *ps[i]) if used[i] else 0.0 for i in range(N)]

    cost0 = cost = _chunked(costs(poses, cams))
    lam, accepted, rejected = 1e-3, 0, 0
    for _ in range(iters):
        acc = [_accum(cams, pts[i], *poses[i], lam) if used[i] else (np.zeros(M * M + 2 * M), None) for i in range(N)]
        tot = _chunked([a[0] for a in acc])
        L, ok = _reduced(tot, free, lam, True)
        x = _subst(L, [-float(tot[M * M + p]) if free[p] else 0.0 for p in range(M)])
        dc = [x[p] if ok and free[p] else 0.0 for p in range(M)]
        cams_n = [apply_ext(c, dc[6 * k:6 * k + 6]) for k, c in enumerate(cams)]
        poses_n = list(poses)
        for i in range(N):
            if not used[i]:
                continue
            U, g, W = acc[i][1]
            r = []
            for k in range(6):
                a = g[k]
                for c in range(nc):
                    for b in range(6):
                        a = a + W[c][6 * k + b] * dc[6 * c + b]
                r.append(a)
            d = fc._solve6(U, r, lam)
            if d is None or not ok:
                d = [0.0] * 6
            poses_n[i] = rc.apply_step(*poses[i], d)
        cn = _chunked(costs(poses_n, cams_n))
        if ok and cn < cost:
            cams, poses, cost, accepted = cams_n, poses_n, cn, accepted + 1
            lam = max(lam / 10.0, 1e-9)
        else:
            rejected += 1
            lam = lam * 10.0
    # the covariance: the undamped reduced matrix at the final state
    acc = [_accum(cams, pts[i], *poses[i], 0.0)[0] if used[i] else np.zeros(M * M + 2 * M) for i in range(N)]
    tot = _chunked(acc)
    L, ok = _reduced(tot, free, 0.0, False)
    corners, n_used = 4 * sum(ntags), sum(used)
    den = 2 * corners - 6 * n_used - sum(free)
    valid = ok and den > 0
    cov = [np.zeros((6, 6)) for _ in range(nc)]
    if valid:
        s2 = cost / float(den)
        for p in range(M):
            w = _subst(L, [1.0 if i == p else 0.0 for i in range(M)])
            c, a = divmod(p, 6)
            for b in range(6):
                cov[c][a, b] = s2 * w[6 * c + b] if free[p] and free[6 * c + b] else 0.0
    final = costs(poses, cams)
    recs = [SimpleNamespace(R=poses[i][0], t=poses[i][1], rms_px=math.sqrt(final[i] / float(4 * ntags[i])),
                            n_tags=ntags[i], used=True) if used[i] else
            SimpleNamespace(R=np.zeros((3, 3)), t=np.zeros(3), rms_px=0.0, n_tags=0, used=False) for i in range(N)]
    return SimpleNamespace(R=[c.ER for c in cams], t=[c.Et for c in cams], cov=cov, cov_valid=valid,
                           rms_before=math.sqrt(cost0 / corners) if corners else 0.0,
                           rms_after=math.sqrt(cost / corners) if corners else 0.0, instants_used=n_used,
                           instants_skipped=N - n_used, accepted=accepted, rejected=rejected, instants=recs, cost=cost)


def same_result(a, b):
    """Every field of two calibration results (library or restatement) equal, the doubles bit for bit."""
    return (a.instants_used == b.instants_used and a.instants_skipped == b.instants_skipped
            and a.accepted == b.accepted and a.rejected == b.rejected and bool(a.cov_valid) == bool(b.cov_valid)
            and a.rms_before == b.rms_before and a.rms_after == b.rms_after and len(a.R) == len(b.R)
            and all(np.array_equal(x, y) for x, y in zip(a.R, b.R))
            and all(np.array_equal(x, y) for x, y in zip(a.t, b.t))
            and all(np.array_equal(x, y) for x, y in zip(a.cov, b.cov)))


def same_instants(a, b):
    return len(a) == len(b) and all(
        x.used == y.used and x.n_tags == y.n_tags and x.rms_px == y.rms_px and np.array_equal(x.R, y.R)
        and np.array_equal(x.t, y.t) for x, y in zip(a, b))
