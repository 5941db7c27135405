"""Scenes and the numpy restatement for the rig-track tests (tests/test_rig_track_host.py,
tests/test_rig_track_gpu.py).

Built on tests/rig_pose_cases.py (mounts, layout, make_instant, the restated rig pose: an instant's
own start); the GPU tests take their rendered instants from tests/rig_calib_cases.py.  A tracker
camera is (intrinsics, ER, Et);
an instant is a namespace of make_instant's rig cameras, its odometry (R, t, sigma_rot, sigma_trans)
since the previous instant -- the robot now in the previous robot frame, x_prev = R x_now + t; None:
a new chain -- and a stamp.  Nothing here needs the library or a GPU.
"""
import math
from types import SimpleNamespace

import numpy as np

import field_pose_cases as fc
import rig_pose_cases as rc

MAX_WINDOW = 64
SIGMA_ROT = 0.004      # rad per step: a drivetrain gyro over one frame interval, generously
SIGMA_TRANS = 0.004    # m per step


# ---- scenes ---------------------------------------------------------------------------------------
def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def cameras(mounts):
    """The tracker cameras of MOUNTS[k] for k in mounts."""
    out = []
    for k in mounts:
        _ids, ER, Et, cam = rc.mount(k)
        out.append(SimpleNamespace(cam=cam, ER=ER, Et=Et))
    return out


def odom_between(a, b, rng=None, sigma_rot=SIGMA_ROT, sigma_trans=SIGMA_TRANS, noisy=False):
    """The odometry from robot pose a to robot pose b, with Gaussian noise of the stated sigmas when noisy."""
    R, t = a[0].T @ b[0], a[0].T @ (b[1] - a[1])
    if noisy:
        R, t = R @ rodrigues(rng.normal(scale=sigma_rot, size=3)), t + rng.normal(scale=sigma_trans, size=3)
    return (R, t, sigma_rot, sigma_trans)


def make_window(mounts, robots, rng, noise_px=0.0, tagless=(), blind=None, noisy_odom=False, sigma_rot=SIGMA_ROT,
                sigma_trans=SIGMA_TRANS, layout=None, **kw):
    """One instant per robot pose; `tagless` instants see nothing in any camera; blind = {instant:
    [cameras that see nothing]} ("foreign" entries of a mounts list work as in make_instant)."""
    out = []
    for i, robot in enumerate(robots):
        ms = [None if (i in tagless or c in (blind or {}).get(i, ())) else k for c, k in enumerate(mounts)]
        cams = rc.make_instant(ms, rng, robot=robot, noise_px=noise_px, layout=layout, **kw)
        od = None if i == 0 else odom_between(robots[i - 1], robot, rng, sigma_rot, sigma_trans, noisy_odom)
        out.append(SimpleNamespace(cams=cams, odom=od, stamp=100.0 + 0.02 * i, robot=robot))
    return out


def as_create_args(cams):
    """The `cameras` argument of ros_vision_amd.RigTracker."""
    return [(c.cam, (c.ER, c.Et)) for c in cams]


def push(trk, inst):
    return trk.push([(c.dets, c.poses) for c in inst.cams], inst.odom, inst.stamp)


def tracker(rva, cams, instants, layout=rc.RIG_LAYOUT, **kw):
    """A RigTracker over cams with `instants` pushed (the window is their number unless given)."""
    kw.setdefault("window", max(2, len(instants)))
    trk = rva.RigTracker(as_create_args(cams), layout, **kw)
    for inst in instants:
        push(trk, inst)
    return trk


def walk(n, rng, turn_deg=1.5, move_m=0.03):
    """n robot poses near rig_pose_cases.ROBOT, each a small step from the one before, pulled back
    towards ROBOT so that every mount keeps its tags in front."""
    R, t = rc.ROBOT
    out = []
    for _ in range(n):
        R = fc.small_rotation(rng, turn_deg) @ R
        t = rc.ROBOT[1] + 0.8 * (t - rc.ROBOT[1]) + rng.uniform(-move_m, move_m, 3)
        if np.degrees(np.arccos(np.clip((np.trace(rc.ROBOT[0].T @ R) - 1) / 2, -1, 1))) > 6.0:
            R = rc.ROBOT[0]
        out.append((R, t))
    return out


# One camera and one far tag: the layout's tag 1 pushed back along the camera's view, for the
# smoothing test.  The rig pose of such an instant scatters by centimetres.
FAR_LAYOUT = [fc.wall_a(1, -0.05, 0.14)]
FAR_ROBOT = (fc.rot_xyz(2.0, -3.0, 1.5), np.array([0.03, 0.02, -4.2]))
FAR_CAM = SimpleNamespace(cam=rc.CAM_A, ER=fc.rot_xyz(-1.0, 1.0, 0.5).T, Et=np.array([0.02, -0.02, 0.0]))


def far_walk(n, rng):
    R, t = FAR_ROBOT
    out = []
    for _ in range(n):
        R = fc.small_rotation(rng, 0.5) @ R
        t = t + rng.uniform(-0.02, 0.02, 3)
        out.append((R, t))
    return out


def far_window(robots, rng, noise_px=0.3, sigma_rot=0.002, sigma_trans=0.003):
    out = []
    for i, robot in enumerate(robots):
        Rc, tc = rc.camera_in_field(*robot, FAR_CAM.ER, FAR_CAM.Et)
        dets, poses = fc.make_frame(FAR_LAYOUT, Rc, tc, rng, cam=FAR_CAM.cam, noise_px=noise_px, pose_rot_deg=1.0,
                                    pose_t_m=0.02)
        od = None if i == 0 else odom_between(robots[i - 1], robot, rng, sigma_rot, sigma_trans, True)
        out.append(SimpleNamespace(cams=[rc.rig_camera(dets, poses, FAR_CAM.cam, FAR_CAM.ER, FAR_CAM.Et)], odom=od,
                                   stamp=0.02 * i, robot=robot))
    return out


def accept_reject_case():
    """2 cameras x 6 noisy instants with noisy odometry: a few accepted steps, after which the cost no
    longer falls and the remaining iterations are rejected (the twin alone shows both counts
    positive: tests/test_rig_track_host.py)."""
    rng = np.random.default_rng(41)
    return cameras([0, 1]), make_window([0, 1], walk(6, rng), rng, noise_px=0.3, noisy_odom=True)


def pose_error(a, b):
    """(angle in rad, distance in m) between robot poses a and b."""
    c = (np.trace(a[0].T @ b[0]) - 1.0) / 2.0
    return math.acos(max(-1.0, min(1.0, c))), float(np.linalg.norm(a[1] - b[1]))


# ---- the algorithm, restated ------------------------------------------------------------------------
# Expression order is csrc/at_rigtrack.h's.  A sum over a camera's corners is the 64-slot tree, the
# cameras are added in order (rig_pose_cases._normal, _cost); a product sum over the six rows of an
# odometry factor and every sum of the block solve runs ascending; the total cost adds the instants
# ascending.
def _mul_atb(a, b):
    return np.array([[(a[0, r] * b[0, k] + a[1, r] * b[1, k]) + a[2, r] * b[2, k] for k in range(3)] for r in range(3)])


def _mul_abt(a, b):
    return np.array([[(a[r, 0] * b[k, 0] + a[r, 1] * b[k, 1]) + a[r, 2] * b[k, 2] for k in range(3)] for r in range(3)])


def forward(a, od):
    rt = rc._rot(a[0], od[1])
    return fc._mul(a[0], np.asarray(od[0], np.float64)), np.array([rt[k] + a[1][k] for k in range(3)])


def backward(b, od):
    Rn = _mul_abt(b[0], np.asarray(od[0], np.float64))
    rt = rc._rot(Rn, od[1])
    return Rn, np.array([b[1][k] - rt[k] for k in range(3)])


def odom_rows(a, b, od):
    """(r [6], Ja [6][6], Jb [6][6]) of the odometry factor between poses a and b: residual rows
    (rotation, translation), columns (w, dt) of a and of b."""
    Ra, ta = a
    Rb, tb = b
    Rm, tm, sr, st = np.asarray(od[0], np.float64), np.asarray(od[1], np.float64), float(od[2]), float(od[3])
    E = _mul_atb(Rm, _mul_atb(Ra, Rb))
    e = E.reshape(9)
    r = [(0.5 * (e[7] - e[5])) / sr, (0.5 * (e[2] - e[6])) / sr, (0.5 * (e[3] - e[1])) / sr]
    d = [tb[k] - ta[k] for k in range(3)]
    q = [(Ra[0, k] * d[0] + Ra[1, k] * d[1]) + Ra[2, k] * d[2] for k in range(3)]
    r += [(q[k] - tm[k]) / st for k in range(3)]
    tr = (e[0] + e[4]) + e[8]
    G = np.array([[(tr if i == j else 0.0) - E[i, j] for j in range(3)] for i in range(3)])
    H = _mul_abt(G, Rm)
    Ja = [[0.0] * 6 for _ in range(6)]
    Jb = [[0.0] * 6 for _ in range(6)]
    for i in range(3):
        for j in range(3):
            Ja[i][j] = (-0.5 * H[i, j]) / sr
            Jb[i][j] = (0.5 * ((tr if i == j else 0.0) - E[j, i])) / sr
            Ja[3 + i][3 + j] = -Ra[j, i] / st
            Jb[3 + i][3 + j] = Ra[j, i] / st
    Ja[3][1], Ja[3][2] = -q[2] / st, q[1] / st
    Ja[4][0], Ja[4][2] = q[2] / st, -q[0] / st
    Ja[5][0], Ja[5][1] = -q[1] / st, q[0] / st
    return [float(x) for x in r], [[float(x) for x in row] for row in Ja], [[float(x) for x in row] for row in Jb]


def odom_residual(a, b, od):
    return np.array(odom_rows(a, b, od)[0])


def _col_dot(x, a, y, b):
    acc = x[0][a] * y[0][b]
    for i in range(1, 6):
        acc = acc + x[i][a] * y[i][b]
    return acc


def _factor(a, b, od):
    r, Ja, Jb = odom_rows(a, b, od)
    Da = [[_col_dot(Ja, i, Ja, j) for j in range(6)] for i in range(6)]
    Db = [[_col_dot(Jb, i, Jb, j) for j in range(6)] for i in range(6)]
    O = [[_col_dot(Jb, i, Ja, j) for j in range(6)] for i in range(6)]
    ga, gb = [], []
    for i in range(6):
        va, vb = Ja[0][i] * r[0], Jb[0][i] * r[0]
        for q in range(1, 6):
            va, vb = va + Ja[q][i] * r[q], vb + Jb[q][i] * r[q]
        ga.append(va)
        gb.append(vb)
    odo = r[0] * r[0]
    for q in range(1, 6):
        odo = odo + r[q] * r[q]
    return SimpleNamespace(Da=Da, Db=Db, O=O, ga=ga, gb=gb, odo=odo)


def _sums(cams, pts, ntags, odoms, poses):
    """Per instant (U, g, px) -- None without tags -- and the factor to its predecessor."""
    vis, fac = [], [None]
    for k, (R, t) in enumerate(poses):
        if ntags[k] > 0:
            with np.errstate(all="ignore"):
                U, g = rc._normal(cams, pts[k], R, t)
            vis.append((U, g, rc._cost(cams, pts[k], R, t)))
        else:
            vis.append(None)
        if k >= 1:
            fac.append(_factor(poses[k - 1], poses[k], odoms[k]))
    return vis, fac


def _total(vis, fac, wpx):
    cn = wpx * (vis[0][2] if vis[0] else 0.0)
    px = vis[0][2] if vis[0] else 0.0
    for k in range(1, len(vis)):
        pk = vis[k][2] if vis[k] else 0.0
        cn = cn + (wpx * pk + fac[k].odo)
        px = px + pk
    return cn, px


def _block_solve(vis, fac, wpx, lam):
    """(L blocks, their diagonals' reciprocals, B blocks, x steps, ok) of the block-tridiagonal system;
    nothing after a failed pivot.  Every division by a diagonal entry of L is a product with its
    reciprocal, formed once per column."""
    N = len(vis)
    D, rhs = [], []
    for k in range(N):
        Dk = [[0.0] * 6 for _ in range(6)]
        for r in range(6):
            for c in range(6):
                v = wpx * vis[k][0][(min(r, c), max(r, c))] if vis[k] else 0.0
                if k >= 1:
                    v = v + fac[k].Db[r][c]
                if k + 1 < N:
                    v = v + fac[k + 1].Da[r][c]
                if r == c:
                    v = v + lam * v
                Dk[r][c] = v
        D.append(Dk)
        gk = []
        for a in range(6):
            v = wpx * vis[k][1][a] if vis[k] else 0.0
            if k >= 1:
                v = v + fac[k].gb[a]
            if k + 1 < N:
                v = v + fac[k + 1].ga[a]
            gk.append(-v)
        rhs.append(gk)
    Ls, Bs, Is = [], [None], []
    for k in range(N):
        if k >= 1:
            Lp = Ls[k - 1]
            B = [list(row) for row in fac[k].O]
            for r in range(6):
                for c in range(6):
                    v = B[r][c]
                    for m in range(c):
                        v = v - B[r][m] * Lp[c][m]
                    B[r][c] = v * Is[k - 1][c]
            Bs.append(B)
            for i in range(6):
                for j in range(6):
                    acc = B[i][0] * B[j][0]
                    for m in range(1, 6):
                        acc = acc + B[i][m] * B[j][m]
                    D[k][i][j] = D[k][i][j] - acc
        L = [[0.0] * 6 for _ in range(6)]
        inv = [0.0] * 6
        for j in range(6):
            s = D[k][j][j]
            for m in range(j):
                s = s - L[j][m] * L[j][m]
            if not s > 0.0:
                return None, None, None, None, False
            L[j][j] = math.sqrt(s)
            inv[j] = 1.0 / L[j][j]
            for i in range(j + 1, 6):
                v = D[k][i][j]
                for m in range(j):
                    v = v - L[i][m] * L[j][m]
                L[i][j] = v * inv[j]
        Ls.append(L)
        Is.append(inv)
    y = []
    for k in range(N):
        yk = list(rhs[k])
        for i in range(6):
            v = yk[i]
            if k >= 1:
                acc = Bs[k][i][0] * y[k - 1][0]
                for m in range(1, 6):
                    acc = acc + Bs[k][i][m] * y[k - 1][m]
                v = v - acc
            for m in range(i):
                v = v - Ls[k][i][m] * yk[m]
            yk[i] = v * Is[k][i]
        y.append(yk)
    x = [None] * N
    for k in range(N - 1, -1, -1):
        xk = list(y[k])
        for i in range(5, -1, -1):
            v = xk[i]
            if k + 1 < N:
                acc = Bs[k + 1][0][i] * x[k + 1][0]
                for m in range(1, 6):
                    acc = acc + Bs[k + 1][m][i] * x[k + 1][m]
                v = v - acc
            for m in range(i + 1, 6):
                v = v - Ls[k][m][i] * xk[m]
            xk[i] = v * Is[k][i]
        x[k] = xk
    return Ls, Is, Bs, x, True


def window_points(cams, window, layout, max_hamming, tag_size):
    """Per instant and camera (X [n, 3], uv [n, 2]) of the selected tags' corners."""
    lay = {int(tid): (np.asarray(R, np.float64), np.asarray(t, np.float64)) for tid, R, t in layout}
    hs = tag_size / 2.0
    pts = []
    for inst in window:
        per = []
        for c in inst.cams:
            X, uv = [], []
            for i in fc.select_ref(c.dets, lay, max_hamming):
                Rt, tt = lay[c.dets[i].id]
                for k, (sx, sy) in enumerate(fc.CORNER_SIGNS):
                    X.append([(Rt[r, 0] * (sx * hs) + Rt[r, 1] * (sy * hs)) + tt[r] for r in range(3)])
                    uv.append(np.asarray(c.dets[i].p, np.float64)[k])
            per.append((np.array(X).reshape(-1, 3), np.array(uv).reshape(-1, 2)))
        pts.append(per)
    return pts


def start_poses(cams, window, layout=rc.RIG_LAYOUT, max_hamming=0, tag_size=rc.TAG_SIZE):
    """(poses, ntags): every instant's start -- its own rig pose, or its neighbour's start moved by the
    odometry -- or (None, ntags) when no instant has one."""
    own, ntags = [], []
    for inst in window:
        s = rc.solve_rig_ref([rc.rig_camera(o.dets, o.poses, c.cam, c.ER, c.Et) for o, c in zip(inst.cams, cams)],
                             layout, max_hamming, tag_size)
        own.append((s.R, s.t))
        ntags.append(s.n_tags)
    k0 = next((k for k, n in enumerate(ntags) if n > 0), None)
    if k0 is None:
        return None, ntags
    poses = [None] * len(window)
    poses[k0] = own[k0]
    for k in range(k0 + 1, len(window)):
        poses[k] = own[k] if ntags[k] > 0 else forward(poses[k - 1], window[k].odom)
    for k in range(k0 - 1, -1, -1):
        poses[k] = backward(poses[k + 1], window[k + 1].odom)
    return poses, ntags


def solve_track_ref(cams, window, layout=rc.RIG_LAYOUT, max_hamming=0, tag_size=rc.TAG_SIZE, sigma_px=0.5, iters=6):
    """The track over `window` (one chain: window[0].odom is ignored) as include/at_api.h defines it.
    Returns a namespace with at_rigtrack_result's fields and the per-instant records, or None for a
    window without a start."""
    N = len(window)
    pts = window_points(cams, window, layout, max_hamming, tag_size)
    poses, ntags = start_poses(cams, window, layout, max_hamming, tag_size)
    if poses is None:
        return None
    odoms = [w.odom for w in window]
    wpx = 1.0 / (sigma_px * sigma_px)
    vis, fac = _sums(cams, pts, ntags, odoms, poses)
    cost, px = _total(vis, fac, wpx)
    cost0, px0 = cost, px
    lam, accepted, rejected = 1e-3, 0, 0
    for _ in range(iters):
        _L, _I, _B, x, ok = _block_solve(vis, fac, wpx, lam)
        take = ok
        if ok:
            poses_n = [rc.apply_step(*poses[k], x[k]) for k in range(N)]
            vis_n, fac_n = _sums(cams, pts, ntags, odoms, poses_n)
            cn, pxn = _total(vis_n, fac_n, wpx)
            take = cn < cost
        if take:
            poses, vis, fac, cost, px, accepted = poses_n, vis_n, fac_n, cn, pxn, accepted + 1
            lam = max(lam / 10.0, 1e-9)
        else:
            rejected += 1
            lam = lam * 10.0
    Ls, Is, _B, _x, ok = _block_solve(vis, fac, wpx, 0.0)
    cov = np.zeros((6, 6))
    if ok:
        L, inv = Ls[N - 1], Is[N - 1]
        for p in range(6):
            w = [0.0] * 6
            for i in range(6):
                v = 1.0 if i == p else 0.0
                for m in range(i):
                    v = v - L[i][m] * w[m]
                w[i] = v * inv[i]
            for i in range(5, -1, -1):
                v = w[i]
                for m in range(i + 1, 6):
                    v = v - L[m][i] * w[m]
                w[i] = v * inv[i]
            cov[p] = w
    corners = 4 * sum(n for n in ntags if n > 0)
    recs = [SimpleNamespace(R=poses[k][0], t=poses[k][1], stamp=window[k].stamp, n_tags=max(ntags[k], 0),
                            rms_px=math.sqrt(vis[k][2] / float(4 * ntags[k])) if ntags[k] > 0 else 0.0)
            for k in range(N)]
    return SimpleNamespace(R=poses[-1][0], t=poses[-1][1], cov=cov, cov_valid=ok, stamp=window[-1].stamp, n=N,
                           with_tags=sum(1 for n in ntags if n > 0), accepted=accepted, rejected=rejected,
                           cost_before=cost0, cost_after=cost,
                           rms_before=math.sqrt(px0 / float(corners)) if corners else 0.0,
                           rms_after=math.sqrt(px / float(corners)) if corners else 0.0, instants=recs)


def same_result(a, b):
    """Every field of two track results (library or restatement) equal, the doubles bit for bit."""
    return (a.n == b.n and a.with_tags == b.with_tags and a.accepted == b.accepted and a.rejected == b.rejected
            and bool(a.cov_valid) == bool(b.cov_valid) and a.cost_before == b.cost_before
            and a.cost_after == b.cost_after and a.rms_before == b.rms_before and a.rms_after == b.rms_after
            and a.stamp == b.stamp and np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t)
            and np.array_equal(a.cov, b.cov))


def same_instants(a, b):
    return len(a) == len(b) and all(
        x.n_tags == y.n_tags and x.rms_px == y.rms_px and x.stamp == y.stamp and np.array_equal(x.R, y.R)
        and np.array_equal(x.t, y.t) for x, y in zip(a, b))
