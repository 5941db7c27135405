"""Scenes and the numpy restatement for the robust rig-pose tests (tests/test_rig_robust_host.py,
tests/test_rig_robust_gpu.py), over tests/rig_pose_cases.py.

The algorithm is csrc/at_rigrobust.h's: Huber cost rho(s) of each corner's squared reprojection
error s, the rig pose's Levenberg-Marquardt loop with each corner's rows of the normal equations
times its weight, then rounds that drop the tags whose (s0 + s1) + (s2 + s3) stays beyond
4 reject_px^2 and fit again.  A dropped tag's slots keep their place in the 64-slot tree and add
+0.0.  Nothing here needs the library or a GPU.
"""
import math
from types import SimpleNamespace

import numpy as np

import field_pose_cases as fc
import rig_pose_cases as rc

INF = math.inf
DEFAULT = SimpleNamespace(huber_px=2.0, reject_px=6.0, max_rounds=3, min_keep=2)
PLAIN = SimpleNamespace(huber_px=INF, reject_px=INF, max_rounds=3, min_keep=2)
SHIFT = np.array([0.25, 0.10, 0.0])      # how far a displaced layout tag is moved, metres


def cfg(**kw):
    d = dict(vars(DEFAULT))
    d.update(kw)
    return SimpleNamespace(**d)


def displaced(layout, ids, shift=SHIFT):
    """The layout with the tags `ids` moved by `shift`: what the solver is told while the scene
    is drawn from the true layout."""
    return [(tid, R, np.asarray(t, np.float64) + (shift if tid in ids else 0.0)) for tid, R, t in layout]


def without(layout, ids):
    return [g for g in layout if g[0] not in ids]


# ---- the algorithm, restated ------------------------------------------------------------------
def _sq(c, R, t, X, uv):
    """Each slot's squared reprojection error, inf with Pz <= 0 (rig_slot_cost)."""
    with np.errstate(all="ignore"):
        _Q, P = rc.points_cam(c, R, t, X)
        ru = (c.cam.fx * (P[:, 0] / P[:, 2]) + c.cam.cx) - uv[:, 0]
        rv = (c.cam.fy * (P[:, 1] / P[:, 2]) + c.cam.cy) - uv[:, 1]
        return np.where(P[:, 2] > 0.0, ru * ru + rv * rv, math.inf)


def _huber(s, k):
    """(rho, w) of rig_huber for an array s."""
    kk = k * k
    with np.errstate(all="ignore"):
        e = np.sqrt(s)
        far = ~(s <= kk)
        rho = np.where(far, (2.0 * k) * e - kk, s)
        w = np.where(far, k / e, 1.0)
    return rho, w


def _cost(cams, pts, live, R, t, k):
    parts = []
    for c, (X, uv), m in zip(cams, pts, live):
        if not len(X):
            parts.append(0.0)
            continue
        rho, _w = _huber(_sq(c, R, t, X, uv), k)
        parts.append(fc._tree(np.where(m, rho, 0.0)))
    return rc._across(parts)


def _normal(cams, pts, live, R, t, k):
    per = []
    for c, (X, uv), m in zip(cams, pts, live):
        if not len(X):
            per.append([0.0] * 27)
            continue
        with np.errstate(all="ignore"):
            ju, jv, P = rc.jacobian_rows(c, R, t, X)
            ru = (c.cam.fx * (P[:, 0] / P[:, 2]) + c.cam.cx) - uv[:, 0]
            rv = (c.cam.fy * (P[:, 1] / P[:, 2]) + c.cam.cy) - uv[:, 1]
            _rho, w = _huber(_sq(c, R, t, X, uv), k)
            vals = [(ju[:, i] * ju[:, j] + jv[:, i] * jv[:, j]) * w for i, j in fc._TRI]
            vals += [(ju[:, i] * ru + jv[:, i] * rv) * w for i in range(6)]
        per.append([fc._tree(np.where(m, v, 0.0)) for v in vals])
    v = [rc._across([p[q] for p in per]) for q in range(27)]
    return {ij: v[q] for q, ij in enumerate(fc._TRI)}, v[21:]


def _fit(cams, pts, live, R, t, cost, k):
    lam, steps, rejected = 1e-3, 0, 0
    for _ in range(rc.ITERS):
        a, g = _normal(cams, pts, live, R, t, k)
        d = fc._solve6(a, g, lam)
        take = d is not None
        if take:
            Rn, tn = rc.apply_step(R, t, d)
            cn = _cost(cams, pts, live, Rn, tn, k)
            take = cn < cost
        if take:
            R, t, cost, steps = Rn, tn, cn, steps + 1
            lam = max(lam / 10.0, 1e-9)
        else:
            rejected += 1
            lam = lam * 10.0
    return R, t, cost, steps, rejected


def _tag_sums(s):
    return (s[0::4] + s[1::4]) + (s[2::4] + s[3::4])


def solve_robust_ref(cams, layout, cfg=DEFAULT, max_hamming=0, tag_size=rc.TAG_SIZE):
    """(record, info) of one instant as include/at_api.h defines the robust rig pose; the record has
    solve_rig_ref's fields, the info at_rig_robust_info's (tag_rms_px cut to tags_per_cam)."""
    lay = {int(tid): (np.asarray(R, np.float64), np.asarray(t, np.float64)) for tid, R, t in layout}
    n_cams = len(cams)
    k = float(cfg.huber_px)
    cut = 4.0 * float(cfg.reject_px) * float(cfg.reject_px)
    sels = [fc.select_ref(c.dets, lay, max_hamming) for c in cams]
    tags_per_cam = [len(s) for s in sels] + [0] * (rc.MAX_CAMS - n_cams)
    ids = [[int(c.dets[i].id) for i in s] for c, s in zip(cams, sels)] + [[] for _ in range(rc.MAX_CAMS - n_cams)]
    n_tags = sum(tags_per_cam)
    hs = tag_size / 2.0
    pts = []
    for c, sel in zip(cams, sels):
        X, uv = [], []
        for i in sel:
            Rt, tt = lay[c.dets[i].id]
            for q, (sx, sy) in enumerate(fc.CORNER_SIGNS):
                X.append([(Rt[r, 0] * (sx * hs) + Rt[r, 1] * (sy * hs)) + tt[r] for r in range(3)])
                uv.append(np.asarray(c.dets[i].p, np.float64)[q])
        pts.append((np.array(X).reshape(-1, 3), np.array(uv).reshape(-1, 2)))
    live = [np.ones(len(X), bool) for X, _uv in pts]
    cost, R, t = math.inf, None, None
    for c, sel in zip(cams, sels):
        for i in sel:
            Rt, tt = lay[c.dets[i].id]
            Rfc = fc._mul(Rt, np.asarray(c.poses[i].R, np.float64).T)
            tfc = tt - rc._rot(Rfc, np.asarray(c.poses[i].t, np.float64))
            Rj = fc._mul(Rfc, c.ER.T)
            tj = tfc - rc._rot(Rj, c.Et)
            cj = _cost(cams, pts, live, Rj, tj, k)
            if cj < cost:
                cost, R, t = cj, Rj, tj
    if R is None:
        rec = SimpleNamespace(n_tags=0, n_cams_used=0, tags_per_cam=[0] * rc.MAX_CAMS,
                              ids=[[] for _ in range(rc.MAX_CAMS)], R=np.zeros((3, 3)), t=np.zeros(3),
                              cov=np.zeros((6, 6)), cov_valid=False, rms_px=0.0, steps_taken=0, rejected=0)
        info = SimpleNamespace(n_kept=0, n_rejected=0, rounds=0, starved=False, rejected_mask=[0] * rc.MAX_CAMS,
                               tag_rms_px=[[] for _ in range(rc.MAX_CAMS)], huber_cost=0.0, n_downweighted=0)
        return rec, info
    R = fc._project_rotation(R)
    c0 = _cost(cams, pts, live, R, t, k)
    if c0 < math.inf:
        cost = c0
    R, t, cost, steps, rejected = _fit(cams, pts, live, R, t, cost, k)
    rounds, starved, n_kept = 0, False, n_tags
    masks = [0] * rc.MAX_CAMS
    for _ in range(int(cfg.max_rounds)):
        cand, nk = [], 0
        for c, (X, uv), m in zip(cams, pts, live):
            if not len(X):
                cand.append(np.zeros(0, bool))
                continue
            s = np.where(m, _sq(c, R, t, X, uv), 0.0)
            cand.append(m[0::4] & (_tag_sums(s) > cut))
            nk += int(m[0::4].sum())
        nc = sum(int(x.sum()) for x in cand)
        if nc == 0:
            break
        if nk - nc < int(cfg.min_keep):
            starved = True
            break
        for i, x in enumerate(cand):
            live[i] = live[i] & ~np.repeat(x, 4)
            masks[i] |= sum(1 << j for j in np.flatnonzero(x))
        n_kept = nk - nc
        rounds += 1
        cost = _cost(cams, pts, live, R, t, k)
        R, t, cost, s2, r2 = _fit(cams, pts, live, R, t, cost, k)
        steps, rejected = steps + s2, rejected + r2
    ws, ss, n_down, tag_rms = [], [], 0, []
    for c, (X, uv), m in zip(cams, pts, live):
        if not len(X):
            ws.append(0.0)
            ss.append(0.0)
            tag_rms.append([])
            continue
        s = _sq(c, R, t, X, uv)
        _rho, w = _huber(s, k)
        ws.append(fc._tree(np.where(m, w * s, 0.0)))
        ss.append(fc._tree(np.where(m, s, 0.0)))
        n_down += int((m & (s > k * k)).sum())
        tag_rms.append([math.sqrt(x / 4.0) for x in _tag_sums(s)])
    sum_ws, sum_s = rc._across(ws), rc._across(ss)
    a, _g = _normal(cams, pts, live, R, t, k)
    s2 = sum_ws / float(8 * n_kept - 6)
    cov, cov_valid = np.zeros((6, 6)), True
    for q in range(6):
        x = fc._solve6(a, [-1.0 if i == q else -0.0 for i in range(6)], 0.0)
        if x is None:
            cov_valid = False
            break
        cov[q] = [s2 * x[i] for i in range(6)]
    if not cov_valid:
        cov = np.zeros((6, 6))
    rec = SimpleNamespace(n_tags=n_tags, n_cams_used=sum(1 for m in tags_per_cam if m), tags_per_cam=tags_per_cam,
                          ids=ids, R=R, t=t, cov=cov, cov_valid=cov_valid,
                          rms_px=math.sqrt(sum_s / float(4 * n_kept)), steps_taken=steps, rejected=rejected)
    info = SimpleNamespace(n_kept=n_kept, n_rejected=n_tags - n_kept, rounds=rounds, starved=starved,
                           rejected_mask=masks, tag_rms_px=tag_rms + [[] for _ in range(rc.MAX_CAMS - n_cams)],
                           huber_cost=cost, n_downweighted=n_down)
    return rec, info


def same_info(a, b):
    """Every field of two infos (library or restatement) equal, the doubles bit for bit."""
    return (a.n_kept == b.n_kept and a.n_rejected == b.n_rejected and a.rounds == b.rounds
            and bool(a.starved) == bool(b.starved) and list(a.rejected_mask) == list(b.rejected_mask)
            and [list(x) for x in a.tag_rms_px] == [list(x) for x in b.tag_rms_px]
            and a.huber_cost == b.huber_cost and a.n_downweighted == b.n_downweighted)


def dropped_views(info, rec):
    """[(camera, id)] of the views the info marks dropped."""
    return [(c, rec.ids[c][j]) for c in range(rc.MAX_CAMS) for j in range(len(rec.ids[c]))
            if info.rejected_mask[c] >> j & 1]


# ---- scenes -------------------------------------------------------------------------------------
# (mounts, displaced ids): the displaced-tag scenes; every camera that sees a displaced tag has a
# view of it to drop
SCENES = {
    "tag4_3cams": ([0, 1, 2], {4}),
    "tag0_3cams": ([0, 1, 2], {0}),          # seen by mounts 0 and 2: two views
    "tags46_3cams": ([0, 1, 2], {4, 6}),
    "tags14_4cams": ([0, 1, 2, 3], {1, 4}),
    "tag1_1cam": ([0], {1}),
    "tag4_2cams": ([0, 1], {4}),
}


def bad_views(mounts, bad):
    return sorted((i, tid) for i, k in enumerate(mounts) for tid in rc.mount(k)[0] if tid in bad)
