"""Scenes and the numpy restatement for the field-map tests (tests/test_field_map_host.py,
tests/test_field_map_gpu.py).

Built on tests/field_pose_cases.py: its walls, make_frame and the restated field pose (a view's
start).  A map tag is (id, R, t, free_rot, free_trans) with R = None for a tag without a start; a
view is (detections, poses, camera).  Nothing here needs the library or a GPU.
"""
import math
from types import SimpleNamespace

import numpy as np

import field_pose_cases as fc

ITERS = 16
CHUNK = 32
MAX_TAGS = 32
MAX_VIEWS = 4096
CAM2 = SimpleNamespace(fx=880.0, fy=885.0, cx=640.0, cy=360.0)   # a second calibrated camera


# ---- scenes ---------------------------------------------------------------------------------------
def field(n, rng=None):
    """n tags on the two walls of field_pose_cases, ids 0, 3, 6, ...: wall A a 4-column grid 0.45 m
    apart, every third tag on wall B behind it."""
    out = []
    for k in range(n):
        col, row = k % 4, k // 4
        x, y = -0.7 + 0.45 * col, -0.5 + 0.33 * row
        out.append(fc.wall_b(3 * k, x + 0.1, y, -0.25) if k % 3 == 2 else fc.wall_a(3 * k, x, y))
    return out


def map_tags(truth, rng, anchors=(0,), rot_deg=3.0, move_m=0.03, unknown=(), free=None):
    """The `tags` argument of FieldMapper: the anchors (indices into truth) fixed at the truth, the
    tags in `unknown` without a start, the others free and started rot_deg / move_m off the truth.
    free = {index: (free_rot, free_trans)} overrides a tag's flags; what it holds fixed starts at
    the truth."""
    out = []
    for k, (tid, R, t) in enumerate(truth):
        fr, ft = (free or {}).get(k, (k not in anchors, k not in anchors))
        if k in unknown:
            out.append((tid, None, None, fr, ft))
            continue
        d = rng.normal(size=3)
        Rs = R @ fc.small_rotation(rng, rot_deg) if fr else R
        ts = t + move_m * d / np.linalg.norm(d) if ft else t
        out.append((tid, Rs, ts, fr, ft))
    return out


def make_views(truth, n, rng, noise_px=0.0, subsets=None, cams=(fc.CAM,), pose_rot_deg=3.0, pose_t_m=0.03):
    """n views of the field from random cameras; subsets[i] (indices into truth) is what view i
    sees, all of it by default; the cameras' intrinsics are taken in turn."""
    out = []
    for i in range(n):
        seen = truth if subsets is None else [truth[k] for k in subsets[i % len(subsets)]]
        R, t = fc.random_camera(rng)
        cam = cams[i % len(cams)]
        dets, poses = fc.make_frame(seen, R, t, rng, cam=cam, noise_px=noise_px, pose_rot_deg=pose_rot_deg,
                                    pose_t_m=pose_t_m)
        out.append((dets, poses, cam))
    return out


def views_from(truth, cam_poses, rng, noise_px=0.0, cam=fc.CAM):
    """One view of all of truth per given camera pose (R, t): the same geometry at every call, the
    noise drawn anew."""
    return [fc.make_frame(truth, R, t, rng, cam=cam, noise_px=noise_px) + (cam,) for R, t in cam_poses]


def mapper(rva, tags, views, **kw):
    """A FieldMapper over tags holding the views it stores, and those views."""
    m = rva.FieldMapper(tags, **kw)
    kept = [v for v in views if m.add(v[0], v[1], rva.CameraMatrix(fx=v[2].fx, cx=v[2].cx, fy=v[2].fy, cy=v[2].cy))]
    assert len(m) == len(kept)
    return m, kept


def chain_case(rng, noise_px=0.0):
    """Tag C (id 6) is seen only with B (id 3), B only with the anchor A (id 0); tags 9 and 12 are
    seen only with each other: nothing placed reaches them."""
    truth = field(5)
    tags = map_tags(truth, rng, unknown=(1, 2, 3, 4))
    views = make_views(truth, 9, rng, noise_px=noise_px, subsets=[(0, 1), (1, 2), (3, 4)])
    return truth, tags, views


def floating_case(rng, noise_px=0.3):
    """Tags 9 and 12 have a start and are free, but no view holds one of them together with a tag
    of the anchored part: a component of the map without a fixed tag."""
    truth = field(5)
    tags = map_tags(truth, rng)
    views = make_views(truth, 8, rng, noise_px=noise_px, subsets=[(0, 1, 2), (3, 4)])
    return truth, tags, views


def windows_case(rng, noise_px=0.3):
    """32 tags (the cap) in 9 views of 16 each, windows 0..15, 2..17, .. 16..31 of the map; view 4 is
    offered a 17th tag, which the selection drops."""
    truth = field(32)
    tags = map_tags(truth, rng)
    subsets = [tuple(range(2 * k, 2 * k + 16)) for k in range(9)]
    subsets[4] = subsets[4] + (31,)
    return truth, tags, make_views(truth, 9, rng, noise_px=noise_px, subsets=subsets)


def behind(view):
    """The view with every tag's own pose mirrored to behind the camera: the start rule finds no
    camera pose with the corners in front, so the view is stored but takes no part."""
    dets, poses, cam = view
    return dets, [SimpleNamespace(id=p.id, R=p.R, t=-np.asarray(p.t), err=p.err) for p in poses], cam


def snapshot(m):
    """The records of the mapper's last solve, byte for byte."""
    tb, tn = m.tag_records()
    vb, vn = m.view_records()
    return bytes(m.record), bytes(tb)[:tn * (len(bytes(tb)) // max(1, len(tb)))], bytes(vb)[:vn * (len(bytes(vb)) // max(1, len(vb)))]


def position_errors(truth, recs):
    """Per placed tag the distance in metres of its start and of its final position from the truth."""
    return [(float(np.linalg.norm(q.t0 - g[2])), float(np.linalg.norm(q.t - g[2]))) for g, q in zip(truth, recs) if q.placed]


# ---- the algorithm, restated ------------------------------------------------------------------------
# at_fieldmap.h in plain float64 without contraction, every sum in the header's order: the records
# are the library's bit for bit.
_TRI = fc._TRI
_tri = {ij: k for k, ij in enumerate(_TRI)}


def _quad(v):
    return (v[0] + v[2]) + (v[1] + v[3])


def _point(tg, sx, sy, R, t):
    X = [(tg[0][k][0] * sx + tg[0][k][1] * sy) + tg[1][k] for k in range(3)]
    Q = [(R[r][0] * X[0] + R[r][1] * X[1]) + R[r][2] * X[2] for r in range(3)]
    return Q, [Q[k] + t[k] for k in range(3)]


def _slot_cost(cam, tg, sx, sy, uv, R, t):
    _Q, P = _point(tg, sx, sy, R, t)
    if not P[2] > 0.0:
        return math.inf
    ru = (cam.fx * (P[0] / P[2]) + cam.cx) - uv[0]
    rv = (cam.fy * (P[1] / P[2]) + cam.cy) - uv[1]
    return ru * ru + rv * rv


def _slot_rows(cam, tg, sx, sy, uv, R, t, fr, ft):
    Q, P = _point(tg, sx, sy, R, t)
    xn, yn = P[0] / P[2], P[1] / P[2]
    ru = (cam.fx * xn + cam.cx) - uv[0]
    rv = (cam.fy * yn + cam.cy) - uv[1]
    A, B = cam.fx / P[2], -(cam.fx * xn) / P[2]
    Cc, D = cam.fy / P[2], -(cam.fy * yn) / P[2]
    jpu = [B * Q[1], A * Q[2] - B * Q[0], -(A * Q[1]), A, 0.0, B]
    jpv = [D * Q[1] - Cc * Q[2], -(D * Q[0]), Cc * Q[0], 0.0, Cc, D]
    G = fc._mul(np.asarray(R), np.asarray(tg[0]))
    dP = [[sy * G[r][2], -(sx * G[r][2]), sx * G[r][1] - sy * G[r][0], R[r][0], R[r][1], R[r][2]] for r in range(3)]
    jtu = [(A * dP[0][c] + B * dP[2][c]) if (fr if c < 3 else ft) else 0.0 for c in range(6)]
    jtv = [(Cc * dP[1][c] + D * dP[2][c]) if (fr if c < 3 else ft) else 0.0 for c in range(6)]
    return jpu, jpv, jtu, jtv, ru, rv


def _step_R(d):
    h = [0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]
    n = math.sqrt(1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]))
    return fc._quat_to_R(1.0 / n, h[0] / n, h[1] / n, h[2] / n)


def _solve6(U, rhs, lam):
    x = fc._solve6({ij: U[k] for k, ij in enumerate(_TRI)}, rhs, lam)
    assert x is not None
    return x


def stored_views(tags, views, max_hamming=0):
    """What at_fieldmap_add keeps of each view: (dets, poses, cam) of the selection, or None."""
    ids = {int(g[0]) for g in tags}
    out = []
    for dets, poses, cam in views:
        sel = fc.select_ref(dets, ids, max_hamming)
        out.append(([dets[i] for i in sel], [poses[i] for i in sel], cam) if len(sel) >= 2 else None)
    return out


def solve_ref(tags, views, start, placed, tag_size=fc.TAG_SIZE, iters=ITERS):
    """The field map as at_fieldmap.h defines it, given the start poses (R0, t0 per tag) and which
    tags are placed.  views: the stored ones.  Returns the result, per-tag and per-view records."""
    T, N = len(tags), len(views)
    idx = {int(g[0]): J for J, g in enumerate(tags)}
    hs = tag_size / 2.0
    signs = [(-hs if c in (0, 3) else hs, hs if c < 2 else -hs) for c in range(4)]
    seen = [0] * T
    for dets, _p, _c in views:
        for d in dets:
            seen[idx[d.id]] += 1
    free = [bool(placed[J] and (tags[J][3] if a < 3 else tags[J][4]) and seen[J] > 0) for J in range(T) for a in range(6)]
    tag = [[(np.asarray(start[J][0], np.float64).tolist(), [float(x) for x in start[J][1]]) for J in range(T)]] * 2
    tag = [list(tag[0]), list(tag[0])]
    layout = [(tags[J][0], np.asarray(start[J][0]), np.asarray(start[J][1])) for J in range(T) if placed[J]]
    # start
    pose = [[None] * N, [None] * N]
    ntags = [0] * N
    for i, (dets, poses, cam) in enumerate(views):
        r = fc.solve_ref(dets, poses, layout, cam=cam, tag_size=tag_size)
        ntags[i] = r.n_tags
        pose[0][i] = pose[1][i] = (np.asarray(r.R).tolist(), [float(x) for x in r.t])

    def slot_tag(i, j):
        dets = views[i][0]
        return idx[dets[j].id] if j < len(dets) and placed[idx[dets[j].id]] else -1

    def view_cost(i, st, ps):
        dets, _p, cam = views[i]
        e = [0.0] * 64
        for j in range(len(dets)):
            J = slot_tag(i, j)
            if J < 0:
                continue
            for c in range(4):
                e[4 * j + c] = _slot_cost(cam, tag[st][J], signs[c][0], signs[c][1], np.asarray(dets[j].p)[c], ps[0], ps[1])
        return fc._tree(e)

    def total(costs):
        cc = []
        for i0 in range(0, N, CHUNK):
            acc = costs[i0]
            for i in range(i0 + 1, min(i0 + CHUNK, N)):
                acc = acc + costs[i]
            cc.append(acc)
        cn = cc[0]
        for v in cc[1:]:
            cn = cn + v
        return cn

    which = 0
    viewcost = [view_cost(i, 0, pose[0][i]) if ntags[i] > 0 else 0.0 for i in range(N)]
    cost = cost0 = total(viewcost)
    lam, accepted, rejected = 1e-3, 0, 0
    corners, used = 4 * sum(ntags), sum(1 for n in ntags if n > 0)
    M = 6 * T
    cov = [[0.0] * 36 for _ in range(T)]
    cov_valid = False
    for it in range(iters + 1):
        final = it == iters
        lm = 0.0 if final else lam
        # accumulate
        keep = [None] * N
        for i, (dets, _p, cam) in enumerate(views):
            if ntags[i] <= 0:
                continue
            R, t = pose[which][i]
            rows = {}
            for j in range(len(dets)):
                J = slot_tag(i, j)
                if J < 0:
                    continue
                for c in range(4):
                    rows[4 * j + c] = _slot_rows(cam, tag[which][J], signs[c][0], signs[c][1], np.asarray(dets[j].p)[c], R, t,
                                                 free[6 * J], free[6 * J + 3])
            U = []
            for a, b in _TRI:
                e = [0.0] * 64
                for s, r in rows.items():
                    e[s] = r[0][a] * r[0][b] + r[1][a] * r[1][b]
                U.append(fc._tree(e))
            g = []
            for a in range(6):
                e = [0.0] * 64
                for s, r in rows.items():
                    e[s] = r[0][a] * r[4] + r[1][a] * r[5]
                g.append(fc._tree(e))
            per = {}
            for j in range(len(dets)):
                J = slot_tag(i, j)
                if J < 0:
                    continue
                q = [rows[4 * j + c] for c in range(4)]
                V = [_quad([r[2][a] * r[2][b] + r[3][a] * r[3][b] for r in q]) for a, b in _TRI]
                h = [_quad([r[2][a] * r[4] + r[3][a] * r[5] for r in q]) for a in range(6)]
                W = [[_quad([r[0][k] * r[2][b] + r[1][k] * r[3][b] for r in q]) for b in range(6)] for k in range(6)]
                Y = [[0.0] * 6 for _ in range(6)]
                for b in range(6):
                    x = _solve6(U, [-W[k][b] for k in range(6)], lm)
                    for k in range(6):
                        Y[k][b] = x[k]
                per[J] = (j, V, h, W, Y)
            y = _solve6(U, [-v for v in g], lm)
            keep[i] = (U, g, y, per)
        # reduce
        S = {}
        rhs, vd = [0.0] * M, [0.0] * M

        def chunked(term):
            tot = 0.0
            for i0 in range(0, N, CHUNK):
                acc = 0.0
                for i in range(i0, min(i0 + CHUNK, N)):
                    v = term(i)
                    if v is not None:
                        acc = acc + v
                tot = tot + acc
            return tot

        for J in range(T):
            for K in range(J, T):
                for a in range(6):
                    for b in range(6):
                        if J == K and a > b:
                            continue

                        def term(i, J=J, K=K, a=a, b=b):
                            if keep[i] is None or J not in keep[i][3] or K not in keep[i][3]:
                                return None
                            Wj, Yk = keep[i][3][J][3], keep[i][3][K][4]
                            tt = Wj[0][a] * Yk[0][b]
                            for k in range(1, 6):
                                tt = tt + Wj[k][a] * Yk[k][b]
                            v0 = keep[i][3][J][1][_tri[(a, b)]] if J == K else 0.0
                            return v0 - tt
                        S[(6 * J + a, 6 * K + b)] = chunked(term)
            for a in range(6):
                def term_r(i, J=J, a=a):
                    if keep[i] is None or J not in keep[i][3]:
                        return None
                    W, yv = keep[i][3][J][3], keep[i][2]
                    tt = W[0][a] * yv[0]
                    for k in range(1, 6):
                        tt = tt + W[k][a] * yv[k]
                    return keep[i][3][J][2][a] - tt

                def term_v(i, J=J, a=a):
                    if keep[i] is None or J not in keep[i][3]:
                        return None
                    return keep[i][3][J][1][_tri[(a, a)]]
                rhs[6 * J + a] = chunked(term_r)
                vd[6 * J + a] = chunked(term_v)
        # solve
        A = [[0.0] * M for _ in range(M)]
        for r in range(M):
            for s in range(r, M):
                a = S[(r, s)]
                if not free[r] or not free[s]:
                    a = 1.0 if r == s else 0.0
                elif r == s and not final:
                    a = a + lam * vd[r]
                A[r][s] = a
        L = [[0.0] * M for _ in range(M)]
        ok = True
        for j in range(M):
            s = A[j][j]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            if not s > 0.0:
                ok = False   # (every step is zero and no covariance: nothing reads L again)
                break
            ljj = math.sqrt(s)
            L[j][j] = ljj
            for i in range(j + 1, M):
                v = A[j][i]
                for k in range(j):
                    v = v - L[i][k] * L[j][k]
                L[i][j] = v / ljj
        if final:
            den = 2 * corners - 6 * used - sum(free)
            cov_valid = ok and den > 0
            if cov_valid:
                s2 = cost / float(den)
                for p in range(M):
                    if not free[p]:
                        continue
                    c = p // 6
                    w = [1.0 if i == p else 0.0 for i in range(M)]
                    for k in range(p, M):
                        w[k] = w[k] / L[k][k]
                        for i in range(k + 1, M):
                            w[i] = w[i] - L[i][k] * w[k]
                    for k in range(M - 1, 6 * c - 1, -1):
                        w[k] = w[k] / L[k][k]
                        for i in range(6 * c, k):
                            w[i] = w[i] - L[k][i] * w[k]
                    for b in range(6):
                        cov[c][(p % 6) * 6 + b] = s2 * w[6 * c + b] if free[6 * c + b] else 0.0
            break
        dc = [0.0] * M
        if ok:
            v = [-rhs[i] if free[i] else 0.0 for i in range(M)]
            yv = [0.0] * M
            for k in range(M):
                yv[k] = v[k] / L[k][k]
                for i in range(k + 1, M):
                    v[i] = v[i] - L[i][k] * yv[k]
            v = list(yv)
            xv = [0.0] * M
            for k in range(M - 1, -1, -1):
                xv[k] = v[k] / L[k][k]
                for i in range(k):
                    v[i] = v[i] - L[k][i] * xv[k]
            dc = [xv[i] if free[i] else 0.0 for i in range(M)]
        other = which ^ 1
        for J in range(T):
            Rj, tj = tag[which][J]
            Rn = fc._mul(np.asarray(Rj), _step_R(dc[6 * J:6 * J + 3])).tolist()
            tn = [tj[k] + dc[6 * J + 3 + k] for k in range(3)]
            tag[other][J] = (Rn if free[6 * J] else Rj, tn if free[6 * J + 3] else tj)
        # back
        cand = [0.0] * N
        for i in range(N):
            if keep[i] is None:
                continue
            U, g, _y, per = keep[i]
            r = []
            for k in range(6):
                acc = g[k]
                for J, (j, _V, _h, W, _Y) in sorted(per.items(), key=lambda kv: kv[1][0]):
                    for b in range(6):
                        acc = acc + W[k][b] * dc[6 * J + b]
                r.append(acc)
            x = fc._solve6({ij: U[k] for k, ij in enumerate(_TRI)}, r, lam)
            d = x if (x is not None and ok) else [0.0] * 6
            R, t = pose[which][i]
            pn = (fc._mul(_step_R(d), np.asarray(R)).tolist(), [t[k] + d[3 + k] for k in range(3)])
            pose[other][i] = pn
            cand[i] = view_cost(i, other, pn)
        cn = total(cand)
        if ok and cn < cost:
            which, cost, accepted, lam = other, cn, accepted + 1, max(lam / 10.0, 1e-9)
        else:
            rejected, lam = rejected + 1, lam * 10.0
    viewcost = [view_cost(i, which, pose[which][i]) if ntags[i] > 0 else 0.0 for i in range(N)]
    res = SimpleNamespace(rms_before=math.sqrt(cost0 / corners) if corners else 0.0,
                          rms_after=math.sqrt(cost / corners) if corners else 0.0, views_used=used,
                          views_skipped=N - used, corners=corners, accepted=accepted, rejected=rejected,
                          cov_valid=cov_valid, cost=cost)
    tag_out = [SimpleNamespace(id=int(tags[J][0]), placed=bool(placed[J]), views=seen[J],
                               R=np.array(tag[which][J][0]) if placed[J] else np.zeros((3, 3)),
                               t=np.array(tag[which][J][1]) if placed[J] else np.zeros(3),
                               cov=np.array(cov[J]).reshape(6, 6) if placed[J] and cov_valid else np.zeros((6, 6)))
               for J in range(T)]
    view_out = [SimpleNamespace(used=ntags[i] > 0, n_tags=ntags[i] if ntags[i] > 0 else 0,
                                R=np.array(pose[which][i][0]) if ntags[i] > 0 else np.zeros((3, 3)),
                                t=np.array(pose[which][i][1]) if ntags[i] > 0 else np.zeros(3),
                                rms_px=math.sqrt(viewcost[i] / float(4 * ntags[i])) if ntags[i] > 0 else 0.0)
                for i in range(N)]
    return res, tag_out, view_out


# ---- residuals for the Jacobian and least-squares checks ------------------------------------------
def rodrigues(w):
    a = float(np.linalg.norm(w))
    if a == 0.0:
        return np.eye(3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / a
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def residuals(views, idx, tag_poses, cam_poses, tag_size=fc.TAG_SIZE):
    """The pixel residuals (u then v per corner, views in order, tags by slot) of the stored views
    under the given tag poses [(R, t)] and camera poses [(R, t)]."""
    out = []
    for (dets, _p, cam), (R, t) in zip(views, cam_poses):
        for d in dets:
            Rt, tt = tag_poses[idx[d.id]]
            px, _z = fc.project(cam, np.asarray(R), np.asarray(t), fc.tag_corners_field(np.asarray(Rt), np.asarray(tt), tag_size))
            out.append((px - np.asarray(d.p)).reshape(-1))
    return np.concatenate(out)
