"""Cases and an independent reference for the game-piece output parse (at_gp_parse_host,
GpuDetector.game_piece_parse).

`reference` restates the contract of include/at_api.h in numpy, on float32 arrays:
per prediction the first class holding the maximum score above 0 (a NaN never wins),
dropped iff that confidence < conf_thr; candidates by np.lexsort((index, -confidence));
greedy suppression of later same-class candidates with iou > iou_thr, where
max(a, b) = b if a < b else a and min(a, b) = b if b < a else a (std::max / std::min, which
is what decides the NaN cases), inter = max(0, dx) * max(0, dy), uni = (wa ha + wb hb) -
inter, iou = inter / uni if uni > 0 else 0; then the scaling by float32 quotients.

`generate` builds a network output with clusters of overlapping "hot" predictions;
`checked` asserts on the reference side that a case is not vacuous."""
import numpy as np

F = np.float32
BOX = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4")])
MAX_CANDIDATES = 4096


def _smax(a, b):
    return np.where(a < b, b, a)


def _smin(a, b):
    return np.where(b < a, b, a)


def reference(raw, conf_thr=0.25, iou_thr=0.45, model=(640, 640), orig=None, stats=None):
    """-> BOX records in NMS order.  `stats` (a dict) receives candidates / kept."""
    raw = np.ascontiguousarray(raw, F)
    orig = model if orig is None else orig
    conf_thr, iou_thr = F(conf_thr), F(iou_thr)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        scores = raw[4:]
        pos = np.where(scores > F(0), scores, F(0))      # what can win: NaN, -0.0, negatives cannot
        best = pos.max(axis=0)
        cls = pos.argmax(axis=0).astype(np.int32)        # the first maximum; all 0 -> class 0
        idx = np.nonzero(~(best < conf_thr))[0]
        idx = idx[np.lexsort((idx, -best[idx]))]
        x, y, w, h = (raw[k][idx] for k in range(4))
        half_w, half_h = w / F(2), h / F(2)
        x1, x2, y1, y2 = x - half_w, x + half_w, y - half_h, y + half_h
        area, c = w * h, cls[idx]
        n = len(idx)
        alive = np.ones(n, bool)
        kept = []
        for a in range(n):
            if not alive[a]:
                continue
            kept.append(a)
            s = slice(a + 1, n)
            dx = _smin(x2[a], x2[s]) - _smax(x1[a], x1[s])
            dy = _smin(y2[a], y2[s]) - _smax(y1[a], y1[s])
            inter = _smax(F(0), dx) * _smax(F(0), dy)
            uni = (area[a] + area[s]) - inter
            iou = np.where(uni > F(0), inter / np.where(uni > F(0), uni, F(1)), F(0))
            alive[s] &= ~((c[s] == c[a]) & (iou > iou_thr))
        sx, sy = F(orig[0]) / F(model[0]), F(orig[1]) / F(model[1])
        out = np.zeros(len(kept), BOX)
        k = np.array(kept, np.int64)
        out["x"], out["y"], out["w"], out["h"] = x[k] * sx, y[k] * sy, w[k] * sx, h[k] * sy
        out["conf"], out["cls"] = best[idx][k], c[k]
    if stats is not None:
        stats["candidates"], stats["kept"] = n, len(kept)
    return out


def same(a, b):
    """Bit for bit: every float field as uint32, the class, the count, the order."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != BOX or b.dtype != BOX or a.shape != b.shape:
        return False
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)))


def assert_same(got, want, what=""):
    assert len(got) == len(want), "%s: %d boxes, want %d" % (what, len(got), len(want))
    if not same(got, want):
        g, w = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 6), np.ascontiguousarray(want).view(np.uint32).reshape(-1, 6)
        bad = np.nonzero((g != w).any(axis=1))[0]
        raise AssertionError("%s: box %d differs: got %s, want %s" % (what, bad[0], got[bad[0]], want[bad[0]]))


# ---- generated network outputs ----------------------------------------------------------
#         P      C   G   quantised
SHAPES = [(77, 1, 3, False), (1000, 3, 10, False), (8400, 1, 20, False), (8400, 80, 40, False),
          (8400, 2, 20, True), (33600, 2, 60, False)]
HOT = 12


def generate(P, C, G, seed=0, quantise=False):
    """[4 + C, P]: background scores 0.2 U(0, 1) (below 0.25), boxes uniform in a 640 x 640
    input; G objects with HOT predictions each: centres jittered by sigma = 4 px, sizes
    +- 8 %, score 0.3 + 0.69 U in the object's class.  quantise: scores in steps of 1/64."""
    rng = np.random.default_rng(seed)
    raw = np.empty((4 + C, P), F)
    raw[0:2] = rng.uniform(0, 640, (2, P))
    raw[2:4] = rng.uniform(20, 200, (2, P))
    raw[4:] = 0.2 * rng.random((C, P))
    hot = rng.permutation(P)[:G * HOT].reshape(G, HOT)
    for g in range(G):
        cx, cy = rng.uniform(40, 600, 2)
        w, h = rng.uniform(60, 200, 2)
        k = int(rng.integers(C))
        i = hot[g]
        raw[0, i] = cx + rng.normal(0, 4, HOT)
        raw[1, i] = cy + rng.normal(0, 4, HOT)
        raw[2, i] = w * rng.uniform(0.92, 1.08, HOT)
        raw[3, i] = h * rng.uniform(0.92, 1.08, HOT)
        raw[4 + k, i] = 0.3 + 0.69 * rng.random(HOT)
    if quantise:
        raw[4:] = np.round(raw[4:] * 64) / 64
    return raw


def with_candidates(n, P=6000, C=2, seed=0):
    """A generated output with exactly n candidates at 0.25: n // HOT objects, and the rest
    as lone predictions raised to 0.26 .. 0.29."""
    raw = generate(P, C, n // HOT, seed)
    rng = np.random.default_rng(seed + 1)
    cold = np.nonzero(raw[4:].max(axis=0) < F(0.25))[0]
    lone = rng.permutation(cold)[:n - HOT * (n // HOT)]
    raw[4 + rng.integers(C, size=len(lone)), lone] = 0.26 + 0.03 * rng.random(len(lone))
    assert int((~(raw[4:].max(axis=0) < F(0.25))).sum()) == n
    return raw


def checked(raw, **kw):
    """The reference's boxes of a generated case, after asserting on the reference side that
    the case tests something: >= 2 boxes kept, >= half of the candidates suppressed, and no
    more candidates than the device path takes."""
    st = {}
    want = reference(raw, stats=st, **kw)
    assert st["kept"] >= 2 and 2 * st["kept"] <= st["candidates"] <= MAX_CANDIDATES, st
    return want


# ---- hand-built cases ---------------------------------------------------------------------
def _tensor(boxes, C=1, P=None):
    """boxes: (x, y, w, h, class, score) per prediction, in prediction order."""
    P = len(boxes) if P is None else P
    raw = np.zeros((4 + C, P), F)
    for i, (x, y, w, h, k, s) in enumerate(boxes):
        raw[0:4, i] = (x, y, w, h)
        raw[4 + k, i] = s
    return raw


def chain():
    """IoU(A, B) = IoU(B, C) = 0.538, IoU(A, C) = 0.25: A suppresses B, so B must not
    suppress C.  Kept: A, C."""
    return _tensor([(100, 100, 100, 100, 0, 0.9), (130, 100, 100, 100, 0, 0.8), (160, 100, 100, 100, 0, 0.7)])


def threshold_edge():
    """B = [1, 2] x [0, 1] inside A = [0, 2] x [0, 1]: inter 1, union 2, IoU exactly 0.5."""
    return _tensor([(1.0, 0.5, 2.0, 1.0, 0, 0.9), (1.5, 0.5, 1.0, 1.0, 0, 0.8)])


def cross_class():
    return _tensor([(50, 50, 40, 40, 0, 0.9), (50, 50, 40, 40, 1, 0.8), (50, 50, 40, 40, 2, 0.8)], C=3)


def ties():
    """Equal confidences: prediction 1 goes before 4 and suppresses it; 2 (another place)
    ties with both and goes between them."""
    return _tensor([(300, 300, 20, 20, 0, 0.3), (100, 100, 50, 50, 0, 0.75), (400, 100, 50, 50, 0, 0.75),
                    (500, 500, 20, 20, 0, 0.5), (101, 100, 50, 50, 0, 0.75)])


def none():
    return _tensor([(100, 100, 50, 50, 0, 0.2), (200, 100, 50, 50, 0, 0.249)])


def everything(seed=5):
    """P = 77 for conf_thr = 0: every prediction is a candidate; a third of them have no
    score above 0 (negative, -0.0 or NaN): class 0, confidence 0."""
    rng = np.random.default_rng(seed)
    raw = generate(77, 3, 3, seed)
    dead = rng.permutation(77)[:26]
    raw[4:, dead] = rng.choice(np.array([-0.5, -0.0, np.nan, 0.0], F), (3, 26))
    return raw


def odd_scores():
    nan, inf = np.nan, np.inf
    raw = _tensor([(100 + 7 * i, 100, 60, 60, 0, 0.0) for i in range(12)], C=3)
    raw[4:, 0] = (nan, 0.6, 0.5)          # NaN first: class 1
    raw[4:, 1] = (0.6, nan, 0.7)          # NaN between: class 2
    raw[4:, 2] = (inf, 0.9, inf)          # +inf wins, the first one
    raw[4:, 3] = (-inf, -1.0, -0.0)       # nothing above 0
    raw[4:, 4] = (nan, nan, nan)
    raw[4:, 5] = (-0.0, 0.0, -0.0)
    raw[4:, 6] = (0.5, 0.5, 0.5)          # equal: the first
    raw[4:, 7] = (-2.0, 0.3, inf)
    raw[4:, 8] = (1e-45, 0.0, 0.0)        # a denormal above 0
    raw[4:, 9] = (0.25, 0.0, 0.0)         # exactly the threshold: kept
    raw[4:, 10] = (np.nextafter(F(0.25), F(0)), 0.0, 0.0)
    raw[4:, 11] = (0.0, 0.0, 3e38)
    return raw


def odd_boxes():
    nan, inf = np.nan, np.inf
    b = [(100, 100, 50, 50), (100, 100, nan, 50), (100, 100, 50, 50), (nan, 100, 50, 50), (100, 100, inf, 50),
         (100, 100, 50, 50), (100, 100, 0, 0), (100, 100, 0, 0), (100, 100, -50, 50), (100, 100, -50, -50),
         (100, 100, -50, -50), (inf, inf, 50, 50), (100, 100, 1e30, 1e30), (100, 100, 1e30, 1e30),
         (100, nan, 50, 50), (100, 100, 50, nan), (100, 100, 50, 50), (-inf, 100, inf, 50), (100, 100, 3e38, 3e38),
         (100, 100, 3e38, 3e38)]
    return _tensor([(x, y, w, h, 0, 0.95 - 0.01 * i) for i, (x, y, w, h) in enumerate(b)])


def odd_boxes_orders():
    """odd_boxes in four confidence orders (which box is the kept one decides the NaN cases)."""
    base = odd_boxes()
    out = [base]
    for seed in range(3):
        r = base.copy()
        r[4] = np.random.default_rng(seed).permutation(r[4])
        out.append(r)
    return out


def grid(n_hot, P=5000, C=2, score=0.5):
    """n_hot predictions of class 1 at `score` on a grid of disjoint 8 x 8 boxes (10 px
    pitch), all equal in confidence, spread over the P indices; the rest at 0.1."""
    raw = np.zeros((4 + C, P), F)
    raw[0:2] = 5.0
    raw[2:4] = 4.0
    raw[4:] = 0.1
    i = np.sort(np.random.default_rng(n_hot).permutation(P)[:n_hot])
    k = np.arange(n_hot)
    raw[0, i], raw[1, i], raw[2, i], raw[3, i] = 10.0 * (k % 80) + 20, 10.0 * (k // 80) + 20, 8.0, 8.0
    raw[5, i] = score
    return raw


HAND = {
    "chain": (chain, {}),
    "edge_at": (threshold_edge, {"iou_thr": 0.5}),
    "edge_below": (threshold_edge, {"iou_thr": float(np.nextafter(F(0.5), F(0)))}),
    "cross_class": (cross_class, {}),
    "ties": (ties, {}),
    "none": (none, {}),
    "everything": (everything, {"conf_thr": 0.0}),
    "odd_scores": (odd_scores, {}),
    "odd_scores_thr0": (odd_scores, {"conf_thr": 0.0}),
    "odd_scores_negthr": (odd_scores, {"conf_thr": -1.0}),
    "non_square": (lambda: generate(1000, 3, 10, 11), {"orig": (1280, 720)}),
}
