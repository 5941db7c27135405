"""Inputs, a plain numpy reference and coverage counters for the detector's front end:
input conversion + decimation (k_pre<FMT>, or the PRE path of k_thr_ccl in latency
mode) and the adaptive threshold of thr_ccl_tile (threshold.cu:16-156).

The reference here is integer numpy and nothing from the library; the tests hold the
C oracle to it on the CPU and the HIP path to the oracle on the GPU.  The generators
reach what the other suites' frames do not: a filtered tile contrast d = max - min on
either side of min_white_black_diff, pixels on either side of the tile threshold th for
th over its whole range, frames below one CCL tile, every BGR8 (R, G) pair and carry of
the fixed-point luma, YUYV with live chroma, and tags against the top and left borders.
"""
import numpy as np

FMT_YUYV, FMT_BGR8, FMT_GRAY8 = 0, 1, 2

# below one CCL tile (64x32 decimated pixels in throughput mode, 32x32 in latency mode),
# exactly one tile of each mode, one tile plus 4 decimated pixels in x, in y and in
# both, 2x2 tiles plus a sliver, several tiles
GEOMETRIES = [(24, 24), (24, 40), (40, 24), (32, 32), (64, 64), (72, 40), (128, 64), (136, 72), (128, 72),
              (264, 136), (520, 264)]
DIFFS = (0, 1, 5, 6, 255)  # min_white_black_diff values
TINY = 100                 # frames with a side below this hold one span each (banded_batch)

# (W, H) -> (side_range, seed) of one-tag frames the oracle detects
TINY_TAGS = {(48, 48): ((30, 34), 2), (64, 64): ((36, 52), 2), (72, 56): ((36, 52), 2), (128, 64): ((36, 52), 2),
             (136, 72): ((36, 52), 2), (264, 136): ((48, 64), 2)}
NTINY = 8  # frames per size: seeds seed .. seed + 7


# ---- the reference ------------------------------------------------------------

def luma(frame, fmt):
    """Full-resolution Y plane of a frame: YUYV the even bytes, GRAY8 the plane, BGR8
    OpenCV's BGR2YUV_YUYV fixed point (ITUR_BT_601_SHIFT 20)."""
    frame = np.asarray(frame, np.uint8)
    if fmt == FMT_YUYV:
        return np.ascontiguousarray(frame[:, 0::2])
    if fmt == FMT_GRAY8:
        return frame.copy()
    b, g, r = (frame[..., k].astype(np.int64) for k in range(3))
    y = (269484 * r + 528482 * g + 102760 * b + (1 << 19) + (16 << 20)) >> 20
    assert y.min() >= 0 and y.max() <= 255
    return y.astype(np.uint8)


def decimate(gray):
    return np.ascontiguousarray(gray[::2, ::2])


def filtered_minmax(dec):
    """Per 4x4 tile of the decimated plane: the 3x3 (clipped at the image) minimum of the
    tile minima and maximum of the tile maxima, as int64 planes (TH, TW)."""
    Hd, Wd = dec.shape
    TH, TW = Hd // 4, Wd // 4
    t = dec.astype(np.int64).reshape(TH, 4, TW, 4)
    mn, mx = t.min(axis=(1, 3)), t.max(axis=(1, 3))
    pmn = np.full((TH + 2, TW + 2), 255, np.int64)
    pmx = np.zeros((TH + 2, TW + 2), np.int64)
    pmn[1:-1, 1:-1], pmx[1:-1, 1:-1] = mn, mx
    fmn, fmx = pmn[1:-1, 1:-1].copy(), pmx[1:-1, 1:-1].copy()
    for dy in range(3):
        for dx in range(3):
            fmn = np.minimum(fmn, pmn[dy:dy + TH, dx:dx + TW])
            fmx = np.maximum(fmx, pmx[dy:dy + TH, dx:dx + TW])
    return fmn, fmx


def _per_pixel(tiles):
    return np.repeat(np.repeat(tiles, 4, axis=0), 4, axis=1)


def threshold(dec, m):
    """127 where the filtered contrast d < m, else 255 where v > th = min + d // 2, else 0."""
    fmn, fmx = filtered_minmax(dec)
    d = fmx - fmn
    th = _per_pixel(fmn + d // 2)
    live = _per_pixel(d >= m)
    v = dec.astype(np.int64)
    return np.where(live, np.where(v > th, 255, 0), 127).astype(np.uint8)


def coverage(dec, m):
    """What a decimated plane exercises at min_white_black_diff = m."""
    fmn, fmx = filtered_minmax(dec)
    d = fmx - fmn
    tth = fmn + d // 2
    live_t = d >= m
    th, live, v = _per_pixel(tth), _per_pixel(live_t), dec.astype(np.int64)
    return dict(d_below=int(np.count_nonzero(d == m - 1)), d_at=int(np.count_nonzero(d == m)),
                d_above=int(np.count_nonzero(d == m + 1)),
                v_eq_th=int(np.count_nonzero(live & (v == th))), v_eq_th1=int(np.count_nonzero(live & (v == th + 1))),
                th_min=int(tth[live_t].min()) if live_t.any() else 256,
                th_max=int(tth[live_t].max()) if live_t.any() else -1,
                n127=int(np.count_nonzero(~live)), nlive=int(np.count_nonzero(live)),
                live_d=sorted(set(int(x) for x in d[live_t])))


def merge_coverage(covs):
    out = dict(covs[0])
    for c in covs[1:]:
        for k in ("d_below", "d_at", "d_above", "v_eq_th", "v_eq_th1", "n127", "nlive"):
            out[k] += c[k]
        out["th_min"], out["th_max"] = min(out["th_min"], c["th_min"]), max(out["th_max"], c["th_max"])
        out["live_d"] = sorted(set(out["live_d"]) | set(c["live_d"]))
    return out


# ---- inputs ---------------------------------------------------------------------

def white_noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


def _spans(m):
    return sorted({min(max(s, 0), 255) for s in range(m - 3, m + 4)})


def _bases(span, rng):
    top = 255 - span
    return [0, top, min(1, top), max(top - 1, 0), min(64, top), min(127, top), min(128, top),
            int(rng.integers(0, top + 1))]


def _fill_tiles(W, H, base, span, rng):
    """Pixels uniform in [base, base + span] per 8x8 full-resolution tile (base, span:
    (H/8, W/8) planes); one decimated pixel of every tile is the tile's base and another
    its base + span, so a tile's own contrast is exactly its span."""
    TH, TW = H // 8, W // 8
    b = np.repeat(np.repeat(base, 8, axis=0), 8, axis=1)
    s = np.repeat(np.repeat(span, 8, axis=0), 8, axis=1)
    img = b + (rng.random((H, W)) * (s + 1)).astype(np.int64)
    lo = rng.integers(0, 16, size=(TH, TW))
    hi = (lo + rng.integers(1, 16, size=(TH, TW))) % 16
    ty, tx = np.mgrid[0:TH, 0:TW]
    img[8 * ty + 2 * (lo // 4), 8 * tx + 2 * (lo % 4)] = base
    img[8 * ty + 2 * (hi // 4), 8 * tx + 2 * (hi % 4)] = base + span
    assert img.min() >= 0 and img.max() <= 255
    return img.astype(np.uint8)


def banded(W, H, seed, m, saturated=None):
    """Gray frame whose 8x8 tiles take a base and a span that are constant over super-blocks
    of 6x6 tiles; spans from m-3 .. m+3 (clipped to 0 .. 255).  The interior tiles of a
    super-block see only their own span after the 3x3 filter, which puts d exactly on
    m-1, m and m+1.  The first super-blocks (in a shuffled order) take the spans m-1, m,
    m+1 at base 0 and at base 255 - span (th down to 0 and up to 254), the rest are drawn.
    saturated (default: m == 255): one more super-block at base 0, span 255."""
    rng = np.random.default_rng(seed)
    TH, TW = H // 8, W // 8
    SH, SW = -(-TH // 6), -(-TW // 6)
    need = []
    for s in (m, m + 1, m - 1):
        if 0 <= s <= 255:
            need += [(0, s), (255 - s, s)]
    if m == 255 if saturated is None else saturated:
        need.insert(0, (0, 255))
    sb = np.zeros((SH, SW), np.int64)
    ss = np.zeros((SH, SW), np.int64)
    # whole super-blocks first, so that the spans that must occur get interior tiles
    order = sorted(range(SH * SW), key=lambda i: (min(6, TH - 6 * (i // SW)) * min(6, TW - 6 * (i % SW)) < 36, rng.random()))
    spans = _spans(m)
    for k, i in enumerate(order):
        if k < len(need):
            base, span = need[k]
        else:
            span = int(spans[rng.integers(0, len(spans))])
            bl = _bases(span, rng)
            base = int(bl[rng.integers(0, len(bl))])
        sb[i // SW, i % SW], ss[i // SW, i % SW] = base, span
    base = np.repeat(np.repeat(sb, 6, axis=0), 6, axis=1)[:TH, :TW]
    span = np.repeat(np.repeat(ss, 6, axis=0), 6, axis=1)[:TH, :TW]
    return _fill_tiles(W, H, base, span, rng)


def banded_batch(W, H, seed, m, n=6):
    """n small gray frames of one span each: m-1, m, m+1 (those within 0 .. 255) in turn,
    bases 0, 255 - span, 1, ... in turn."""
    rng = np.random.default_rng(seed)
    spans = [s for s in (m - 1, m, m + 1) if 0 <= s <= 255]
    out = []
    for k in range(n):
        span = spans[k % len(spans)]
        bl = _bases(span, rng)
        base = bl[(k // len(spans)) % len(bl)]
        TH, TW = H // 8, W // 8
        out.append(_fill_tiles(W, H, np.full((TH, TW), base, np.int64), np.full((TH, TW), span, np.int64), rng))
    return out


def banded_frames(W, H, seed, m, n=6):
    """The banded inputs of one geometry: super-block frames where they fit, else a batch
    of one-span frames."""
    if min(W, H) < TINY:
        return banded_batch(W, H, seed, m, n)
    return [banded(W, H, seed + k, m) for k in range(n)]


def tiny_tag(W, H, codes, k=0):
    """One-tag frame at one of the TINY_TAGS sizes: (gray, id)."""
    from ros_vision_amd import synth
    side, seed = TINY_TAGS[(W, H)]
    gray, truth = synth.render_board(W, H, seed + k, ntags=1, side_range=side, codes=codes)
    return gray, truth[0][0]


def flipped_edge_board(W, H, seed, codes):
    """render_edge_board rotated by 180 degrees: its tags and blobs against the top and
    left borders (a rotated tag is still that tag).  (gray, pasted ids)."""
    from ros_vision_amd import synth
    gray, ids = synth.render_edge_board(W, H, seed=seed, codes=codes)
    return np.ascontiguousarray(gray[::-1, ::-1]), ids


# B of the six regions of each colour-cube frame; the first two of a row are the whole
# 256x256 blocks
CUBE_B = ((0, 255, 2, 129, 64, 191), (128, 1, 17, 85, 170, 213), (254, 127, 42, 99, 230, 7))


def color_cube(k):
    """Frame k of 3: 512x384 BGR8, R = x % 256, G = y % 256, B constant per region: the two
    256x256 blocks of rows 0..255 (every (R, G) pair) and four 256x64 regions below them
    (G 0..127).  The three frames hold 18 values of B, with 0, 255 and 128 in whole blocks."""
    yy, xx = np.mgrid[0:384, 0:512]
    f = np.empty((384, 512, 3), np.uint8)
    f[..., 2] = xx % 256
    f[..., 1] = yy % 256
    region = np.where(yy < 256, xx // 256, 2 + 2 * ((yy - 256) // 64) + xx // 256)
    f[..., 0] = np.array(CUBE_B[k], np.uint8)[region]
    return f


def tinted(gray):
    """BGR8 whose channels are three different affine maps of a gray plane: the luma
    equals no channel."""
    g = gray.astype(np.int64)
    return np.ascontiguousarray(np.stack([g, 3 * g // 4, 255 - g // 2], axis=-1).astype(np.uint8))


def to_yuyv_chroma(gray, seed):
    """YUYV with the gray plane as Y and random bytes as U and V."""
    h, w = gray.shape
    out = np.random.default_rng(seed).integers(0, 256, size=(h, 2 * w), dtype=np.uint8)
    out[:, 0::2] = gray
    return out


def as_format(gray, fmt, seed=0, chroma=False):
    """A gray plane as a frame of format fmt whose luma is that plane (BGR8: tinted,
    whose luma is another plane)."""
    from ros_vision_amd import synth
    if fmt == FMT_GRAY8:
        return gray
    if fmt == FMT_YUYV:
        return to_yuyv_chroma(gray, seed) if chroma else synth.to_yuyv(gray)
    return tinted(gray)
