"""Throughput mode's FitQuads runs in k_fit_quads, a row of 16 lanes per kept blob and
four blobs per wave, from the hand-over record the blob kernels leave per blob.

What can go wrong only there: a group of fewer than four blobs (0, 1 or 3 kept blobs, the
fifth of 5), rows whose blobs have different peak counts (no fit at all under 4 peaks, one
row round for 4, five fit rounds and 14 combination rounds from 10 on), the closing
segment of a quad, which wraps around the end of the blob's point list, combinations of
equal error (the reference takes the first: a blob all of whose 210 combinations fail
records the first one's indices), an invalid blob next to valid ones, and the
records of the blob kernels' other launches (513-1,024 points a wave, 1,025-4,096 a
256-thread team, above 4,096 a 512-thread team).

Scenes are black polygons on white, one kept blob each, so the kept blobs of a frame can
be counted.  CPU part (no marker): the oracle alone pins the blob counts, peak counts and
point counts that make the GPU half meaningful.  GPU part: a max_batch = 8 detector with
the taps on, every frame alone and all frames of a size in one batch; copy_quads and
copy_blob_points bit-equal to a max_batch = 1 detector's (whose blob kernels fit the quads
themselves) and to the oracle's.
"""
import numpy as np
import pytest

import tag_scenes as ts
from parity_util import compare_frame

GRAY8 = 2
SMALL = (256, 192)
VGA = (640, 480)
FHD = (1920, 1080)


def fill(img, pts):
    """Fill the polygon pts (x, y) black: even-odd test at the pixel centres."""
    pts = np.asarray(pts, np.float64)
    hh, ww = img.shape
    ys, xs = np.mgrid[0:hh, 0:ww]
    x, y = xs + 0.5, ys + 0.5
    inside = np.zeros(img.shape, bool)
    for (x0, y0), (x1, y1) in zip(pts, np.roll(pts, -1, axis=0)):
        if y0 == y1:
            continue
        inside ^= ((y0 > y) != (y1 > y)) & (x < (x1 - x0) * (y - y0) / (y1 - y0) + x0)
    img[inside] = 0


def ngon(cx, cy, r, n, phase):
    a = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)


def star(cx, cy, r0, r1, n, phase):
    a = phase + np.pi * np.arange(2 * n) / n
    r = np.where(np.arange(2 * n) % 2 == 0, r0, r1)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)


def rect(x0, y0, w, h):
    return [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)]


# shapes by what FitQuads makes of them (test_oracle_* pin it): name -> polygon at a centre
SHAPES = {
    "square": lambda cx, cy: rect(cx - 20, cy - 20, 40, 40),      # axis-aligned: 4 peaks, one combination
    "sliver": lambda cx, cy: rect(cx - 26, cy - 3, 52, 6),        # 2 peaks: no quad
    "turned": lambda cx, cy: ngon(cx, cy, 16, 4, 0.5),            # a turned square: 4-9 peaks
    "pentagon": lambda cx, cy: ngon(cx, cy, 14, 5, 0.3),          # 4-9 peaks
    "octagon": lambda cx, cy: ngon(cx, cy, 26, 8, 0.2),           # 10 or more peaks, a valid quad
    "star": lambda cx, cy: star(cx, cy, 28, 14, 5, 0.1),          # 10 or more peaks, a valid quad all the same
    "bigstar": lambda cx, cy: star(cx, cy, 70, 35, 5, 0.1),       # 10 or more peaks, every combination fails
}
CENTRES = [(34, 48), (98, 48), (162, 48), (222, 48), (34, 144), (98, 144), (162, 144), (222, 144)]

# 256 x 192 frames: kept blobs 0, 1, 3, 4, 5 (and the shapes' peak classes between them)
SMALL_FRAMES = {
    "kept0": [],
    "kept1": ["square"],
    "kept3": ["sliver", "turned", "octagon"],
    "kept4": ["square", "sliver", "pentagon", "octagon"],  # an invalid blob among valid ones in one row group
    "kept5": ["octagon", "turned", "sliver", "square", "star"],
    "ties": ["bigstar"],
}
CENTRES_OF = {"ties": [(128, 96)]}


def centres(key):
    return CENTRES_OF.get(key, CENTRES)

_FRAMES = {}
_ORACLES = {}


def frame(key):
    if key not in _FRAMES:
        if key in SMALL_FRAMES:
            img = np.full((SMALL[1], SMALL[0]), 255, np.uint8)
            for name, (cx, cy) in zip(SMALL_FRAMES[key], centres(key)):
                fill(img, SHAPES[name](cx, cy))
        elif key == "vga":  # squares of 200 and 400 px: 800 and 1,600 boundary points
            img = np.full((VGA[1], VGA[0]), 255, np.uint8)
            fill(img, rect(12, 40, 400, 400))
            fill(img, rect(428, 140, 200, 200))
        elif key == "fhd_tag":  # tag 5 stretched to 1800 x 1000 px: a border of 1440 x 800
            img = np.full((FHD[1], FHD[0]), ts.BACKGROUND, np.uint8)
            ts.draw_tag(img, ts.codes()[5], np.array(rect(60, 40, 1800, 1000), np.float64))
        elif key == "fhd_shapes":
            img = np.full((FHD[1], FHD[0]), 255, np.uint8)
            for k, name in enumerate(("square", "star", "octagon", "turned", "sliver")):
                fill(img, SHAPES[name](200 + 300 * k, 500))
        else:
            raise KeyError(key)
        img = np.ascontiguousarray(img)
        img.setflags(write=False)
        _FRAMES[key] = img
    return _FRAMES[key]


def size_of(key):
    return SMALL if key in SMALL_FRAMES else VGA if key == "vga" else FHD


def oracle(oracle_mod, key):
    if key not in _ORACLES:
        w, h = size_of(key)
        orc = oracle_mod.Oracle(w, h, oracle_mod.default_params(w, h, "tag36h11"))
        orc.detect(frame(key), GRAY8)
        _ORACLES[key] = orc
    return _ORACLES[key]


def blob_stats(orc):
    """(points, peaks, centroid x, centroid y) of every kept blob in blob order, from the
    oracle's taps: a peak is a strict cyclic local maximum of the blob's filtered errors;
    the centroid is in full-resolution pixels."""
    ip, fe = orc.sorted_index_points(), orc.filtered_errs()
    bi = (ip >> np.uint64(52)).astype(np.int64)
    x = ((ip >> np.uint64(14)) & np.uint64(0x3ff)).astype(np.float64) * 2
    y = ((ip >> np.uint64(4)) & np.uint64(0x3ff)).astype(np.float64) * 2
    out = []
    for b in np.unique(bi):
        m = bi == b
        f = fe[m]
        out.append((len(f), int(np.sum((f > np.roll(f, 1)) & (f > np.roll(f, -1)))), x[m].mean(), y[m].mean()))
    assert sum(s[1] for s in out) == orc.num_peaks()
    return out


def by_shape(orc, key):
    """name -> (points, peaks, valid) of the frame's shapes, each matched to the kept
    blob whose centroid is nearest to the shape's centre."""
    stats, fq = blob_stats(orc), orc.fitquads()
    assert len(stats) == len(fq) == len(SMALL_FRAMES[key])
    out = {}
    for name, (cx, cy) in zip(SMALL_FRAMES[key], centres(key)):
        k = int(np.argmin([(sx - cx) ** 2 + (sy - cy) ** 2 for _, _, sx, sy in stats]))
        assert abs(stats[k][2] - cx) < 6 and abs(stats[k][3] - cy) < 6, (key, name, stats[k])
        out[name] = (stats[k][0], stats[k][1], bool(fq[k].valid))
    assert len(out) == len(stats)
    return out


def peak_class(p):
    return "<4" if p < 4 else "4-9" if p < 10 else ">=10"


# ---- CPU part ---------------------------------------------------------------------

@pytest.mark.parametrize("key,kept", [("kept0", 0), ("kept1", 1), ("kept3", 3), ("kept4", 4), ("kept5", 5), ("ties", 1)])
def test_oracle_kept_blobs(oracle_mod, key, kept):
    orc = oracle(oracle_mod, key)
    assert len(blob_stats(orc)) == len(orc.fitquads()) == kept == len(SMALL_FRAMES[key])
    assert orc.status() == 0


def test_oracle_shape_classes(oracle_mod):
    """Peak classes and validity of the shapes, in every frame that holds them."""
    want = {"square": ("4-9", True), "sliver": ("<4", False), "turned": ("4-9", True), "pentagon": ("4-9", True),
            "octagon": (">=10", True), "star": (">=10", True), "bigstar": (">=10", False)}
    for key in SMALL_FRAMES:
        for name, (n, p, valid) in by_shape(oracle(oracle_mod, key), key).items():
            assert (peak_class(p), valid) == want[name], (key, name, n, p, valid)
            if name == "square":
                assert p == 4  # the axis-aligned square: exactly its corners
    # kept4: one invalid blob and three valid ones, all in one group of four rows
    assert sorted(v for _, _, v in by_shape(oracle(oracle_mod, "kept4"), "kept4").values()) == [False, True, True, True]


def test_oracle_closing_segment_wraps(oracle_mod):
    """The quad's indices ascend, so its closing side runs from the last index over the
    end of the point list to the first: the wrap-around branch of the segment moments."""
    for key in ("kept1", "kept4", "vga"):
        orc = oracle(oracle_mod, key)
        for f, (n, _, _, _) in zip(orc.fitquads(), blob_stats(orc)):
            if f.valid:
                idx = [int(v) for v in f.indices]
                assert idx == sorted(idx) and 0 < idx[0] and idx[3] < n - 1


def test_oracle_large_blobs(oracle_mod):
    orc = oracle(oracle_mod, "vga")
    stats = sorted(s[0] for s in blob_stats(orc))
    assert len(stats) == 2 and 513 <= stats[0] <= 1024 and 1025 <= stats[1] <= 4096
    assert all(f.valid for f in orc.fitquads()) and len(orc.quads()) == 2
    orc = oracle(oracle_mod, "fhd_tag")
    big = max(range(len(orc.fitquads())), key=lambda k: blob_stats(orc)[k][0])
    assert blob_stats(orc)[big][0] > 4096 and orc.fitquads()[big].valid and len(orc.quads()) == 1
    assert len(blob_stats(oracle(oracle_mod, "fhd_shapes"))) == 5


# ---- GPU part ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


_DETS = {}


def detectors(gpu, size):
    """(throughput detector, latency detector) of a frame size, made once."""
    if size not in _DETS:
        _DETS[size] = (gpu.GpuDetector(size[0], size[1], max_batch=8, family="tag36h11"),
                       gpu.GpuDetector(size[0], size[1], max_batch=1, family="tag36h11"))
    return _DETS[size]


def quad_bytes(det, idx):
    """Every field of frame idx's fitted-quad records, as comparable values."""
    return [(q["blob_index"], q["valid"], q["accepted"], tuple(q["indices"]), q["corners"].tobytes())
            for q in det.copy_quads(idx)]


def check_batch(gpu, oracle_mod, keys):
    size = size_of(keys[0])
    det8, det1 = detectors(gpu, size)
    det8.detect_batch([frame(k) for k in keys], gpu.AT_FMT_GRAY8)
    for idx, key in enumerate(keys):
        orc = oracle(oracle_mod, key)
        assert compare_frame(det8, orc, frame_idx=idx) == [], key
        quads, points = quad_bytes(det8, idx), det8.copy_blob_points(idx)
        fq = orc.fitquads()
        assert [(q[0], q[1]) for q in quads] == [(int(f.blob_index), bool(f.valid)) for f in fq], key
        assert [q[3] for q in quads if q[1]] == [tuple(int(v) for v in f.indices) for f in fq if f.valid], key
        det1.detect_batch([frame(key)], gpu.AT_FMT_GRAY8)
        assert compare_frame(det1, orc, frame_idx=0) == [], key
        assert quad_bytes(det1, 0) == quads, key
        assert np.array_equal(det1.copy_blob_points(0), points), key


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(SMALL_FRAMES))
def test_gpu_small_frame_alone(gpu, oracle_mod, key):
    """0, 1, 3, 4 and 5 kept blobs: a launch with no group, groups of one, three and four
    rows, and a full group followed by a group of one; "ties": 210 combinations of equal
    (maximal) error, whose first is recorded (compared with the latency detector's)."""
    check_batch(gpu, oracle_mod, [key])


@pytest.mark.gpu
def test_gpu_small_frames_in_one_batch(gpu, oracle_mod):
    """14 kept blobs of six frames (one of them empty) in one work list: groups that mix
    frames and peak classes."""
    check_batch(gpu, oracle_mod, list(SMALL_FRAMES))


@pytest.mark.gpu
def test_gpu_large_blobs(gpu, oracle_mod):
    """One blob of the one-wave 513-1,024-point launch and one of the 256-thread teams."""
    check_batch(gpu, oracle_mod, ["vga"])


@pytest.mark.gpu
def test_gpu_border_over_4096_points(gpu, oracle_mod):
    """1920 x 1080: a tag border of more than 4,096 points (the 512-thread teams' launch)
    in a batch with a frame of small blobs."""
    check_batch(gpu, oracle_mod, ["fhd_tag", "fhd_shapes"])
