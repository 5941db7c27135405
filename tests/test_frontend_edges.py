"""Front-end parity at value edges, tiny frames, every format and both launch modes.

Input conversion + decimation (k_pre<FMT>; the PRE path of k_thr_ccl in latency mode)
and the adaptive threshold of thr_ccl_tile, on inputs that reach their edges
(tests/frontend_cases.py): a filtered tile contrast on either side of
min_white_black_diff, pixels on either side of the tile threshold over its whole range,
frames from 24x24 (below one CCL tile) upwards, the BGR8 colour cube, YUYV with live
chroma, tags against the top and left borders, device-resident frames with a padded
stride.

CPU part: the C oracle's gray / decimated / thresholded planes equal the plain numpy
restatement bit for bit, the inputs meet their coverage conditions, the oracle finds
the expected ids.  GPU part: every stage of the HIP path equals the oracle's
(compare_frame + compare_detections), in latency mode (max_batch 1) and in throughput
mode (max_batch 8, batches of different frames).
"""
import functools

import numpy as np
import pytest

import frontend_cases as fc
from parity_util import compare_detections, compare_frame

FORMATS = (fc.FMT_GRAY8, fc.FMT_YUYV, fc.FMT_BGR8)
BIG = [(648, 488), (800, 600)]
CPU_GEOMETRIES = fc.GEOMETRIES + [(48, 48), (72, 56), (512, 384)] + BIG


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True  # the IndexPoint tap (copy_blob_points) for every detector here
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


@pytest.fixture(scope="module")
def codes(oracle_mod):
    return dict(oracle_mod.family_entries())


def _oracle(oracle_mod, W, H, m=5):
    p = oracle_mod.default_params(W, H)
    p.min_white_black_diff = m
    return oracle_mod.Oracle(W, H, p)


@functools.lru_cache(maxsize=None)
def _banded(W, H, m):
    return tuple(fc.banded_frames(W, H, 7000 + 13 * m + W + H, m, 6))


@functools.lru_cache(maxsize=None)
def _flipped(W, H, k):
    import ao
    return fc.flipped_edge_board(W, H, W + H + 7 * k, dict(ao.family_entries()))


def _grays(W, H, m, codes):
    """The gray planes of one geometry at one min_white_black_diff: (name, plane, id or
    None); eight of them, so that they fill a throughput batch."""
    out = [("noise", fc.white_noise(W, H, 3 * W + H), None)]
    out += [("banded%d" % k, f, None) for k, f in enumerate(_banded(W, H, m))]
    if (W, H) in fc.TINY_TAGS:
        g, tid = fc.tiny_tag(W, H, codes)
        out.append(("tag", g, tid))
    else:
        out.append(("noise2", fc.white_noise(W, H, 5 * W + H + 1), None))
    return out


# ---- CPU: restatement == oracle, coverage conditions, expected ids --------------

def _assert_front_end(orc, frame, fmt, m, what):
    orc.detect(frame, fmt)
    y = fc.luma(frame, fmt)
    dec = fc.decimate(y)
    assert np.array_equal(orc.gray(), y), ("gray",) + what
    assert np.array_equal(orc.decimated(), dec), ("decimated",) + what
    assert np.array_equal(orc.thresholded(), fc.threshold(dec, m)), ("thresholded",) + what


@pytest.mark.parametrize("W,H", CPU_GEOMETRIES)
def test_oracle_equals_numpy_restatement(oracle_mod, codes, W, H):
    """ao_oracle.c's gray(), decimated() and thresholded() against frontend_cases' luma,
    decimate and threshold: every input of the geometry, all three formats (YUYV with
    live chroma, BGR8 tinted), min_white_black_diff in {0, 1, 5, 6, 255}.  (The two border
    geometries, which are not in the list of small ones, take white noise, three banded
    frames and a flipped board; 512x384 takes the colour cube as well.)"""
    for m in fc.DIFFS:
        orc = _oracle(oracle_mod, W, H, m)
        grays = _grays(W, H, m, codes)
        if (W, H) in BIG:
            grays = grays[:4] + [("flipped", _flipped(W, H, 0)[0], None)]
        for name, g, _ in grays:
            for fmt in FORMATS:
                _assert_front_end(orc, fc.as_format(g, fmt, seed=W + m, chroma=True), fmt, m, (W, H, m, name, fmt))
        if (W, H) == (512, 384):
            for k in range(3):
                _assert_front_end(orc, fc.color_cube(k), fc.FMT_BGR8, m, (W, H, m, "cube", k))


def test_color_cube_holds_every_pair():
    seen = np.zeros((256, 256), bool)
    bs = set()
    for k in range(3):
        f = fc.color_cube(k)
        assert f.shape == (384, 512, 3)
        top = f[:256]
        seen[top[..., 2].ravel(), top[..., 1].ravel()] = True
        bs |= set(int(b) for b in np.unique(f[..., 0]))
        for b in np.unique(top[..., 0]):  # whole blocks: every (R, G) pair at this B
            blk = top[top[..., 0] == b]
            assert len(set(zip(blk[:, 2].tolist(), blk[:, 1].tolist()))) == 65536
    assert seen.all() and len(bs) == 18 and {0, 128, 255} <= bs
    # ... and it tells each luma coefficient from the next one up (the next one down gives
    # the same Y for every one of the 2^24 colours: the sums never land that close above a
    # multiple of 2^20)
    cube = np.concatenate([fc.color_cube(k) for k in range(3)]).astype(np.int64)
    coef = (102760, 528482, 269484)
    want = fc.luma(cube, fc.FMT_BGR8)
    for ch in range(3):
        c = list(coef)
        c[ch] += 1
        y = (c[0] * cube[..., 0] + c[1] * cube[..., 1] + c[2] * cube[..., 2] + (1 << 19) + (16 << 20)) >> 20
        assert np.count_nonzero(y != want) >= 10, ch


@pytest.mark.parametrize("W,H", [g for g in CPU_GEOMETRIES if min(g) >= fc.TINY])
@pytest.mark.parametrize("m", [1, 5, 6])
def test_banded_coverage(W, H, m):
    """Conditions on the inputs (from the numpy reference alone): each banded frame of a
    geometry that holds super-blocks decides d < m on both sides and at m, and v > th on
    both sides of th, for th from near 0 to near 255."""
    for k, f in enumerate(_banded(W, H, m)):
        c = fc.coverage(fc.decimate(f), m)
        assert min(c["d_below"], c["d_at"], c["d_above"]) >= 5, (k, c)
        assert c["v_eq_th"] >= 100 and c["v_eq_th1"] >= 100, (k, c)
        assert c["th_min"] <= 3 and c["th_max"] >= 250, (k, c)
        assert c["n127"] >= 1 and c["nlive"] >= 1, (k, c)


@pytest.mark.parametrize("W,H", [g for g in CPU_GEOMETRIES if min(g) >= fc.TINY])
def test_banded_coverage_at_0_and_255(W, H):
    """m = 0: d = -1 does not exist and no pixel is 127; every other condition holds.
    m = 255: a tile is live only at d = 255 (th = 127 then, so the th range and the
    hundreds of pixels at th do not exist); the frame holds a saturated super-block, so
    live tiles exist, and tiles at d = 254 and d = 255."""
    for k, f in enumerate(_banded(W, H, 0)):
        c = fc.coverage(fc.decimate(f), 0)
        assert c["n127"] == 0 and c["d_below"] == 0 and min(c["d_at"], c["d_above"]) >= 5, (k, c)
        assert c["v_eq_th"] >= 100 and c["v_eq_th1"] >= 100 and c["th_min"] <= 3 and c["th_max"] >= 250, (k, c)
        assert not np.any(fc.threshold(fc.decimate(f), 0) == 127)
    for k, f in enumerate(_banded(W, H, 255)):
        c = fc.coverage(fc.decimate(f), 255)
        assert c["live_d"] == [255] and c["nlive"] >= 16 * 5 and c["n127"] >= 1, (k, c)
        assert min(c["d_below"], c["d_at"]) >= 5 and c["d_above"] == 0, (k, c)
        assert c["v_eq_th"] >= 1 and c["v_eq_th1"] >= 1 and c["th_min"] == c["th_max"] == 127, (k, c)


@pytest.mark.parametrize("W,H", [g for g in CPU_GEOMETRIES if min(g) < fc.TINY])
@pytest.mark.parametrize("m", fc.DIFFS)
def test_tiny_banded_coverage(W, H, m):
    """A small frame holds one span; over the batch all of d = m-1, m, m+1 (those within
    0 .. 255) occur, and pixels at th and at th + 1."""
    c = fc.merge_coverage([fc.coverage(fc.decimate(f), m) for f in _banded(W, H, m)])
    for key, d in (("d_below", m - 1), ("d_at", m), ("d_above", m + 1)):
        assert (c[key] >= 1) == (0 <= d <= 255), (key, c)
    assert c["v_eq_th"] >= 1 and c["v_eq_th1"] >= 1, c
    assert (c["n127"] == 0) == (m == 0), c
    if m == 255:
        assert c["live_d"] == [255]


@pytest.mark.parametrize("W,H", sorted(fc.TINY_TAGS))
def test_tiny_tag_frames_detect_on_the_oracle(oracle_mod, codes, W, H):
    orc = _oracle(oracle_mod, W, H)
    for k in range(fc.NTINY):
        g, tid = fc.tiny_tag(W, H, codes, k)
        orc.detect(g, fc.FMT_GRAY8)
        assert orc.status() == 0 and [d["id"] for d in orc.detections()] == [tid], (k, tid)


@pytest.mark.parametrize("W,H", BIG)
def test_flipped_edge_boards_detect_on_the_oracle(oracle_mod, W, H):
    orc = _oracle(oracle_mod, W, H)
    for k in range(8):
        g, ids = _flipped(W, H, k)
        assert len(ids) == 10
        orc.detect(g, fc.FMT_GRAY8)
        assert orc.status() == 0 and set(ids) <= set(d["id"] for d in orc.detections()), k


# ---- GPU: every stage against the oracle, both launch modes -----------------------

def _run(det, oracle_mod, frames, fmt, m=5, ids=None, what=()):
    """frames through det -- one call in throughput mode, one by one in latency mode --
    and every stage and detection of every frame against the oracle.  ids: per frame the
    ids that must be among the detections (or None).  Returns the detections."""
    orc = _oracle(oracle_mod, det.width, det.height, m)
    if det.max_batch > 1:
        res = det.detect_batch(frames, fmt)
    out = []
    for c, f in enumerate(frames):
        dets = res[c] if det.max_batch > 1 else det.detect(f, fmt)
        orc.detect(f, fmt)
        assert det.frame_status(c if det.max_batch > 1 else 0) == orc.status(), what + (c,)
        assert compare_frame(det, orc, frame_idx=c if det.max_batch > 1 else 0) == [], what + (c,)
        assert compare_detections(dets, orc.detections()) == [], what + (c,)
        if ids is not None and ids[c] is not None:
            assert set(ids[c]) <= set(d.id for d in dets), what + (c,)
        out.append(dets)
    return out


gpu_mark = pytest.mark.gpu
BATCHES = [1, 8]  # latency mode (32-wide CCL tiles, conversion fused into k_thr_ccl); throughput mode


@gpu_mark
@pytest.mark.parametrize("W,H", fc.GEOMETRIES + [(48, 48), (72, 56)])
@pytest.mark.parametrize("batch", BATCHES)
def test_geometries(gpu, oracle_mod, codes, W, H, batch):
    """From below one CCL tile to several: white noise, the banded frames and (where one
    fits) a tag, as GRAY8 and as YUYV with live chroma."""
    det = gpu.GpuDetector(W, H, max_batch=batch)
    grays = _grays(W, H, 5, codes)
    ids = [None if t is None else [t] for _, _, t in grays]
    for fmt in (fc.FMT_GRAY8, fc.FMT_YUYV):
        frames = [fc.as_format(g, fmt, seed=W + k, chroma=True) for k, (_, g, _) in enumerate(grays)]
        res = _run(det, oracle_mod, frames, fmt, ids=ids, what=(W, H, batch, fmt))
        for dets, want in zip(res, ids):
            if want is not None:
                assert [d.id for d in dets] == want
    det.close()


@gpu_mark
@pytest.mark.parametrize("m", fc.DIFFS)
@pytest.mark.parametrize("W,H,fmt", [(264, 136, fc.FMT_YUYV), (136, 72, fc.FMT_GRAY8)])
@pytest.mark.parametrize("batch", BATCHES)
def test_min_white_black_diff(gpu, oracle_mod, codes, W, H, fmt, m, batch):
    """The frames banded around m, with that m on both sides."""
    det = gpu.GpuDetector(W, H, max_batch=batch, min_white_black_diff=m)
    frames = [fc.as_format(g, fmt, seed=m + k, chroma=True) for k, (_, g, _) in enumerate(_grays(W, H, m, codes))]
    _run(det, oracle_mod, frames, fmt, m=m, what=(W, H, batch, m))
    thr = det.copy_thresholded(0)
    assert np.array_equal(thr, fc.threshold(fc.decimate(fc.luma(frames[0 if batch > 1 else -1], fmt)), m))
    det.close()


@gpu_mark
@pytest.mark.parametrize("batch", BATCHES)
def test_bgr_color_cube(gpu, oracle_mod, codes, batch):
    """Every (R, G) pair and carry of the BGR -> Y fixed point: the gray plane equals the
    numpy luma as well as the oracle's.  Throughput mode: one call of eight BGR8 frames."""
    from ros_vision_amd import synth
    W, H = 512, 384
    rng = np.random.default_rng(8)
    frames = [fc.color_cube(k) for k in range(3)]
    frames += [fc.tinted(synth.render_board(W, H, seed=50 + k, ntags=4, codes=codes)[0]) for k in range(3)]
    frames += [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(2)]
    det = gpu.GpuDetector(W, H, max_batch=batch)
    if batch > 1:
        _run(det, oracle_mod, frames, fc.FMT_BGR8, what=("cube", batch))
        for c, f in enumerate(frames):
            assert np.array_equal(det.copy_gray(c), fc.luma(f, fc.FMT_BGR8)), c
    else:
        for c, f in enumerate(frames):
            _run(det, oracle_mod, [f], fc.FMT_BGR8, what=("cube", batch, c))
            assert np.array_equal(det.copy_gray(0), fc.luma(f, fc.FMT_BGR8)), c
    det.close()


@gpu_mark
@pytest.mark.parametrize("W,H", BIG + [(136, 72)])
@pytest.mark.parametrize("batch", BATCHES)
def test_bgr_tinted_boards(gpu, oracle_mod, codes, W, H, batch):
    """BGR8 whose luma equals no channel: the decode samples the written gray plane.
    Partial-tile geometries and one tile plus a sliver."""
    from ros_vision_amd import synth
    if (W, H) in BIG:
        grays = [synth.render_edge_board(W, H, seed=W + H + 7 * k, codes=codes)[0] for k in range(4)]
        grays += [_flipped(W, H, k)[0] for k in range(4)]
    else:
        grays = [fc.tiny_tag(W, H, codes, k)[0] for k in range(4)] + [g for _, g, _ in _grays(W, H, 5, codes)[:4]]
    frames = [fc.tinted(g) for g in grays]
    det = gpu.GpuDetector(W, H, max_batch=batch)
    res = _run(det, oracle_mod, frames, fc.FMT_BGR8, what=(W, H, batch))
    if (W, H) in BIG:
        assert all(len(r) >= 1 for r in res)
    det.close()


@gpu_mark
@pytest.mark.parametrize("W,H,fmt", [(648, 488, fc.FMT_YUYV), (800, 600, fc.FMT_GRAY8)])
@pytest.mark.parametrize("batch", BATCHES)
def test_top_and_left_borders(gpu, oracle_mod, W, H, fmt, batch):
    """Tags and blobs flush against the top and left borders (negative halo coordinates,
    the x > 0 / y > 0 guards): every stage equal, every pasted id detected."""
    boards = [_flipped(W, H, k) for k in range(8 if batch > 1 else 3)]
    frames = [fc.as_format(g, fmt, seed=k, chroma=True) for k, (g, _) in enumerate(boards)]
    det = gpu.GpuDetector(W, H, max_batch=batch)
    _run(det, oracle_mod, frames, fmt, ids=[ids for _, ids in boards], what=(W, H, batch))
    det.close()


@gpu_mark
@pytest.mark.parametrize("W,H", [(136, 72), (648, 488)])
@pytest.mark.parametrize("batch", BATCHES)
def test_device_frames_with_padded_stride(gpu, oracle_mod, codes, W, H, batch):
    """Frames in HBM at a stride above the frame size (padding 0xA5): YUYV + 16, GRAY8 + 8
    (frames 1 and 2 start 8 mod 16), BGR8 + 24.  Throughput mode: the three frames in one
    call; latency mode: frame by frame.  Stages and detections equal the oracle's on each
    frame alone, the buffer is unchanged, strides the loads cannot take are refused."""
    import torch
    from ros_vision_amd import synth
    if (W, H) == (136, 72):
        grays = [fc.tiny_tag(W, H, codes, 0)[0], _banded(W, H, 5)[1], fc.white_noise(W, H, 77)]
    else:
        grays = [_flipped(W, H, 0)[0], synth.render_edge_board(W, H, seed=W + H, codes=codes)[0],
                 _banded(W, H, 5)[0]]
    det = gpu.GpuDetector(W, H, max_batch=batch)
    orc = _oracle(oracle_mod, W, H)
    for fmt, pad in ((fc.FMT_YUYV, 16), (fc.FMT_GRAY8, 8), (fc.FMT_BGR8, 24)):
        frames = [np.ascontiguousarray(fc.as_format(g, fmt, seed=k, chroma=True)) for k, g in enumerate(grays)]
        nb = frames[0].nbytes
        stride = nb + pad
        host = np.full(3 * stride, 0xA5, np.uint8)
        for k, f in enumerate(frames):
            host[k * stride:k * stride + nb] = f.ravel()
        t = torch.from_numpy(host.copy()).cuda()
        assert t.data_ptr() % 16 == 0
        if batch > 1:
            res = det.detect_device(t.data_ptr(), stride, 3, fmt)
        for k, f in enumerate(frames):
            if batch == 1:
                res = {k: det.detect_device(t.data_ptr() + k * stride, stride, 1, fmt)[0]}
            orc.detect(f, fmt)
            assert compare_frame(det, orc, frame_idx=k if batch > 1 else 0) == [], (fmt, k)
            assert compare_detections(res[k], orc.detections()) == [], (fmt, k)
        assert np.array_equal(t.cpu().numpy(), host), fmt
        bad = [nb + 4] + ([nb + 8] if fmt == fc.FMT_YUYV else [])
        for s in bad:
            with pytest.raises(RuntimeError, match=r"\(%d\)" % gpu.detector.AT_E_INVALID):
                det.enqueue_device(t.data_ptr(), s, 1, fmt)
    det.close()


@gpu_mark
def test_call_order_keeps_no_tile_state(gpu, oracle_mod, codes):
    """One throughput detector: a banded batch (frames full of 127 pixels), a tag batch,
    the banded batch again -- each equal to the oracle."""
    W, H = 264, 136
    det = gpu.GpuDetector(W, H, max_batch=8)
    banded = list(_banded(W, H, 5)) + list(_banded(W, H, 6))[:2]
    tags = [fc.tiny_tag(W, H, codes, k) for k in range(8)]
    _run(det, oracle_mod, banded, fc.FMT_GRAY8, what=("banded",))
    res = _run(det, oracle_mod, [g for g, _ in tags], fc.FMT_GRAY8, ids=[[t] for _, t in tags], what=("tags",))
    assert [[d.id for d in r] for r in res] == [[t] for _, t in tags]
    _run(det, oracle_mod, banded, fc.FMT_GRAY8, what=("banded again",))
    det.close()
