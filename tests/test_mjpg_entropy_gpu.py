"""MJPG entropy decode on the GPU (at_mjpg_set_device_entropy, k_mjpg_entropy): the host
parses markers only, the scan bytes cross the link as they are and the kernel leaves the
dense coefficient layout k_mjpg_idct reads.

Everything is compared with the switch off (the host decode, pinned by test_mjpg_gpu.py and
test_mjpg_color_gpu.py) and with Pillow: planes and BGR images equal, detections equal.  Bad
entropy-coded data, which only the device sees now, gives a flat frame with status
AT_E_INVALID while the rest of its batch stands."""
import io
import json
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import mjpg_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL, MID = (24, 40), (328, 248)   # a handful of pieces, one partial; partial MCUs at 4:2:0
AT_E_INVALID = -1
TABLE_BLOCK = 64 + 3 * 256 + 6 * 1424   # geometry, stream headers, at most six decode tables


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True  # AT_STAGE_GRAY of the decoded plane
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


@pytest.fixture(scope="module")
def dets(gpu):
    """Detectors shared by the tests: (w, h, device entropy on?, colour on?, max_batch)."""
    cache = {}

    def get(w, h, on, color=False, batch=1):
        key = (w, h, on, color, batch)
        if key not in cache:
            d = gpu.GpuDetector(w, h, max_batch=batch)
            d.set_mjpg_device_entropy(on)
            d.set_mjpg_color(color)
            cache[key] = d
        return cache[key]
    yield get
    for d in cache.values():
        d.close()


@pytest.fixture(scope="module")
def boards():
    return {(w, h): mc.board(w, h, ntags=2 if w > 100 else 1, side_range=(40, 72) if w > 100 else (16, 20))
            for w, h in (SMALL, MID)}


def pil_bgr(jpg):
    return np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))[:, :, ::-1]


def scan_bytes(jpg):
    """Bytes behind the SOS segment: what the compressed-input slot (W * H bytes) has to hold."""
    return len(jpg) - mc.segments(jpg)[-1][2]


def _same_detections(a, b):
    """The same plane through the same kernels: equal."""
    assert [d.id for d in a] == [d.id for d in b]
    for x, y in zip(a, b):
        assert x.hamming == y.hamming
        for f in ("p", "c", "H"):
            assert np.array_equal(getattr(x, f), getattr(y, f))


def _plane_on_equals_off(dets, size, jpg, want=None):
    on, off = dets(*size, True), dets(*size, False)
    a = on.detect_mjpg(jpg)
    b = off.detect_mjpg(jpg)
    got = on.copy_gray()
    assert np.array_equal(got, off.copy_gray())
    assert np.array_equal(got, mc.pil_luma(jpg) if want is None else want)
    assert on.frame_status(0) == 0 and on.last_status == 0
    _same_detections(a, b)
    s = on.mjpg_stats()
    if scan_bytes(jpg) > size[0] * size[1]:   # (q100 at the small sizes: more than a byte per pixel)
        assert s["host_route_frames"] == 1
    else:
        assert s["sync_rounds"] >= 1 and s["host_route_frames"] == 0
        assert abs(s["device_bytes"] - s["compressed_bytes"]) <= TABLE_BLOCK + 256
    return s


@pytest.mark.parametrize("quality", [5, 75, 100])
@pytest.mark.parametrize("sampling", list(mc.SAMPLINGS))
@pytest.mark.parametrize("size", [SMALL, MID])
def test_plane_equals_switch_off_and_pillow(dets, boards, size, sampling, quality):
    _plane_on_equals_off(dets, size, mc.encode(boards[size], quality, sampling))


@pytest.mark.parametrize("extra", [{"restart_marker_blocks": 1}, {"restart_marker_rows": 1}])
@pytest.mark.parametrize("sampling", list(mc.SAMPLINGS))
def test_plane_restart_markers(dets, boards, sampling, extra):
    jpg = mc.encode(boards[MID], 75, sampling, **extra)
    assert jpg.count(b"\xff\xd7") >= 1
    _plane_on_equals_off(dets, MID, jpg)


def test_plane_without_dht_and_optimised_tables(dets, boards):
    jpg = mc.encode(boards[MID], 75, "422")
    _plane_on_equals_off(dets, MID, mc.with_avi1_app0(mc.strip_dht(jpg)), want=mc.pil_luma(jpg))
    _plane_on_equals_off(dets, MID, mc.encode(boards[MID], 75, "420", optimize=True))


@pytest.mark.parametrize("size,quality,sampling", [((640, 480), 85, "422"), ((1280, 720), 80, "422")])
def test_plane_larger_frames(dets, size, quality, sampling):
    """More pieces than the workgroup has threads at 1280x720: the loop over pieces."""
    from ros_vision_amd import synth
    gray, _ = synth.render_board(size[0], size[1], seed=766, ntags=4)
    s = _plane_on_equals_off(dets, size, mc.encode(gray, quality, sampling))
    print("sync rounds at %dx%d q%d: %d" % (size[0], size[1], quality, s["sync_rounds"]))


@pytest.mark.parametrize("subseq", [16, 64, 256])
def test_other_piece_sizes(dets, boards, subseq):
    det = dets(*MID, True)
    det.set_mjpg_subseq(subseq)
    try:
        for s in ("420", "gray"):
            _plane_on_equals_off(dets, MID, mc.encode(boards[MID], 75, s, restart_marker_rows=1))
    finally:
        det.set_mjpg_subseq(128)
    with pytest.raises(RuntimeError):
        det.set_mjpg_subseq(48)


@pytest.mark.parametrize("sampling", list(mc.SAMPLINGS))
def test_colour_image_equals_pillow(dets, sampling):
    w, h = MID
    jpg = mc.encode(mc.tinted(mc.board(w, h, ntags=2)), 75, sampling)
    on, off = dets(w, h, True, True), dets(w, h, False, True)
    on.detect_mjpg(jpg)
    off.detect_mjpg(jpg)
    got = on.copy_bgr()
    assert np.array_equal(got, off.copy_bgr())
    assert np.array_equal(got, pil_bgr(jpg))
    assert np.array_equal(on.copy_gray(), mc.pil_luma(jpg))


# ---- detections ------------------------------------------------------------------
def _detections_equal(gpu, jpg, want_ids=None):
    h, w = mc.pil_luma(jpg).shape
    res = []
    for on in (False, True):
        det = gpu.GpuDetector(w, h, tag_size=0.1651)
        det.set_mjpg_device_entropy(on)
        found = det.detect_mjpg(jpg)
        res.append((found, det.poses(), det.copy_gray()))
        det.close()
    (a, pa, ga), (b, pb, gb) = res
    assert np.array_equal(ga, gb)
    _same_detections(a, b)
    assert [p.id for p in pa] == [p.id for p in pb]
    for x, y in zip(pa, pb):
        assert np.array_equal(x.R, y.R) and np.array_equal(x.t, y.t)
    if want_ids is not None:
        assert [d.id for d in b] == want_ids
    return b


def test_detections_board_640x480(gpu):
    from ros_vision_amd import synth
    gray, _ = synth.render_board(640, 480, seed=766, ntags=4, ids=[0, 1, 2, 554])
    assert len(_detections_equal(gpu, mc.encode(gray, 85, "422"))) >= 1


def test_detections_one_tag_328x248(gpu):
    gray = mc.board(328, 248, seed=3, ntags=1, ids=[17], side_range=(72, 96))
    _detections_equal(gpu, mc.encode(gray, 60, "420"))


@pytest.mark.parametrize("name,ids", [("colorimage.jpg", [554]), ("grayimage.jpg", [585])])
def test_detections_reference_fixtures(gpu, golden_dir, name, ids):
    """1920x1080 4:2:0 (1080 rows: padded luma blocks are decoded and dropped) and 1280x800
    single-component."""
    _detections_equal(gpu, open(os.path.join(golden_dir, name), "rb").read(), ids)


# ---- batches ---------------------------------------------------------------------
def _mixed_batch(w, h):
    from ros_vision_amd import synth
    frames = [synth.render_board(w, h, seed=40 + i, ntags=4)[0] for i in range(8)]
    jpgs = [mc.encode(f, 80, ("444", "422", "420", "gray")[i % 4]) for i, f in enumerate(frames)]
    jpgs[3] = mc.encode(frames[3], 80, "422", restart_marker_rows=1)
    jpgs[5] = mc.encode(np.full((h, w, 3), 93, np.uint8), 75, "420")
    jpgs[6] = mc.encode(mc.noise(w, h), 100, "444")
    return jpgs


def test_mixed_batch_with_a_host_route_frame(dets):
    """Three samplings, restart markers, a flat frame, and q100 noise whose scan exceeds
    W * H bytes: that frame is decoded by the host inside the same batch."""
    w, h = 640, 480
    jpgs = _mixed_batch(w, h)
    assert scan_bytes(jpgs[6]) > w * h
    assert all(len(j) < w * h for i, j in enumerate(jpgs) if i != 6)
    on, off = dets(w, h, True, batch=8), dets(w, h, False, batch=8)
    a = on.detect_mjpg_batch(jpgs)
    b = off.detect_mjpg_batch(jpgs)
    s = on.mjpg_stats()
    assert s["host_route_frames"] == 1 and s["sync_rounds"] >= 1
    for f, jpg in enumerate(jpgs):
        assert np.array_equal(on.copy_gray(f), mc.pil_luma(jpg)), "frame %d" % f
        assert on.frame_status(f) == 0
        _same_detections(a[f], b[f])
    assert sum(len(x) for x in a) >= 5


def test_back_to_back_batches_and_switching(dets):
    """Both staging sets and stale payloads: two batches with the switch on, then off, on
    again, fewer frames, through one detector."""
    w, h = MID
    det = dets(w, h, True, batch=3)
    batches = [[mc.encode(mc.board(w, h, seed=30 + 3 * k + i, ntags=2, side_range=(48, 80)), q, s)
                for i, (s, q) in enumerate((("422", 75), ("420", 95), ("gray", 50)))] for k in range(3)]
    try:
        for k, (jpgs, on) in enumerate([(batches[0], True), (batches[1], True), (batches[2], False),
                                        (batches[0][::-1], True), (batches[1][:2], False), (batches[2][:1], True)]):
            det.set_mjpg_device_entropy(on)
            det.enqueue_mjpg(jpgs)
            det.collect()
            for f, jpg in enumerate(jpgs):
                assert np.array_equal(det.copy_gray(f), mc.pil_luma(jpg)), "batch %d frame %d" % (k, f)
        det.enqueue_mjpg(batches[0])
        det.enqueue_mjpg(batches[1])   # over a batch not yet collected
        det.collect()
        for f, jpg in enumerate(batches[1]):
            assert np.array_equal(det.copy_gray(f), mc.pil_luma(jpg))
    finally:
        det.set_mjpg_device_entropy(True)


def _bad_entropy_streams(gpu, good, w, h):
    """One truncated scan and one corrupted one, headers intact, both refused by the host
    decoder (tests/test_mjpg_entropy_host.py runs such streams under the sanitizers)."""
    scan = good.index(b"\xff\xda") + 14
    cut = good[:scan + (len(good) - scan) // 2]
    bad = None
    for c in mc.corruptions(good, 200):
        if c[:scan] != good[:scan]:
            continue
        try:
            gpu.mjpg_stream_mode(c, w, h)
        except gpu.MjpgError:
            bad = c
            break
    assert bad is not None
    for s in (cut, bad):
        with pytest.raises(gpu.MjpgError):
            gpu.mjpg_stream_mode(s, w, h)
    return cut, bad


def test_bad_entropy_data_gives_flat_frames_and_status(gpu, dets):
    w, h = MID
    good = [mc.encode(mc.board(w, h, seed=20 + i, ntags=2, side_range=(48, 80)), 80, "420", restart_marker_rows=1)
            for i in range(2)]
    cut, bad = _bad_entropy_streams(gpu, good[0], w, h)
    on, off = dets(w, h, True, batch=4), dets(w, h, False, batch=4)
    want = off.detect_mjpg_batch(good)
    got = on.detect_mjpg_batch([good[0], cut, bad, good[1]])   # enqueue succeeds
    assert on.last_status == AT_E_INVALID
    assert [on.frame_status(f) for f in range(4)] == [0, AT_E_INVALID, AT_E_INVALID, 0]
    for f in (1, 2):
        assert got[f] == [] and np.all(on.copy_gray(f) == 128)
    for f, g in ((0, 0), (3, 1)):
        assert np.array_equal(on.copy_gray(f), mc.pil_luma(good[g]))
        _same_detections(got[f], want[g])
    # and the detector goes on
    again = on.detect_mjpg_batch(good)
    assert on.last_status == 0 and [on.frame_status(f) for f in range(2)] == [0, 0]
    for f in range(2):
        _same_detections(again[f], want[f])


# ---- upper layers ----------------------------------------------------------------
def test_python_node_publishes_the_same(gpu):
    from ros_vision_amd import synth
    from ros_vision_amd.node import ApriltagsDetectorNode
    gray, _ = synth.render_board(640, 480, seed=766, ntags=4, ids=[0, 1, 2, 554])
    jpg = mc.encode(gray, 85, "422")
    out = []
    for on in (False, True):
        node = ApriltagsDetectorNode(640, 480, mjpg_device_entropy=on)
        out.append(node.image_callback(jpg, stamp_s=5.0, encoding="jpeg"))
        node.close()
    a, b = out
    assert len(a.tag_detection_array) >= 1
    assert a.tag_detection_array == b.tag_detection_array
    assert a.tag_detection_camera_array == b.tag_detection_camera_array
    assert a.networktables_pose_data == b.networktables_pose_data


def test_mock_node_publishes_the_same(gpu, tmp_path):
    from ros_vision_amd import synth
    node_dir = os.path.join(ROOT, "node")
    subprocess.run(["make", "-C", node_dir, "-s"], check=True)
    W, H = 640, 480
    jpgs = [mc.encode(synth.render_board(W, H, seed=50 + i, ntags=3)[0], 85, s) for i, s in enumerate(("422", "420"))]
    (tmp_path / "cam.mjpg").write_bytes(b"".join(jpgs))
    outs = []
    for flags in ([], ["--mjpg-device-entropy"]):
        r = subprocess.run([os.path.join(node_dir, "at_mock_node")] + flags +
                           ["--width", str(W), "--height", str(H), "--format", "mjpg", "--frames",
                            str(tmp_path / "cam.mjpg")], check=True, capture_output=True, text=True, timeout=180)
        outs.append([json.loads(l) for l in r.stdout.splitlines()][1:])
    assert len(outs[0]) == len(outs[1]) == 2
    for a, b in zip(*outs):
        assert len(a["detections"]) >= 1 and a["status"] == b["status"] == 0
        for k in ("detections", "robot", "camera", "networktables"):
            assert a[k] == b[k], k
