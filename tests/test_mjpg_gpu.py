"""MJPG input on the GPU: JPEG bytes in, host entropy decode, k_mjpg_idct, detection.

The decoded plane (AT_STAGE_GRAY with the taps on) must equal the host decode and
Pillow's luma-only decode of the same bytes; the detections must equal the oracle
run on that luma as GRAY8 (tests/parity_util.py, unchanged)."""
import json
import os
import subprocess

import numpy as np
import pytest

import mjpg_cases as mc
from parity_util import compare_detections, compare_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(328, 248), (24, 40)]


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True  # AT_STAGE_GRAY of a GRAY8 batch, and the parity taps
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


@pytest.fixture(scope="module")
def dets(gpu):
    """One latency-mode detector per size, shared by the plane tests."""
    cache = {}

    def get(w, h):
        if (w, h) not in cache:
            cache[(w, h)] = gpu.GpuDetector(w, h)
        return cache[(w, h)]
    yield get
    for d in cache.values():
        d.close()


@pytest.fixture(scope="module")
def boards():
    return {(w, h): mc.board(w, h, ntags=2 if w > 100 else 1, side_range=(40, 72) if w > 100 else (16, 20))
            for w, h in SIZES}


def _plane_equal(gpu, det, jpg, want=None):
    found = det.detect_mjpg(jpg)
    got = det.copy_gray()
    want = mc.pil_luma(jpg) if want is None else want
    assert np.array_equal(gpu.mjpg_decode_gray(jpg), want)
    nd = int(np.count_nonzero(got != want))
    assert got.shape == want.shape and nd == 0, "%d pixels of the GPU plane differ" % nd
    return found


@pytest.mark.parametrize("quality", [30, 95])
@pytest.mark.parametrize("sampling", list(mc.SAMPLINGS))
@pytest.mark.parametrize("size", SIZES)
def test_plane_equals_host_and_pillow(gpu, dets, boards, size, sampling, quality):
    _plane_equal(gpu, dets(*size), mc.encode(boards[size], quality, sampling))


def test_plane_dense_noise_frame(gpu, dets):
    w, h = SIZES[0]
    det = dets(w, h)
    _plane_equal(gpu, det, mc.encode(mc.noise(w, h), 100, "444"))
    s = det.mjpg_stats()
    assert s["dense_frames"] == 1 and s["device_bytes"] == 256 + 2 * w * h


def test_plane_flat_q5_dc_only(gpu, dets):
    w, h = SIZES[0]
    det = dets(w, h)
    jpg = mc.encode(np.full((h, w, 3), 93, np.uint8), 5, "420")
    _plane_equal(gpu, det, jpg)
    s = det.mjpg_stats()
    assert s["dense_frames"] == 0 and s["compressed_bytes"] == len(jpg) and s["device_bytes"] < w * h // 4


@pytest.mark.parametrize("extra", [{"restart_marker_blocks": 1}, {"restart_marker_rows": 1}])
def test_plane_restart_markers(gpu, dets, boards, extra):
    _plane_equal(gpu, dets(*SIZES[0]), mc.encode(boards[SIZES[0]], 75, "420", **extra))


def test_plane_without_dht(gpu, dets, boards):
    jpg = mc.encode(boards[SIZES[0]], 75, "422")
    _plane_equal(gpu, dets(*SIZES[0]), mc.with_avi1_app0(mc.strip_dht(jpg)), want=mc.pil_luma(jpg))


# ---- detection parity with the oracle on Pillow's luma ---------------------------
def _parity(gpu, oracle_mod, jpg, want_ids=None):
    y = mc.pil_luma(jpg)
    H, W = y.shape
    det = gpu.GpuDetector(W, H)
    found = det.detect_mjpg(jpg)
    orc = oracle_mod.Oracle(W, H)
    orc.detect(np.ascontiguousarray(y), 2)
    assert compare_frame(det, orc) == []
    assert compare_detections(found, orc.detections()) == []
    if want_ids is not None:
        assert [d.id for d in found] == want_ids
    det.close()
    return found


def test_parity_board_640x480_q85_422(gpu, oracle_mod):
    from ros_vision_amd import synth
    gray, _ = synth.render_board(640, 480, seed=766, ntags=4, ids=[0, 1, 2, 554])
    found = _parity(gpu, oracle_mod, mc.encode(gray, 85, "422"))
    assert len(found) >= 1   # (which tags survive the compression is the oracle's call)


def test_parity_one_tag_328x248_q60_420(gpu, oracle_mod):
    gray = mc.board(328, 248, seed=3, ntags=1, ids=[17], side_range=(72, 96))
    _parity(gpu, oracle_mod, mc.encode(gray, 60, "420"))


def test_parity_reference_colorimage_jpg(gpu, oracle_mod, golden_dir):
    """The reference's own 1920x1080 4:2:0 fixture (gpu_detector_test.cu:84-92): id 554."""
    _parity(gpu, oracle_mod, open(os.path.join(golden_dir, "colorimage.jpg"), "rb").read(), [554])


def test_parity_reference_grayimage_jpg(gpu, oracle_mod, golden_dir):
    """The reference's 1280x800 single-component fixture: id 585."""
    _parity(gpu, oracle_mod, open(os.path.join(golden_dir, "grayimage.jpg"), "rb").read(), [585])


# ---- batches ---------------------------------------------------------------------
def _same_detections(a, b):
    """Two runs of the same plane through this library (one per mode): equal ids and
    hamming; corners, centre and H within 2e-4 -- each mode is within 1e-4 of the
    oracle (parity_util.compare_detections), so of each other within twice that."""
    assert [d.id for d in a] == [d.id for d in b]
    for x, y in zip(a, b):
        assert x.hamming == y.hamming
        for f in ("p", "c", "H"):
            assert np.allclose(getattr(x, f), getattr(y, f), rtol=0, atol=2e-4)


def _check_batch(gpu, single, batch_det, jpgs):
    got = batch_det.detect_mjpg_batch(jpgs)
    planes = [batch_det.copy_gray(f) for f in range(len(jpgs))]
    for f, jpg in enumerate(jpgs):
        want = single.detect_mjpg(jpg)
        assert np.array_equal(planes[f], single.copy_gray()), "frame %d plane" % f
        assert np.array_equal(planes[f], mc.pil_luma(jpg))
        _same_detections(got[f], want)
    return got


def test_batch_of_three_samplings(gpu, dets):
    """One call, three streams: three sampling modes, three quantisation tables."""
    w, h = SIZES[0]
    jpgs = [mc.encode(mc.board(w, h, seed=10 + i, ntags=2, side_range=(48, 80)), q, s)
            for i, (s, q) in enumerate([("444", 90), ("422", 70), ("420", 50)])]
    det = gpu.GpuDetector(w, h, max_batch=3)
    got = _check_batch(gpu, dets(w, h), det, jpgs)
    assert sum(len(g) for g in got) >= 1
    assert det.mjpg_stats()["compressed_bytes"] == sum(len(j) for j in jpgs)
    det.close()


def test_batch_of_eight_throughput_mode(gpu):
    """max_batch=8 selects the throughput-mode kernels; 8 distinct frames, one of them
    dense (a board under noise at q100), one with restart markers; two host threads."""
    from ros_vision_amd import synth
    w, h = 640, 480
    frames = [synth.render_board(w, h, seed=40 + i, ntags=4)[0] for i in range(8)]
    rs = np.random.RandomState(2)
    noisy = np.clip(frames[2].astype(np.float64) + rs.normal(0, 12, (h, w)), 0, 255).astype(np.uint8)
    jpgs = [mc.encode(f, 80, ("444", "422", "420", "gray")[i % 4]) for i, f in enumerate(frames)]
    jpgs[2] = mc.encode(np.stack([noisy] * 3, -1), 100, "444")
    jpgs[5] = mc.encode(frames[5], 80, "422", restart_marker_rows=1)
    single = gpu.GpuDetector(w, h)
    det = gpu.GpuDetector(w, h, max_batch=8)
    det.set_mjpg_threads(2)
    got = _check_batch(gpu, single, det, jpgs)
    assert det.mjpg_stats()["dense_frames"] == 1
    assert sum(len(g) for g in got) >= 8
    # fewer frames than max_batch through the same detector
    _check_batch(gpu, single, det, jpgs[5:7])
    det.close()
    single.close()


def test_bad_frame_in_a_batch_leaves_the_detector_usable(gpu, dets):
    w, h = SIZES[0]
    good = [mc.encode(mc.board(w, h, seed=20 + i, ntags=2, side_range=(48, 80)), 80, "422") for i in range(3)]
    det = gpu.GpuDetector(w, h, max_batch=3)
    first = det.detect_mjpg_batch(good)
    for bad, code in ((mc.encode(mc.board(w, h), 80, "422", progressive=True), -6),
                      (good[1][:len(good[1]) // 2], -1),
                      (mc.encode(mc.board(w + 8, h), 80, "422"), -1)):
        with pytest.raises(gpu.MjpgError) as e:
            det.detect_mjpg_batch([good[0], bad, good[2]])
        assert e.value.frame == 1 and e.value.code == code
    # nothing was enqueued: the last batch's results are still the first one's
    assert det.copy_gray(1).tobytes() == mc.pil_luma(good[1]).tobytes()
    again = _check_batch(gpu, dets(w, h), det, good[::-1])
    for a, b in zip(again, first[::-1]):
        _same_detections(a, b)
    det.close()


def test_two_batches_back_to_back_reuse_the_staging(gpu, dets):
    """enqueue_mjpg / collect twice with different contents (both staging sets, then the
    first again), and an enqueue over a batch not yet collected."""
    w, h = SIZES[0]
    det = gpu.GpuDetector(w, h, max_batch=2)
    single = dets(w, h)
    batches = [[mc.encode(mc.board(w, h, seed=30 + 2 * k + i, ntags=2, side_range=(48, 80)), 75, s)
                for i, s in enumerate(("422", "420"))] for k in range(3)]
    for jpgs in batches:
        det.enqueue_mjpg(jpgs)
        got = det.collect()
        for f, jpg in enumerate(jpgs):
            assert np.array_equal(det.copy_gray(f), mc.pil_luma(jpg))
            _same_detections(got[f], single.detect_mjpg(jpg))
    det.enqueue_mjpg(batches[0])
    det.enqueue_mjpg(batches[1])   # waits for the pending batch itself, then replaces it
    got = det.collect()
    for f, jpg in enumerate(batches[1]):
        assert np.array_equal(det.copy_gray(f), mc.pil_luma(jpg))
        _same_detections(got[f], single.detect_mjpg(jpg))
    det.close()


def test_annotate_staged_after_mjpg_raises(gpu, dets, boards):
    det = dets(*SIZES[0])
    det.detect_mjpg(mc.encode(boards[SIZES[0]], 80, "422"))
    with pytest.raises(RuntimeError):
        det.annotate_staged(0)


# ---- nodes -----------------------------------------------------------------------
def test_python_node_jpeg_equals_mono8(gpu):
    from ros_vision_amd import synth
    from ros_vision_amd.node import ApriltagsDetectorNode
    gray, _ = synth.render_board(640, 480, seed=766, ntags=4, ids=[0, 1, 2, 554])
    jpg = mc.encode(gray, 85, "422")
    node = ApriltagsDetectorNode(640, 480)
    a = node.image_callback(jpg, stamp_s=5.0, encoding="jpeg")
    b = node.image_callback(mc.pil_luma(jpg), stamp_s=5.0, encoding="mono8")
    node.close()
    assert len(a.tag_detection_array) >= 1 and a.image is None
    # the same plane through the same kernels: equal up to the 1e-12 the node tests
    # allow between two runs (tests/test_node_cpp.py)
    assert [t[0] for t in a.tag_detection_array] == [t[0] for t in b.tag_detection_array]
    assert np.allclose(np.array(a.tag_detection_array), np.array(b.tag_detection_array), rtol=0, atol=1e-12)
    assert np.allclose(np.array(a.tag_detection_camera_array), np.array(b.tag_detection_camera_array), rtol=0,
                       atol=1e-12)
    assert np.allclose(a.networktables_pose_data, b.networktables_pose_data, rtol=0, atol=1e-12)


def test_mock_node_process_compressed_equals_gray(gpu, tmp_path):
    """DetectorCore::process_compressed through at_mock_node on an .mjpg file of two
    frames: the published records equal those of the same luma fed as gray frames."""
    from ros_vision_amd import synth
    node_dir = os.path.join(ROOT, "node")
    subprocess.run(["make", "-C", node_dir, "-s"], check=True)
    W, H = 640, 480
    jpgs = [mc.encode(synth.render_board(W, H, seed=50 + i, ntags=3)[0], 85, s) for i, s in enumerate(("422", "420"))]
    (tmp_path / "cam.mjpg").write_bytes(b"".join(jpgs))
    (tmp_path / "cam.gray").write_bytes(b"".join(mc.pil_luma(j).tobytes() for j in jpgs))
    outs = {}
    for name, fmt in (("cam.mjpg", "yuyv"), ("cam.gray", "gray")):   # the .mjpg suffix selects the format
        r = subprocess.run([os.path.join(node_dir, "at_mock_node"), "--width", str(W), "--height", str(H), "--format",
                            fmt, "--frames", str(tmp_path / name)], check=True, capture_output=True, text=True,
                           timeout=180)
        outs[name] = [json.loads(l) for l in r.stdout.splitlines()][1:]
    assert len(outs["cam.mjpg"]) == len(outs["cam.gray"]) == 2
    for a, b in zip(outs["cam.mjpg"], outs["cam.gray"]):
        assert len(a["detections"]) >= 1 and a["status"] == b["status"] == 0
        assert [d["id"] for d in a["detections"]] == [d["id"] for d in b["detections"]]
        for x, y in zip(a["detections"], b["detections"]):
            assert x["hamming"] == y["hamming"] and np.allclose(x["p"], y["p"], rtol=0, atol=1e-12)
        # (the same plane through the same kernels: the 1e-12 of tests/test_node_cpp.py)
        assert [r[0] for r in a["robot"]] == [r[0] for r in b["robot"]]
        for k in ("robot", "camera", "networktables"):
            assert np.allclose(np.array(a[k]), np.array(b[k]), rtol=0, atol=1e-12), k
