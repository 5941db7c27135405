"""MJPG colour on the GPU: with at_mjpg_set_color the Cb / Cr coefficients travel too,
k_mjpg_idct_chroma writes the chroma planes and k_mjpg_bgr the BGR8 image.

The image must equal the host decode (at_mjpg_decode_bgr_host) and Pillow's RGB decode of
the same bytes, channel-reversed, with zero differing bytes; the luma plane and the
detections must be those of the colour-off run of the same bytes.  The annotated image,
the game-piece tensors and the two nodes' published images follow from that image and
are compared with what the existing BGR8 paths give for Pillow's image."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import mjpg_cases as mc
import mjpg_color_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(ROOT, "node")
SIZES = cc.SIZES


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True  # AT_STAGE_GRAY of a GRAY8 batch
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


@pytest.fixture(scope="module")
def dets(gpu):
    """Per size one detector with colour on and one that never had it on."""
    cache = {}

    def get(w, h, color):
        if (w, h, color) not in cache:
            d = gpu.GpuDetector(w, h)
            if color:
                d.set_mjpg_color(True)
            cache[(w, h, color)] = d
        return cache[(w, h, color)]
    yield get
    for d in cache.values():
        d.close()


@pytest.fixture(scope="module")
def images():
    return {s: cc.tinted_board(*s) for s in SIZES}


@pytest.fixture(scope="module")
def nodelib():
    import fcntl
    from ros_vision_amd import detector
    with open(os.path.join(NODE, ".build.lock"), "w") as lk:   # one make at a time, as tests/test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", NODE, "-s"], check=True)
    detector.load_library()
    L = C.CDLL(os.path.join(NODE, "libat_node.so"))
    L.at_node_draw_detection_outlines.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return L


def _records(d):
    """Everything of a detection, floats as their bytes."""
    return (d.id, d.hamming, np.float32(d.decision_margin).tobytes(), np.asarray(d.H).tobytes(),
            np.asarray(d.c).tobytes(), np.asarray(d.p).tobytes())


def _cpu_outlines(nodelib, bgr, arr, n):
    """node/at_node.cpp's draw_detection_outlines (the CPU drawing the GPU drawing is
    tested equal to in tests/test_node_cpp.py) on a copy of `bgr`."""
    img = np.ascontiguousarray(bgr).copy()
    h, w = img.shape[:2]
    nodelib.at_node_draw_detection_outlines(img.ctypes.data, w, h, arr, n)
    return img


def _image_and_detection_path(gpu, dets, size, jpg, ref=None):
    """Colour on: the image equals the host decode and Pillow.  The gray plane and the
    detections equal the colour-off run of the same bytes through another detector."""
    on, off = dets(*size, True), dets(*size, False)
    want = cc.pil_bgr(jpg if ref is None else ref)
    found = on.detect_mjpg(jpg)
    got, gray = on.copy_bgr(), on.copy_gray()
    assert np.array_equal(gpu.mjpg_decode_bgr(jpg), want)
    nd = int(np.count_nonzero(got != want))
    print("differing bytes: %d of %d" % (nd, want.size))
    assert got.shape == want.shape and nd == 0, "%d bytes of the GPU image differ" % nd
    found_off = off.detect_mjpg(jpg)
    assert np.array_equal(gray, off.copy_gray()) and np.array_equal(gray, mc.pil_luma(jpg if ref is None else ref))
    assert [_records(d) for d in found] == [_records(d) for d in found_off]
    with pytest.raises(RuntimeError):
        off.copy_bgr()
    return found


@pytest.mark.parametrize("quality", cc.QUALITIES)
@pytest.mark.parametrize("sampling", list(mc.SAMPLINGS))
@pytest.mark.parametrize("size", SIZES)
def test_image_equals_host_and_pillow(gpu, dets, images, size, sampling, quality):
    _image_and_detection_path(gpu, dets, size, mc.encode(images[size], quality, sampling))


@pytest.mark.parametrize("sampling", ["444", "420"])
def test_image_dense_noise_frame(gpu, dets, sampling):
    """Every plane dense: the slot's worst case at 4:4:4."""
    w, h = SIZES[0]
    jpg = mc.encode(mc.noise(w, h), 100, sampling)
    _image_and_detection_path(gpu, dets, (w, h), jpg)
    s = dets(w, h, True).mjpg_stats()
    assert s["dense_frames"] == 1
    nchroma = (w // 8) * (h // 8) if sampling == "444" else ((w + 15) // 16) * ((h + 15) // 16)
    assert s["device_bytes"] == (256 + 2 * w * h) + 2 * (256 + 128 * nchroma)
    assert dets(w, h, False).mjpg_stats()["device_bytes"] == 256 + 2 * w * h


@pytest.mark.parametrize("extra", [{"restart_marker_blocks": 1}, {"restart_marker_rows": 1}])
@pytest.mark.parametrize("sampling", ["422", "420"])
def test_image_restart_markers(gpu, dets, images, sampling, extra):
    _image_and_detection_path(gpu, dets, SIZES[0], mc.encode(images[SIZES[0]], 75, sampling, **extra))


def test_image_three_tables_and_no_dht(gpu, dets, images):
    _image_and_detection_path(gpu, dets, SIZES[0], cc.three_tables(images[SIZES[0]], "420"))
    full = mc.encode(images[SIZES[0]], 75, "422")
    _image_and_detection_path(gpu, dets, SIZES[0], mc.with_avi1_app0(mc.strip_dht(full)), ref=full)


def test_colour_off_sends_the_same_bytes(gpu, dets, images):
    """The colour-off stream on the link is as long as the host says, which
    tests/test_mjpg_color_host.py pins to the parent commit's; colour on adds to it."""
    size = SIZES[0]
    jpg = mc.encode(images[size], 75, "420")
    on, off = dets(*size, True), dets(*size, False)
    off.detect_mjpg(jpg)
    on.detect_mjpg(jpg)
    assert off.mjpg_stats()["device_bytes"] == gpu.mjpg_stream_mode(jpg, *size)[1]
    assert on.mjpg_stats()["device_bytes"] > off.mjpg_stats()["device_bytes"]
    assert off.mjpg_stats()["color_kernels_ns"] == 0 and on.mjpg_stats()["color_kernels_ns"] == 0   # not profiling


def test_mixed_batch_and_buffer_reuse(gpu):
    """max_batch = 8 (throughput mode), every sampling in one enqueue_mjpg, two host
    threads; then a shorter batch with the samplings permuted through the same buffers."""
    w, h = SIZES[0]
    order = ["444", "422", "420", "gray", "420", "gray", "444", "422"]
    imgs = [mc.tinted(mc.board(w, h, seed=60 + i, ntags=2, side_range=(48, 80))) for i in range(8)]
    jpgs = [mc.encode(im, q, s) for im, s, q in zip(imgs, order, [90, 70, 50, 80, 95, 30, 60, 85])]
    det = gpu.GpuDetector(w, h, max_batch=8)
    det.set_mjpg_color(True)
    det.set_mjpg_threads(2)
    det.detect_mjpg_batch(jpgs)
    for f, jpg in enumerate(jpgs):
        assert np.array_equal(det.copy_bgr(f), cc.pil_bgr(jpg)), "frame %d (%s)" % (f, order[f])
        assert np.array_equal(det.copy_gray(f), mc.pil_luma(jpg))
    second = [mc.encode(imgs[i], 75, s) for i, s in enumerate(["gray", "420", "422", "444", "422"])]
    det.enqueue_mjpg(second)
    det.collect()
    for f, jpg in enumerate(second):
        assert np.array_equal(det.copy_bgr(f), cc.pil_bgr(jpg)), "second batch, frame %d" % f
    with pytest.raises(RuntimeError):
        det.copy_bgr(len(second))   # not a frame of the last batch
    det.close()


def _one_tag_jpg():
    gray = mc.board(328, 248, seed=3, ntags=1, ids=[17], side_range=(72, 96))
    return mc.encode(mc.tinted(gray), 90, "422")


def test_annotated_image(gpu, nodelib):
    w, h = SIZES[0]
    jpg = _one_tag_jpg()
    det = gpu.GpuDetector(w, h)
    det.set_mjpg_color(True)
    found = det.detect_mjpg(jpg)
    assert [d.id for d in found] == [17]
    arr, n = det._records_array(0)
    want = _cpu_outlines(nodelib, cc.pil_bgr(jpg), arr, n)
    assert not np.array_equal(want, cc.pil_bgr(jpg))
    got = det.annotate_staged(0)
    assert np.array_equal(got, want), int((got != want).any(axis=-1).sum())
    # the next batch decodes afresh (the drawing consumed only that batch's image)
    det.detect_mjpg(jpg)
    assert np.array_equal(det.copy_bgr(), cc.pil_bgr(jpg))
    det.set_mjpg_color(False)
    det.detect_mjpg(jpg)
    with pytest.raises(RuntimeError):
        det.annotate_staged(0)
    det.close()


@pytest.mark.parametrize("channels", [1, 3])
def test_game_piece_input(gpu, channels):
    """at_gp_enable + a colour MJPG batch: the tensor is the one a BGR8 batch of Pillow's
    image of the same JPEG gives."""
    w, h = 64, 48
    jpg = mc.encode(mc.noise(w, h, seed=9), 90, "420")
    det = gpu.GpuDetector(w, h)
    det.enable_game_piece_input(40, 28, channels)
    det.detect(cc.pil_bgr(jpg), gpu.AT_FMT_BGR8)
    want = det.game_piece_tensor(0)
    assert want.shape == (channels, 28, 40) and want.std() > 0.05
    det.detect_mjpg(jpg)                      # colour off: no tensor
    with pytest.raises(RuntimeError):
        det.game_piece_tensor(0)
    det.set_mjpg_color(True)
    det.detect_mjpg(jpg)
    assert det.game_piece_tensor_ptr(0) != 0
    assert det.game_piece_tensor(0).tobytes() == want.tobytes()
    det.set_mjpg_color(False)
    det.detect_mjpg(jpg)                      # a later colour-off batch invalidates it again
    with pytest.raises(RuntimeError):
        det.game_piece_tensor(0)
    det.close()


def test_gating(gpu, images):
    """copy_bgr follows what the last batch was, not the current setting; the first
    colour-on batch of a detector that has luma-only MJPG buffers replaces them."""
    size = SIZES[0]
    jpg = mc.encode(images[size], 80, "420")
    det = gpu.GpuDetector(*size)
    with pytest.raises(RuntimeError):
        det.copy_bgr()                        # no batch at all
    det.detect_mjpg(jpg)                      # colour off
    with pytest.raises(RuntimeError):
        det.copy_bgr()
    det.set_mjpg_color(True)                  # ... and on without a new batch
    with pytest.raises(RuntimeError):
        det.copy_bgr()
    with pytest.raises(RuntimeError):
        det.mjpg_bgr_ptr()
    det.detect_mjpg(jpg)
    assert det.mjpg_bgr_ptr() != 0
    assert np.array_equal(det.copy_bgr(), cc.pil_bgr(jpg)) and np.array_equal(det.copy_gray(), mc.pil_luma(jpg))
    with pytest.raises(RuntimeError):
        det.copy_bgr(1)
    det.detect(cc.pil_bgr(jpg), gpu.AT_FMT_BGR8)   # a BGR8 batch
    with pytest.raises(RuntimeError):
        det.copy_bgr()
    det.set_mjpg_color(False)                 # off without a new batch: the last batch still was not colour
    with pytest.raises(RuntimeError):
        det.copy_bgr()
    det.set_mjpg_color(True)
    det.detect_mjpg(jpg)
    det.set_mjpg_color(False)                 # the last batch was a colour batch, whatever the setting is now
    assert np.array_equal(det.copy_bgr(), cc.pil_bgr(jpg))
    det.close()


def test_colour_kernel_time_is_reported_while_profiling(gpu, dets, images):
    size = SIZES[0]
    det = gpu.GpuDetector(*size)
    det.set_mjpg_color(True)
    det.set_profiling(True)
    det.detect_mjpg(mc.encode(images[size], 80, "420"))
    s = det.mjpg_stats()
    print(s)
    assert s["idct_kernel_ns"] > 0 and s["color_kernels_ns"] > 0
    det.close()


# ---- nodes -----------------------------------------------------------------------
def test_python_node_publishes_the_annotated_image(gpu, nodelib):
    from ros_vision_amd import synth
    from ros_vision_amd.node import ApriltagsDetectorNode
    gray, _ = synth.render_board(640, 480, seed=766, ntags=4, ids=[0, 1, 2, 554])
    jpg = mc.encode(mc.tinted(gray), 85, "422")
    out = {}
    for color in (True, False):
        got = {}
        node = ApriltagsDetectorNode(640, 480, mjpg_color=color,
                                     publishers={"apriltags/images": lambda m, g=got: g.setdefault("img", m)})
        res = node.image_callback(jpg, stamp_s=5.0, encoding="jpeg")
        arr, n = node.detector._records_array(0)
        out[color] = (res, got, _cpu_outlines(nodelib, cc.pil_bgr(jpg), arr, n), n)
        node.close()
    res, got, want, n = out[True]
    assert n >= 1 and len(res.tag_detection_array) >= 1
    assert res.image is got["img"] and np.array_equal(res.image, want)
    plain, got_plain, _, _ = out[False]
    assert plain.image is None and "img" not in got_plain
    assert res.tag_detection_array == plain.tag_detection_array
    assert res.tag_detection_camera_array == plain.tag_detection_camera_array
    assert res.networktables_pose_data == plain.networktables_pose_data


def test_mock_node_mjpg_color_writes_the_annotated_frames(gpu, nodelib, tmp_path):
    """at_mock_node --mjpg-color on a two-frame .mjpg file (422, 420): --image-out holds the
    last processed frame's annotated image, so one run per frame (--count 1, then both)."""
    import ros_vision_amd as rva
    from ros_vision_amd import synth
    W, H = 640, 480
    jpgs = [mc.encode(mc.tinted(synth.render_board(W, H, seed=50 + i, ntags=3)[0]), 85, s)
            for i, s in enumerate(("422", "420"))]
    (tmp_path / "cam.mjpg").write_bytes(b"".join(jpgs))
    for count in (1, 2):
        img_out = tmp_path / ("annotated%d.raw" % count)
        r = subprocess.run([os.path.join(NODE, "at_mock_node"), "--mjpg-color", "--width", str(W), "--height", str(H),
                            "--frames", str(tmp_path / "cam.mjpg"), "--count", str(count), "--image-out", str(img_out)],
                           check=True, capture_output=True, text=True, timeout=180)
        recs = [json.loads(l) for l in r.stdout.splitlines()][1:]
        assert len(recs) == count and recs[-1]["status"] == 0 and len(recs[-1]["detections"]) >= 1
        arr = (rva.detector.AtDetection * len(recs[-1]["detections"]))()
        for i, d in enumerate(recs[-1]["detections"]):
            arr[i].id = d["id"]
            for k in range(4):
                arr[i].p[k][0], arr[i].p[k][1] = d["p"][k]
            arr[i].c[0], arr[i].c[1] = d["c"]
        want = _cpu_outlines(nodelib, cc.pil_bgr(jpgs[count - 1]), arr, len(arr))
        got = np.fromfile(img_out, np.uint8).reshape(H, W, 3)
        assert np.array_equal(got, want), int((got != want).any(axis=-1).sum())
    # without the switch nothing is written for an MJPG file, as before
    img_out = tmp_path / "none.raw"
    subprocess.run([os.path.join(NODE, "at_mock_node"), "--width", str(W), "--height", str(H), "--frames",
                    str(tmp_path / "cam.mjpg"), "--count", "1", "--image-out", str(img_out)], check=True,
                   capture_output=True, text=True, timeout=180)
    assert not img_out.exists()
