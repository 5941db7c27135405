"""JPEG output, host side (no GPU): at_jpeg_encode_host -- the sequential encoder over the
arithmetic the encode kernels share (csrc/at_mjpg.h) -- against Pillow (libjpeg-turbo)
saving the same image with one restart interval per MCU row.  The target is equality,
byte for byte: every segment that is no APPn, and the entropy-coded data.

Also: rejected arguments, a short buffer, the capacity bound, a stand-alone program built
with the address and undefined-behaviour sanitizers, the ABI version of the compiled C
consumer, and the Python node's image_jpeg option with a stand-in for the detector."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import jpeg_enc_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 3 x 5 blocks (a partial MCU at the right and at the bottom at once), 5 x 3, whole MCUs,
# 41 x 31 blocks (31 intervals at 4:4:4 and 4:2:2: RSTm wraps past 7 three times)
SIZES = [(24, 40), (40, 24), (64, 48), (328, 248)]
QUALITIES = [1, 30, 75, 95, 100]   # the extremes pin the clamp of the table rule (255 and 1)


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


@pytest.fixture(scope="module")
def images():
    out = {}
    for w, h in SIZES:
        out[(w, h)] = {"noise": jc.noise(w, h), "board": jc.board(w, h), "primaries": jc.primaries(w, h)}
    return out


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("sampling", list(jc.SAMPLINGS))
@pytest.mark.parametrize("size", SIZES)
def test_stream_equals_pillow(rva, images, size, sampling, quality):
    for name, img in images[size].items():
        got = rva.jpeg_encode_host(img, quality, sampling)
        jc.assert_same_stream(got, jc.pillow(img, quality, sampling))
        back = jc.decode(got)
        assert back.shape == img.shape, name


def test_1080p_420_equals_pillow(rva):
    """1080 rows are 67.5 MCU rows: a row of dummy luma blocks, 68 restart intervals."""
    img = jc.board(1920, 1080)
    got = rva.jpeg_encode_host(img, 95, "4:2:0")
    jc.assert_same_stream(got, jc.pillow(img, 95, "4:2:0"))
    segs, scan = jc.split(got)
    dri = next(s for m, s in segs if m == 0xDD)
    assert dri[4] * 256 + dri[5] == 120
    assert sum(scan.count(bytes([0xFF, 0xD0 + m])) for m in range(8)) == 67
    assert jc.decode(got).shape == (1080, 1920, 3)


def test_flat_images_are_eob_only(rva):
    """All black, all white: every AC coefficient zero, the shortest segments there are."""
    for value in (0, 255):
        img = jc.flat(64, 48, value)
        for s in jc.SAMPLINGS:
            got = rva.jpeg_encode_host(img, 95, s)
            jc.assert_same_stream(got, jc.pillow(img, 95, s))
            assert np.array_equal(jc.decode(got), img)


def test_header_is_jfif_and_defaults(rva):
    img = jc.noise(64, 48)
    got = rva.jpeg_encode_host(img)
    assert got == rva.jpeg_encode_host(img, 95, "4:2:0")   # OpenCV's defaults
    segs, _ = jc.split(got)
    assert segs[0][0] == 0xE0 and segs[0][1][4:9] == b"JFIF\x00"
    sof = next(s for m, s in segs if m == 0xC0)
    assert sof[4] == 8 and sof[5:9] == bytes([0, 48, 0, 64]) and sof[9] == 3 and sof[11] == 0x22


def _raw(rva, img, quality, sampling, cap, guard=64):
    L = rva.load_library()
    h, w = img.shape[:2]
    buf = np.full(cap + guard, 0xA5, np.uint8)
    n = C.c_size_t(77)
    rc = L.at_jpeg_encode_host(img.ctypes.data, w, h, quality, sampling, buf.ctypes.data, cap, C.byref(n))
    return rc, n.value, buf


def test_rejected_arguments(rva):
    from ros_vision_amd.detector import AT_E_INVALID
    img = jc.noise(64, 48)
    for q, s in [(0, 0), (101, 0), (-5, 2), (50, 3), (50, -1)]:
        rc, n, buf = _raw(rva, img, q, s, 4096)
        assert rc == AT_E_INVALID and n == 0 and np.all(buf == 0xA5)
    L = rva.load_library()
    n = C.c_size_t(77)
    out = np.zeros(4096, np.uint8)
    for w, h in [(60, 48), (64, 44), (0, 48), (64, 0), (65536, 8)]:
        assert L.at_jpeg_encode_host(img.ctypes.data, w, h, 50, 0, out.ctypes.data, out.size, C.byref(n)) == AT_E_INVALID
        assert L.at_jpeg_max_bytes(w, h, 0) == 0
    assert L.at_jpeg_max_bytes(64, 48, 3) == 0
    with pytest.raises(rva.JpegError) as e:
        rva.jpeg_encode_host(img, 95, "4:1:1")
    assert e.value.code == AT_E_INVALID
    with pytest.raises(rva.JpegError):
        rva.jpeg_encode_host(img[:, :, 0])


def test_short_buffer_reports_the_needed_length(rva):
    from ros_vision_amd.detector import AT_E_CAPACITY
    img = jc.board(64, 48)
    want = rva.jpeg_encode_host(img, 75, "4:2:0")
    for cap in (len(want) - 1, 100, 0):
        rc, n, buf = _raw(rva, img, 75, 0, cap)
        assert rc == AT_E_CAPACITY and n == len(want)
        assert np.all(buf[cap:] == 0xA5)          # nothing behind the capacity
    rc, n, buf = _raw(rva, img, 75, 0, len(want))   # the exact size fits
    assert rc == 0 and n == len(want) and buf[:n].tobytes() == want and np.all(buf[n:] == 0xA5)
    with pytest.raises(rva.JpegError) as e:
        rva.jpeg_encode_host(img, 75, "4:2:0", cap=100)
    assert e.value.code == AT_E_CAPACITY and e.value.needed == len(want)


def test_max_bytes_holds_for_q100_noise(rva):
    """The longest stream per pixel: every coefficient non-zero with long codes, 4:4:4."""
    w, h = SIZES[3]
    for s in jc.SAMPLINGS:
        got = rva.jpeg_encode_host(jc.noise(w, h), 100, s)
        assert w * h < len(got) <= rva.jpeg_max_bytes(w, h, s)
    assert rva.jpeg_max_bytes(1920, 1080, "4:2:0") >= 1920 * 1080 * 3 // 2


def test_sanitized_standalone_program(tmp_path):
    """tests/jpeg_enc_host_check.cpp + csrc/at_mjpg.cpp built with the host compiler and
    -fsanitize=address,undefined (the runtimes linked statically), run as a child process:
    edge sizes at every sampling into exact-size and too-small heap buffers, and the round
    trip through the library's own decoder."""
    exe = tmp_path / "jpeg_enc_host_check"
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "jpeg_enc_host_check.cpp"),
                    os.path.join(ROOT, "ros_vision_amd", "csrc", "at_mjpg.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.split()[1]) == 6 * 3 * 2 * 3


def test_abi_version_8_in_the_compiled_consumer(rva):
    """node/abi_check.c (a C11 consumer of include/at_api.h) asserts the version at compile
    time; built as the node tests build it, it reports the library's."""
    import fcntl
    with open(os.path.join(ROOT, "node", ".build.lock"), "w") as lk:   # one make at a time, as test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", os.path.join(ROOT, "node"), "-s"], check=True, timeout=600)
    r =subprocess.run([os.path.join(ROOT, "node", "abi_check"), "layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lay = json.loads(r.stdout)
    assert lay["abi_version"] == lay["library_abi_version"] == rva.load_library().at_abi_version() == 8


# ---- Python node: image_jpeg -----------------------------------------------------
class _StandInDetector:
    """Stands in for GpuDetector where the GPU would be needed: fixed detections, and the
    annotated image either raw or as the host encoder's JPEG of it."""

    IMAGE = None

    def __init__(self, *a, **k):
        self.calls = []

    def detect(self, frame, fmt):
        from ros_vision_amd.detector import Detection
        self.calls.append(("detect", fmt))
        return [Detection(id=3, hamming=0, decision_margin=80.0, H=np.eye(3), c=np.zeros(2),
                          p=np.array([[5.0, 30.0], [30.0, 30.0], [30.0, 5.0], [5.0, 5.0]]))]

    def poses(self, frame=0):
        from ros_vision_amd.detector import Pose
        return [Pose(id=3, R=np.eye(3), t=np.array([0.1, 0.0, 1.5]), err=1e-6)]

    def annotate_staged(self, frame=0):
        self.calls.append(("annotate_staged", frame))
        return self.IMAGE

    def annotate_jpeg(self, frame=0, quality=95, sampling="4:2:0"):
        from ros_vision_amd import jpeg_encode_host
        self.calls.append(("annotate_jpeg", frame, quality, sampling))
        return jpeg_encode_host(self.IMAGE, quality, sampling)

    def close(self):
        pass


def test_node_image_jpeg_host_logic(monkeypatch, rva):
    """image_jpeg=<quality>: the annotated image goes out as JPEG bytes on
    <publish_images_to_topic>/compressed and the raw topic is silent; with the default
    nothing changes."""
    from ros_vision_amd import node as N
    from ros_vision_amd.detector import AT_FMT_BGR8
    monkeypatch.setattr(N, "GpuDetector", _StandInDetector)
    w, h = 64, 48
    _StandInDetector.IMAGE = jc.board(w, h)
    out = {}
    for jq in (None, 90):
        got = {}
        pubs = {"apriltags/images": lambda m, g=got: g.setdefault("raw", m),
                "apriltags/images/compressed": lambda m, g=got: g.setdefault("jpg", m)}
        node = N.ApriltagsDetectorNode(w, h, publishers=pubs, **({} if jq is None else {"image_jpeg": jq}))
        res = node.image_callback(_StandInDetector.IMAGE, stamp_s=3.5, encoding="bgr8")
        out[jq] = (res, got, node.detector.calls)
        node.close()
    res, got, calls = out[None]
    assert calls == [("detect", AT_FMT_BGR8)]   # (a bgr8 frame is outlined on the host copy, as before)
    want = N.draw_detection_outlines(_StandInDetector.IMAGE.copy(), _StandInDetector().detect(None, 0))
    assert "jpg" not in got and np.array_equal(got["raw"], want) and res.image_jpeg is None
    res, got, calls = out[90]
    assert calls == [("detect", AT_FMT_BGR8), ("annotate_jpeg", 0, 90, "4:2:0")]
    assert "raw" not in got and res.image is None
    assert got["jpg"] == res.image_jpeg == rva.jpeg_encode_host(_StandInDetector.IMAGE, 90, "4:2:0")
    assert jc.decode(got["jpg"]).shape == (h, w, 3)
