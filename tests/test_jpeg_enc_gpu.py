"""JPEG output on the GPU: k_jpg_fdct, the entropy-coding kernels and k_jpg_pack encode a device-resident
BGR8 image; at_annotate_jpeg draws the outlines on the staged image and encodes that.

The stream must equal the host encoder's (at_jpeg_encode_host) byte for byte -- the whole
file -- and Pillow's (libjpeg-turbo, one restart interval per MCU row) in every segment
that is no APPn and in the entropy-coded data.  The detection path must not notice."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import jpeg_enc_cases as jc
import mjpg_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(ROOT, "node")
# 3 x 5 blocks: partial MCUs at the right and at the bottom at once, rows of 9 to 12 blocks.
# 41 x 31 blocks: rows of 123 (4:4:4), 84 (4:2:2) and 126 (4:2:0) blocks; 31 intervals at 4:4:4,
# so RSTm wraps.  A row's bit offsets are scanned by 256 lanes, a block each, with a carry from
# chunk to chunk: these rows are one partly filled chunk, the 1080p frame's rows of 720 blocks
# three, and WIDE (344 x 3 blocks: rows of 1032 blocks at 4:4:4 and 4:2:0, 688 at 4:2:2) five
# and three at three rows only, where the detector's smallest height keeps the frame small.
SMALL, MID, WIDE = (24, 40), (328, 248), (2752, 24)


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    return rva


@pytest.fixture(scope="module")
def dets(gpu):
    cache = {}

    def get(w, h):
        if (w, h) not in cache:
            cache[(w, h)] = gpu.GpuDetector(w, h)
        return cache[(w, h)]
    yield get
    for d in cache.values():
        d.close()


@pytest.fixture(scope="module")
def nodelib():
    import fcntl
    from ros_vision_amd import detector
    with open(os.path.join(NODE, ".build.lock"), "w") as lk:   # one make at a time, as tests/test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", NODE, "-s"], check=True)
    detector.load_library()
    return C.CDLL(os.path.join(NODE, "libat_node.so"))


def _device_encode(det, img, quality, sampling, **kw):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    out = det.encode_jpeg_device(dev.data_ptr(), quality, sampling, **kw)
    assert np.array_equal(dev.cpu().numpy(), img)   # the image is only read
    return out


def _check(gpu, det, img, quality, sampling):
    got = _device_encode(det, img, quality, sampling)
    want = gpu.jpeg_encode_host(img, quality, sampling)
    if got != want:
        n = min(len(got), len(want))
        at = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError("GPU stream differs from the host encoder's at byte %d (%d / %d bytes)"
                             % (at, len(got), len(want)))
    jc.assert_same_stream(got, jc.pillow(img, quality, sampling))
    assert jc.decode(got).shape == img.shape
    assert det.jpeg_stats()["bytes"] == len(got)
    return got


@pytest.mark.parametrize("quality", [30, 95])
@pytest.mark.parametrize("sampling", list(jc.SAMPLINGS))
@pytest.mark.parametrize("size", [SMALL, MID])
def test_device_encode_equals_host_and_pillow(gpu, dets, size, sampling, quality):
    for make in (jc.board, jc.primaries, jc.noise):
        _check(gpu, dets(*size), make(*size), quality, sampling)


def test_q100_noise_444(gpu, dets):
    """The longest stream per pixel: stuffing frequent, every buffer nearest its bound."""
    got = _check(gpu, dets(*MID), jc.noise(*MID), 100, "4:4:4")
    assert got.count(b"\xff\x00") > 100 and len(got) > MID[0] * MID[1]
    assert len(got) <= gpu.jpeg_max_bytes(*MID, "4:4:4")


@pytest.mark.parametrize("value", [0, 255])
def test_flat_images(gpu, dets, value):
    """EOB-only blocks: the shortest segments (a 4:2:0 MCU is 24 bits)."""
    for s in jc.SAMPLINGS:
        for size in (SMALL, MID):
            _check(gpu, dets(*size), jc.flat(*size, value), 95, s)


@pytest.mark.parametrize("sampling", ["4:4:4", "4:2:0", "4:2:2"])
def test_wide_rows_take_several_chunks(gpu, dets, sampling):
    """1032 blocks a row at 4:4:4 and 4:2:0 (688 at 4:2:2): several chunks of the row scan."""
    for make in (jc.noise, jc.primaries):
        _check(gpu, dets(*WIDE), make(*WIDE), 95, sampling)


def test_1080p_420(gpu):
    """Rows of 720 blocks, a row of dummy luma blocks, 68 intervals."""
    det = gpu.GpuDetector(1920, 1080)
    _check(gpu, det, jc.board(1920, 1080), 95, "4:2:0")
    det.close()


def _tag_frame(w, h, seed, tag_id):
    gray = mc.board(w, h, seed=seed, ntags=1, ids=[tag_id], side_range=(72, 96))
    return np.ascontiguousarray(mc.tinted(gray)[:, :, ::-1])   # BGR


def _records(d):
    return (d.id, d.hamming, np.float32(d.decision_margin).tobytes(), np.asarray(d.H).tobytes(),
            np.asarray(d.c).tobytes(), np.asarray(d.p).tobytes())


@pytest.mark.parametrize("max_batch", [1, 8])
@pytest.mark.parametrize("source", ["bgr8", "mjpg"])
def test_annotate_jpeg_equals_host_encode_of_annotate_staged(gpu, source, max_batch):
    """Two identically prepared detectors: one publishes raw (annotate_staged), the other
    as JPEG; the bytes are the host encoder's of the raw image.  A frame other than 0 where
    the batch has one.  Detections and poses are the same bytes either way, and so is the
    batch that follows the encode (buffer reuse, stream order)."""
    w, h = MID
    nf = 1 if max_batch == 1 else 3
    frame = nf - 1
    imgs = [_tag_frame(w, h, 3 + i, 17 + i) for i in range(nf)]
    jpgs = [mc.encode(np.ascontiguousarray(im[:, :, ::-1]), 90, "422") for im in imgs]
    a, b = (gpu.GpuDetector(w, h, max_batch=max_batch) for _ in range(2))

    def run(d):
        if source == "bgr8":
            return d.detect_batch(imgs, gpu.AT_FMT_BGR8)
        d.set_mjpg_color(True)
        return d.detect_mjpg_batch(jpgs)

    fa, fb = run(a), run(b)
    assert [d.id for d in fa[frame]] == [17 + frame]
    raw = a.annotate_staged(frame)
    plain = imgs[frame] if source == "bgr8" else gpu.mjpg_decode_bgr(jpgs[frame])
    assert not np.array_equal(raw, plain)           # something was drawn
    got = b.annotate_jpeg(frame, 90, "4:2:0")
    assert got == gpu.jpeg_encode_host(raw, 90, "4:2:0")
    assert jc.decode(got).shape == (h, w, 3)
    for f in range(nf):
        assert [_records(d) for d in fa[f]] == [_records(d) for d in fb[f]]
        assert [(p.id, p.R.tobytes(), p.t.tobytes(), p.err) for p in a.poses(f)] == \
               [(p.id, p.R.tobytes(), p.t.tobytes(), p.err) for p in b.poses(f)]
    with pytest.raises(gpu.JpegError) as e:
        b.annotate_jpeg(nf, 90)                     # not a frame of the batch
    assert e.value.code == -1
    # the next batch through both
    fa2, fb2 = run(a), run(b)
    for f in range(nf):
        assert [_records(d) for d in fa2[f]] == [_records(d) for d in fb2[f]] == [_records(d) for d in fa[f]]
    assert b.annotate_jpeg(frame, 90) == got        # ... and the same image again
    a.close()
    b.close()


def test_gating_and_arguments(gpu):
    from ros_vision_amd import synth
    w, h = MID
    det = gpu.GpuDetector(w, h)
    gray = mc.board(w, h, seed=3, ntags=1, ids=[17], side_range=(72, 96))
    with pytest.raises(gpu.JpegError) as e:
        det.annotate_jpeg(0)                        # no batch at all
    assert e.value.code == -1
    det.detect(synth.to_yuyv(gray))                 # a YUYV batch: no BGR image staged
    with pytest.raises(gpu.JpegError):
        det.annotate_jpeg(0)
    det.detect_mjpg(mc.encode(mc.tinted(gray), 90, "422"))   # colour off: no chroma on the device
    with pytest.raises(gpu.JpegError):
        det.annotate_jpeg(0)
    bgr = _tag_frame(w, h, 3, 17)
    det.detect(bgr, gpu.AT_FMT_BGR8)
    for q, s in [(0, "4:2:0"), (101, "4:2:0"), (50, "4:1:1")]:
        with pytest.raises(gpu.JpegError) as e:
            det.annotate_jpeg(0, q, s)
        assert e.value.code == -1
    with pytest.raises(gpu.JpegError):
        det.annotate_jpeg(1)
    with pytest.raises(gpu.JpegError):
        det.annotate_jpeg(-1)
    assert len(det.annotate_jpeg(0)) > 1000         # the refused calls consumed nothing
    det.close()


def test_short_capacity_leaves_the_guard_alone(gpu, dets):
    import torch
    from ros_vision_amd.detector import AT_E_CAPACITY
    w, h = MID
    det = dets(w, h)
    img = jc.board(w, h)
    want = gpu.jpeg_encode_host(img, 95, "4:2:0")
    dev = torch.from_numpy(img).cuda()
    L = gpu.load_library()
    for cap in (len(want) - 1, 700, 0):
        buf = np.full(cap + 4096, 0xA5, np.uint8)
        n = C.c_size_t(0)
        rc = L.at_encode_jpeg_device(det._h, dev.data_ptr(), 95, 0, buf.ctypes.data, cap, C.byref(n))
        assert rc == AT_E_CAPACITY and n.value == len(want)
        assert np.all(buf[cap:] == 0xA5)
    buf = np.full(len(want) + 4096, 0xA5, np.uint8)
    n = C.c_size_t(0)
    assert L.at_encode_jpeg_device(det._h, dev.data_ptr(), 95, 0, buf.ctypes.data, len(want), C.byref(n)) == 0
    assert buf[:n.value].tobytes() == want and np.all(buf[n.value:] == 0xA5)
    with pytest.raises(gpu.JpegError) as e:
        det.encode_jpeg_device(dev.data_ptr(), 95, "4:2:0", cap=700)
    assert e.value.code == AT_E_CAPACITY and e.value.needed == len(want)


def test_kernel_time_is_reported_only_while_profiling(gpu):
    w, h = MID
    det = gpu.GpuDetector(w, h)
    img = jc.board(w, h)
    _device_encode(det, img, 95, "4:2:0")
    assert det.jpeg_stats()["encode_kernels_ns"] == 0 and det.jpeg_stats()["bytes"] > 0
    det.set_profiling(True)
    _device_encode(det, img, 95, "4:2:0")
    s = det.jpeg_stats()
    print(s)
    assert s["encode_kernels_ns"] > 0
    det.set_profiling(False)
    _device_encode(det, img, 95, "4:2:0")
    assert det.jpeg_stats()["encode_kernels_ns"] == 0
    det.close()


# ---- nodes -----------------------------------------------------------------------
def test_python_node_publishes_the_compressed_image(gpu):
    from ros_vision_amd.node import ApriltagsDetectorNode
    w, h = MID
    bgr = _tag_frame(w, h, 3, 17)
    out = {}
    for jq in (None, 95):
        got = {}
        pubs = {"apriltags/images": lambda m, g=got: g.setdefault("raw", m),
                "apriltags/images/compressed": lambda m, g=got: g.setdefault("jpg", m),
                "camera/pose": lambda m, g=got: g.setdefault("pose", m)}
        node = ApriltagsDetectorNode(w, h, publishers=pubs, image_jpeg=jq)
        res = node.image_callback(bgr, stamp_s=5.0, encoding="bgr8")
        staged = None
        if jq is not None:
            # what at_annotate_staged gives an identically prepared detector
            other = gpu.GpuDetector(w, h, tag_size=gpu.TAG_SIZE)
            other.detect(bgr, gpu.AT_FMT_BGR8)
            staged = other.annotate_staged(0)
            other.close()
        out[jq] = (res, got, staged)
        node.close()
    res, got, staged = out[95]
    assert "raw" not in got and res.image is None
    assert got["jpg"] == res.image_jpeg == gpu.jpeg_encode_host(staged, 95, "4:2:0")
    plain, got_plain, _ = out[None]
    # the default: the payloads the node published before this option existed
    from ros_vision_amd.node import draw_detection_outlines
    d = gpu.GpuDetector(w, h)
    want = draw_detection_outlines(bgr.copy(), d.detect(bgr, gpu.AT_FMT_BGR8))
    d.close()
    assert "jpg" not in got_plain and plain.image_jpeg is None and np.array_equal(got_plain["raw"], want)
    assert got_plain["pose"] == got["pose"] == res.tag_detection_array and len(got["pose"]) == 1


def test_mock_node_jpeg_out(gpu, nodelib, tmp_path):
    """at_mock_node --jpeg-out DIR writes every frame's annotated image as a .jpg: the host
    encoder's bytes of what --image-out holds for the same frame."""
    w, h = MID
    frames = [_tag_frame(w, h, 3 + i, 17 + i) for i in range(2)]
    (tmp_path / "cam.bgr").write_bytes(b"".join(f.tobytes() for f in frames))
    outdir = tmp_path / "jpg"
    r = subprocess.run([os.path.join(NODE, "at_mock_node"), "--width", str(w), "--height", str(h), "--format", "bgr8",
                        "--frames", str(tmp_path / "cam.bgr"), "--count", "2", "--jpeg-out", str(outdir)],
                       check=True, capture_output=True, text=True, timeout=180)
    recs = [json.loads(l) for l in r.stdout.splitlines()][1:]
    assert len(recs) == 2 and all(len(x["detections"]) == 1 for x in recs)
    files = sorted(os.listdir(outdir))
    assert files == ["frame_000000.jpg", "frame_000001.jpg"]
    raw = tmp_path / "last.raw"
    subprocess.run([os.path.join(NODE, "at_mock_node"), "--width", str(w), "--height", str(h), "--format", "bgr8",
                    "--frames", str(tmp_path / "cam.bgr"), "--count", "2", "--image-out", str(raw)],
                   check=True, capture_output=True, text=True, timeout=180)
    last = np.fromfile(raw, np.uint8).reshape(h, w, 3)
    for i, name in enumerate(files):
        jpg = (outdir / name).read_bytes()
        assert jc.decode(jpg).shape == (h, w, 3)
    assert (outdir / files[1]).read_bytes() == gpu.jpeg_encode_host(last, 95, "4:2:0")
