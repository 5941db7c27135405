"""The preview stream on the GPU: k_preview turns the staged frame of any input format into
the scaled BGR8 image, the draw and JPEG kernels run on it at preview geometry, and the
byte-budget search picks the quality.  Every result must equal the CPU reference
(at_preview_host / at_preview_jpeg_host) bit for bit, and the staged frame, the full-size
JPEG route and the detection path must not notice."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpeg_enc_cases as jc
import mjpg_cases as mc
from preview_cases import make_frame, search_ref, size_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(ROOT, "node")
W, H = 328, 248
SCALES = [1, 2, 3, 4, 8]
SOURCES = ["yuyv", "gray8", "bgr8", "mjpg_luma", "mjpg_color"]
NF, FRAME = 3, 2            # max_batch 3, the frame under test is the last


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    return rva


@pytest.fixture(scope="module")
def nodelib(gpu):
    import fcntl
    with open(os.path.join(NODE, ".build.lock"), "w") as lk:   # one make at a time, as tests/test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", NODE, "-s"], check=True)
    gpu.load_library()
    return C.CDLL(os.path.join(NODE, "libat_node.so"))


def _gray(w, h, i):
    return mc.board(w, h, seed=3 + i, ntags=1, ids=[17 + i], side_range=(72, 96))


def _bgr(w, h, i):
    return np.ascontiguousarray(mc.tinted(_gray(w, h, i))[:, :, ::-1])


def _yuyv(w, h, i):
    """The board as luma, smooth chroma of its own in U and in V: (h, 2 w)."""
    yy, xx = np.mgrid[0:h, 0:w // 2]
    f = np.empty((h, w, 2), np.uint8)
    f[:, :, 0] = _gray(w, h, i)
    f[:, 0::2, 1] = (128 + 100 * np.sin(xx / 11.0 + i) * np.cos(yy / 17.0)).astype(np.uint8)
    f[:, 1::2, 1] = (128 + 110 * np.cos(xx / 7.0) * np.sin(yy / 13.0 + i)).astype(np.uint8)
    return f.reshape(h, 2 * w)


def _batch(gpu, det, source, w=W, h=H, nf=NF):
    """Runs one batch of `source` through `det`; returns per frame (host frame, at_pixfmt) as
    the CPU reference takes it."""
    if source == "yuyv":
        frames = [_yuyv(w, h, i) for i in range(nf)]
        det.detect_batch(frames, gpu.AT_FMT_YUYV)
        return [(f, gpu.AT_FMT_YUYV) for f in frames]
    if source == "gray8":
        frames = [_gray(w, h, i) for i in range(nf)]
        det.detect_batch(frames, gpu.AT_FMT_GRAY8)
        return [(f, gpu.AT_FMT_GRAY8) for f in frames]
    if source == "bgr8":
        frames = [_bgr(w, h, i) for i in range(nf)]
        det.detect_batch(frames, gpu.AT_FMT_BGR8)
        return [(f, gpu.AT_FMT_BGR8) for f in frames]
    jpgs = [mc.encode(mc.tinted(_gray(w, h, i)), 90, ("422", "420", "444")[i % 3]) for i in range(nf)]
    det.set_mjpg_color(source == "mjpg_color")
    det.detect_mjpg_batch(jpgs)
    if source == "mjpg_color":
        return [(gpu.mjpg_decode_bgr(j), gpu.AT_FMT_BGR8) for j in jpgs]
    return [(gpu.mjpg_decode_gray(j), gpu.AT_FMT_GRAY8) for j in jpgs]


def _boxes(gpu, w=W, h=H):
    return np.array([(w / 2, h / 2, 90.5, 60.25, 0.9, 1), (10, 12, 70, 50, 0.8, 3)], gpu.GP_BOX_DTYPE)


@pytest.mark.parametrize("source", SOURCES)
def test_preview_bgr_equals_the_host_reference(gpu, source):
    det = gpu.GpuDetector(W, H, max_batch=NF)
    try:
        host = _batch(gpu, det, source)
        recs = det._frame_records(FRAME)
        assert [r.id for r in recs] == [17 + FRAME]
        boxes = _boxes(gpu)
        for frame in (FRAME, 1):
            fr, fmt = host[frame]
            for s in SCALES:
                got = det.preview_bgr(frame, s, boxes=boxes)
                want = gpu.preview_host(fr, fmt, s, detections=det._frame_records(frame), boxes=boxes)
                assert got.shape == want.shape == size_ref(W, H, s)[1::-1] + (3,)
                assert np.array_equal(got, want), (source, frame, s, int((got != want).any(axis=2).sum()))
                plain = gpu.preview_host(fr, fmt, s)
                assert (want != plain).any()                        # something was drawn
                st = det.preview_stats()
                assert (st["bytes"], st["encodes"], st["width"], st["height"]) == (want.size, 0) + want.shape[1::-1]
        # without records the image is the plain preview
        assert np.array_equal(det.preview_bgr(FRAME, 3, detections=[]), gpu.preview_host(*host[FRAME], 3))
    finally:
        det.close()


@pytest.fixture(scope="module")
def bgr_det(gpu):
    """One detector with a host BGR8 batch staged, shared by the tests that only read it."""
    det = gpu.GpuDetector(W, H, max_batch=NF)
    host = _batch(gpu, det, "bgr8")
    yield det, host
    det.close()


@pytest.mark.parametrize("sampling", ["4:2:0", "4:2:2", "4:4:4"])
def test_preview_jpeg_equals_the_host_reference(gpu, bgr_det, sampling):
    det, host = bgr_det
    boxes = _boxes(gpu)
    for s in (2, 3):
        got, used = det.preview_jpeg(FRAME, s, quality=70, sampling=sampling, boxes=boxes)
        want, want_used = gpu.preview_jpeg_host(*host[FRAME], s, detections=det._frame_records(FRAME), boxes=boxes,
                                                quality=70, sampling=sampling)
        assert used == want_used == 70 and got == want
        pw, ph = size_ref(W, H, s)[:2]
        assert jc.decode(got).shape == (ph, pw, 3)
        st = det.preview_stats()
        assert (st["bytes"], st["quality_used"], st["encodes"], st["width"], st["height"]) == (len(got), 70, 1, pw, ph)


def test_byte_budget(gpu):
    """The budget case of the CPU test: 328 x 248 noise at s = 2."""
    det = gpu.GpuDetector(W, H, max_batch=NF)
    try:
        noise = make_frame("bgr8", W, H, seed=77)
        det.detect_batch([_bgr(W, H, 0), noise], gpu.AT_FMT_BGR8)
        recs = det._frame_records(1)
        img = gpu.preview_host(noise, gpu.AT_FMT_BGR8, 2, detections=recs)
        size = {q: len(gpu.jpeg_encode_host(img, q, "4:2:0")) for q in (1, 90)}
        used_seen = set()
        for q0, budget in [(90, size[90]), (90, size[90] - 1), (90, (size[1] + size[90]) // 2), (50, size[90] // 3),
                           (90, size[1] + 40), (90, size[1])]:
            want, want_q, runs = search_ref(lambda q: gpu.jpeg_encode_host(img, q, "4:2:0"), q0, budget)
            hjpg, hq = gpu.preview_jpeg_host(noise, gpu.AT_FMT_BGR8, 2, detections=recs, quality=q0, max_bytes=budget)
            got, used = det.preview_jpeg(1, 2, quality=q0, max_bytes=budget)
            assert (used, got) == (hq, hjpg) == (want_q, want) and len(got) <= budget
            st = det.preview_stats()
            assert (st["bytes"], st["quality_used"], st["encodes"]) == (len(got), used, runs)
            used_seen.add(used)
        # (quality 1 and 2 quantise alike -- every divisor clamps to 255 -- so the tightest budget ends at 2)
        assert len(used_seen) >= 4 and min(used_seen) <= 2 and 90 in used_seen
        # impossible: below the header's size
        _, _, runs = search_ref(lambda q: gpu.jpeg_encode_host(img, q, "4:2:0"), 90, 100)
        with pytest.raises(gpu.JpegError) as e:
            det.preview_jpeg(1, 2, quality=90, max_bytes=100)
        assert e.value.code == -3 and e.value.quality_used == 1 and e.value.needed == size[1]
        assert det.preview_stats()["encodes"] == runs
        # a small cap: the size needed, nothing written beyond (the guard bytes stay)
        L = gpu.load_library()
        plain = len(gpu.jpeg_encode_host(gpu.preview_host(noise, gpu.AT_FMT_BGR8, 2), 90, "4:2:0"))
        for cap in (plain - 1, 64, 0):
            buf = np.full(cap + 4096, 0xA5, np.uint8)
            n, qu = C.c_size_t(), C.c_int()
            rc = L.at_preview_jpeg(det._h, 1, 2, None, 0, None, 0, 90, 0, 0, buf.ctypes.data, cap, C.byref(n),
                                   C.byref(qu))
            assert rc == -3 and qu.value == 90 and (buf == 0xA5).all()
            assert n.value == plain
        with pytest.raises(gpu.JpegError) as e:
            det.preview_jpeg(1, 2, quality=90, cap=64)
        assert e.value.code == -3 and e.value.quality_used == 90
    finally:
        det.close()


def _records(d):
    return (d.id, d.hamming, np.float32(d.decision_margin).tobytes(), np.asarray(d.H).tobytes(),
            np.asarray(d.c).tobytes(), np.asarray(d.p).tobytes())


def test_the_source_is_untouched(gpu):
    """annotate_staged after preview calls is what it is without them, and so is the next batch."""
    a, b = (gpu.GpuDetector(W, H, max_batch=NF) for _ in range(2))
    try:
        frames = [_bgr(W, H, i) for i in range(NF)]
        fa, fb = (d.detect_batch(frames, gpu.AT_FMT_BGR8) for d in (a, b))
        for s in SCALES:
            b.preview_bgr(FRAME, s, boxes=_boxes(gpu))
        b.preview_jpeg(FRAME, 2, quality=90, max_bytes=3000)
        assert np.array_equal(a.annotate_staged(FRAME), b.annotate_staged(FRAME))
        # the preview after the annotation shows the annotated frame: the staged copy is what is read
        assert np.array_equal(b.preview_bgr(FRAME, 1, detections=[]), a.annotate_staged(FRAME))
        fa2, fb2 = (d.detect_batch(frames, gpu.AT_FMT_BGR8) for d in (a, b))
        for f in range(NF):
            assert [_records(d) for d in fa[f]] == [_records(d) for d in fb[f]] == [_records(d) for d in fa2[f]] \
                == [_records(d) for d in fb2[f]]
    finally:
        a.close()
        b.close()


def test_header_cache_is_keyed_by_geometry(gpu):
    det = gpu.GpuDetector(W, H, max_batch=NF)
    try:
        host = _batch(gpu, det, "bgr8")
        recs = det._frame_records(FRAME)
        p2, _ = det.preview_jpeg(FRAME, 2, quality=80)
        full = det.annotate_jpeg(FRAME, 80, "4:2:0")            # same quality and sampling, another size
        p4, _ = det.preview_jpeg(FRAME, 4, quality=80, detections=recs)
        staged = det.preview_bgr(FRAME, 1, detections=[])       # (the staged frame as the annotation left it)
        assert jc.decode(p2).shape == size_ref(W, H, 2)[1::-1] + (3,)
        assert jc.decode(full).shape == (H, W, 3)
        assert jc.decode(p4).shape == size_ref(W, H, 4)[1::-1] + (3,)
        assert p2 == gpu.preview_jpeg_host(*host[FRAME], 2, detections=recs, quality=80)[0]
        assert full == gpu.jpeg_encode_host(staged, 80, "4:2:0")
        other = gpu.GpuDetector(W, H, max_batch=NF)
        other.detect_batch([h[0] for h in host], gpu.AT_FMT_BGR8)
        assert np.array_equal(staged, other.annotate_staged(FRAME))
        other.close()
        assert p4 == gpu.preview_jpeg_host(staged, gpu.AT_FMT_BGR8, 4, detections=recs, quality=80)[0]
    finally:
        det.close()


def test_gating_and_the_device_entry(gpu):
    import torch
    det = gpu.GpuDetector(W, H, max_batch=NF)
    small = gpu.GpuDetector(24, 40)
    try:
        with pytest.raises(gpu.JpegError) as e:
            det.preview_jpeg(0, 2)                              # no batch at all
        assert e.value.code == -1
        frames = [_yuyv(W, H, i) for i in range(NF)]
        dev = torch.from_numpy(np.stack(frames)).cuda()
        det.enqueue_device(dev.data_ptr(), frames[0].size, NF, gpu.AT_FMT_YUYV)
        det.collect()
        recs = det._frame_records(1)
        assert [r.id for r in recs] == [18]
        for call in (lambda: det.preview_jpeg(1, 2), lambda: det.preview_bgr(1, 2)):
            with pytest.raises(gpu.JpegError) as e:
                call()                                          # not host-fed: nothing staged
            assert e.value.code == -1
        ptr = dev.data_ptr() + frames[0].size
        got, used = det.preview_jpeg_device(ptr, gpu.AT_FMT_YUYV, 2, quality=60, detections=recs, boxes=_boxes(gpu))
        assert (got, used) == gpu.preview_jpeg_host(frames[1], gpu.AT_FMT_YUYV, 2, detections=recs,
                                                    boxes=_boxes(gpu), quality=60)
        assert np.array_equal(dev.cpu().numpy(), np.stack(frames))
        for bad in (0, ptr + 4):
            with pytest.raises(gpu.JpegError) as e:
                det.preview_jpeg_device(bad, gpu.AT_FMT_YUYV, 2)
            assert e.value.code == -1
        det.detect_batch(frames, gpu.AT_FMT_YUYV)               # host-fed now
        for s in (0, 9, -1):
            with pytest.raises(gpu.JpegError) as e:
                det.preview_jpeg(1, s)
            assert e.value.code == -1
        for frame in (-1, NF):
            with pytest.raises(gpu.JpegError) as e:
                det.preview_jpeg(frame, 2)
            assert e.value.code == -1
        for kw in ({"quality": 0}, {"quality": 101}, {"sampling": "4:1:1"}):
            with pytest.raises(gpu.JpegError) as e:
                det.preview_jpeg(1, 2, **kw)
            assert e.value.code == -1
        assert det.preview_jpeg(1, 2)[1] == 50                  # the refused calls changed nothing
        small.detect(np.zeros((40, 24), np.uint8), gpu.AT_FMT_GRAY8)
        assert small.preview_bgr(0, 1).shape == (40, 24, 3) and small.preview_bgr(0, 3).shape == (8, 8, 3)
        with pytest.raises(gpu.JpegError) as e:
            small.preview_jpeg(0, 4)                            # 24 // 4 = 6: no preview under 8 x 8
        assert e.value.code == -1
    finally:
        det.close()
        small.close()


def test_1080p_yuyv_at_scale_4(gpu):
    w, h = 1920, 1080
    det = gpu.GpuDetector(w, h)
    try:
        frame = make_frame("yuyv", w, h, seed=4).reshape(h, 2 * w)
        frame[:, 0::2] = mc.board(w, h, seed=766, ntags=4)      # real tags in the luma, noise in the chroma
        det.detect(frame, gpu.AT_FMT_YUYV)
        recs = det._frame_records(0)
        assert len(recs) >= 1
        got = det.preview_bgr(0, 4)
        assert got.shape == (264, 480, 3)
        assert np.array_equal(got, gpu.preview_host(frame, gpu.AT_FMT_YUYV, 4, detections=recs))
        jpg, used = det.preview_jpeg(0, 4, quality=50, max_bytes=20000)
        assert (jpg, used) == gpu.preview_jpeg_host(frame, gpu.AT_FMT_YUYV, 4, detections=recs, quality=50,
                                                    max_bytes=20000)
        assert len(jpg) <= 20000
    finally:
        det.close()


def test_kernel_time_only_while_profiling(gpu, bgr_det):
    det, _ = bgr_det
    det.preview_jpeg(FRAME, 2)
    assert det.preview_stats()["kernels_ns"] == 0
    det.set_profiling(True)
    det.preview_jpeg(FRAME, 2)
    s = det.preview_stats()
    print(s)
    det.set_profiling(False)
    assert s["kernels_ns"] > 0
    det.preview_bgr(FRAME, 2)
    assert det.preview_stats()["kernels_ns"] == 0


# ---- nodes -----------------------------------------------------------------------------------
def _node_frames(gpu):
    gray = _gray(W, H, 0)
    return {"yuyv": (_yuyv(W, H, 0), gpu.AT_FMT_YUYV), "mono8": (gray, gpu.AT_FMT_GRAY8),
            "jpeg": (mc.encode(mc.tinted(gray), 90, "422"), None), "bgr8": (_bgr(W, H, 0), gpu.AT_FMT_BGR8)}


@pytest.mark.parametrize("encoding", ["yuyv", "mono8", "jpeg", "bgr8"])
def test_python_node_publishes_a_preview_for_every_encoding(gpu, encoding):
    from ros_vision_amd.node import ApriltagsDetectorNode
    image, fmt = _node_frames(gpu)[encoding]
    got = {}
    pubs = {"apriltags/images/preview/compressed": lambda m: got.setdefault("preview", m),
            "apriltags/images": lambda m: got.setdefault("raw", m), "camera/pose": lambda m: got.setdefault("pose", m)}
    node = ApriltagsDetectorNode(W, H, publishers=pubs, preview_scale=2, preview_quality=60)
    try:
        res = node.image_callback(image, stamp_s=5.0, encoding=encoding)
        recs = node.detector._frame_records(0)
        assert [r.id for r in recs] == [17]
        host, hfmt = (gpu.mjpg_decode_gray(image), gpu.AT_FMT_GRAY8) if encoding == "jpeg" else (image, fmt)
        want, _ = gpu.preview_jpeg_host(host, hfmt, 2, detections=recs, quality=60)
        assert got["preview"] == res.preview_jpeg == want
        assert jc.decode(want).shape == size_ref(W, H, 2)[1::-1] + (3,)
        assert ("raw" in got) == (encoding == "bgr8") and len(got["pose"]) == 1
        # a budget nothing meets: no preview, everything else as before
        node.preview_max_bytes = 100
        got.clear()
        res = node.image_callback(image, stamp_s=6.0, encoding=encoding)
        assert res.preview_jpeg is None and "preview" not in got and len(got["pose"]) == 1
    finally:
        node.close()
    off = ApriltagsDetectorNode(W, H, publishers=pubs)           # the default: no preview work
    try:
        got.clear()
        assert off.image_callback(image, stamp_s=5.0, encoding=encoding).preview_jpeg is None and "preview" not in got
        assert off.detector.preview_stats()["encodes"] == 0
    finally:
        off.close()


@pytest.mark.parametrize("fmt_name", ["yuyv", "gray", "mjpg"])
def test_mock_node_preview_out_equals_the_python_route(gpu, nodelib, tmp_path, fmt_name):
    from ros_vision_amd.node import ApriltagsDetectorNode
    key = {"yuyv": "yuyv", "gray": "mono8", "mjpg": "jpeg"}[fmt_name]
    frames = []
    for i in range(2):
        gray = _gray(W, H, i)
        frames.append({"yuyv": _yuyv(W, H, i), "gray": gray}.get(fmt_name) if fmt_name != "mjpg"
                      else mc.encode(mc.tinted(gray), 90, "422"))
    blob = b"".join(f if isinstance(f, bytes) else f.tobytes() for f in frames)
    path = tmp_path / ("cam.mjpg" if fmt_name == "mjpg" else "cam.raw")
    path.write_bytes(blob)
    outdir = tmp_path / "pv"
    subprocess.run([os.path.join(NODE, "at_mock_node"), "--width", str(W), "--height", str(H), "--format", fmt_name,
                    "--frames", str(path), "--count", "2", "--preview-out", str(outdir), "--preview-scale", "2",
                    "--preview-quality", "60", "--preview-max-bytes", "4000"],
                   check=True, capture_output=True, text=True, timeout=180)
    assert sorted(os.listdir(outdir)) == ["preview_000000.jpg", "preview_000001.jpg"]
    node = ApriltagsDetectorNode(W, H, preview_scale=2, preview_quality=60, preview_max_bytes=4000)
    try:
        for i, f in enumerate(frames):
            res = node.image_callback(f, stamp_s=1.0, encoding=key)
            jpg = (outdir / ("preview_%06d.jpg" % i)).read_bytes()
            assert jpg == res.preview_jpeg and len(jpg) <= 4000
            assert jc.decode(jpg).shape == size_ref(W, H, 2)[1::-1] + (3,)
    finally:
        node.close()


def test_game_piece_node_preview_carries_the_boxes(gpu):
    import gp_parse_cases as gc
    from ros_vision_amd.node import GamePieceDetectorNode
    import torch
    w, h = 640, 480
    raw = gc.generate(8400, 3, 12, seed=31)
    frame = np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = torch.from_numpy(raw[None]).cuda()
    sent = {}
    node = GamePieceDetectorNode(w, h, lambda x: out.clone(), class_names=["coral", "algae", "robot"],
                                 preview_scale=2, preview_quality=60,
                                 publishers={"game_piece_detector/images/preview/compressed":
                                             lambda m: sent.setdefault("preview", m),
                                             "game_piece_detector/images": lambda m: sent.setdefault("image", m)})
    try:
        res = node.image_callback(frame, 1.0)
        boxes = gc.checked(raw, orig=(w, h))
        assert len(res.boxes) == len(boxes) > 0
        want, _ = gpu.preview_jpeg_host(frame, gpu.AT_FMT_BGR8, 2, boxes=boxes, quality=60)
        assert sent["preview"] == res.preview_jpeg == want
        assert want != gpu.preview_jpeg_host(frame, gpu.AT_FMT_BGR8, 2, quality=60)[0]       # the boxes are on it
        assert res.image is not None and (res.image != frame).any()                         # the full image as before
    finally:
        node.close()
