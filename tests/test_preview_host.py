"""The preview stream on the CPU (no GPU): at_preview_size, at_preview_host,
at_preview_jpeg_host -- the reference the device path is held to bit for bit.

Everything is integer arithmetic restated here in numpy from the definition in
include/at_api.h, so every comparison is exact.  The YUYV constants are the library's own
definition: equality with cv::cvtColor is not tested anywhere (no OpenCV here)."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from preview_cases import make_frame, search_ref, size_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(ROOT, "node")
ODD, SMALL = (328, 248), (72, 56)
SCALES = [1, 2, 3, 4, 8]
FMTS = ["bgr8", "gray8", "yuyv"]


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


@pytest.fixture(scope="module")
def nodelib(rva):
    import fcntl
    with open(os.path.join(NODE, ".build.lock"), "w") as lk:   # one make at a time, as tests/test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", NODE, "-s"], check=True)
    rva.load_library()
    L = C.CDLL(os.path.join(NODE, "libat_node.so"))
    L.at_node_draw_detection_outlines.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.at_node_draw_detection_outlines.restype = None
    L.at_node_draw_boxes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.at_node_draw_boxes.restype = None
    return L


# ---- the definition, restated -------------------------------------------------------
def yuyv_to_bgr(frame):
    """(H, W, 2) YUYV -> (H, W, 3) BGR, int64 arithmetic (floor shifts)."""
    f = frame.astype(np.int64)
    Y = f[:, :, 0]
    U = np.repeat(f[:, 0::2, 1], 2, axis=1) - 128
    V = np.repeat(f[:, 1::2, 1], 2, axis=1) - 128
    y = np.maximum(0, Y - 16) * 1220542 + (1 << 19)
    r = (y + 1673527 * V) >> 20
    g = (y - 852492 * V - 409993 * U) >> 20
    b = (y + 2116026 * U) >> 20
    return np.clip(np.stack([b, g, r], -1), 0, 255)


def to_bgr(frame, fmt):
    if fmt == "bgr8":
        return frame.astype(np.int64)
    if fmt == "gray8":
        return np.repeat(frame.astype(np.int64)[:, :, None], 3, axis=2)
    return yuyv_to_bgr(frame)


def preview_ref(frame, fmt, s):
    bgr = to_bgr(frame, fmt)
    h, w = bgr.shape[:2]
    pw, ph, ox, oy = size_ref(w, h, s)
    box = bgr[oy:oy + ph * s, ox:ox + pw * s].reshape(ph, s, pw, s, 3).sum((1, 3))
    return ((box + (s * s) // 2) // (s * s)).astype(np.uint8)


def fmt_code(rva, fmt):
    return {"bgr8": rva.AT_FMT_BGR8, "gray8": rva.AT_FMT_GRAY8, "yuyv": rva.AT_FMT_YUYV}[fmt]


def det_at(rva, tag_id, cx, cy, half):
    sx, sy = (-1, 1, 1, -1), (1, 1, -1, -1)
    return rva.Detection(id=tag_id, hamming=0, decision_margin=50.0, H=np.eye(3), c=np.array([cx, cy], float),
                         p=np.array([[cx + sx[k] * half, cy + sy[k] * half] for k in range(4)], float))


def records(rva, w, h):
    """A tag inside, one across the left / top edge of every crop, one beyond the right / bottom
    edge, one far outside; a box inside, one across the corner, one clamped on every side."""
    dets = [det_at(rva, 7, w / 2 + 0.4, h / 2 - 0.3, 20.5), det_at(rva, 123, 3.0, 5.0, 30.0),
            det_at(rva, 586, w - 2.0, h - 1.0, 25.0), det_at(rva, 1, -5000.0, 1e7, 40.0)]
    boxes = np.array([(w / 2, h / 2, 50.5, 30.25, 0.9, 0), (-10, -10, 60, 60, 0.8, 7), (w, h, 1e9, 40, 0.7, -3),
                      (w / 3, h / 3, 21, 33, 0.6, 2)], rva.GP_BOX_DTYPE)
    return dets, boxes


def mapped(rva, dets, boxes, s, ox, oy):
    """The records in preview coordinates: (p - o) / s in double, boxes in float32."""
    from ros_vision_amd.detector import _detection_records
    md = [rva.Detection(id=d.id, hamming=d.hamming, decision_margin=d.decision_margin, H=d.H,
                        c=(np.asarray(d.c) - (ox, oy)) / s, p=(np.asarray(d.p) - (ox, oy)) / s) for d in dets]
    mb = boxes.copy()
    f = np.float32
    mb["x"] = (boxes["x"] - f(ox)) / f(s)
    mb["y"] = (boxes["y"] - f(oy)) / f(s)
    mb["w"] = boxes["w"] / f(s)
    mb["h"] = boxes["h"] / f(s)
    assert mb["x"].dtype == np.float32
    return _detection_records(md), mb


# ---- geometry ---------------------------------------------------------------------------
def test_preview_size_of_the_deployed_geometries(rva):
    assert rva.preview_size(1920, 1080, 4) == (480, 264, 0, 12)
    assert rva.preview_size(1280, 800, 4) == (320, 200, 0, 0)
    assert rva.preview_size(640, 480, 2) == (320, 240, 0, 0)
    for w, h in [(1920, 1080), (1280, 800), (1280, 720), (640, 480)]:
        for s in range(1, 9):
            pw, ph, ox, oy = rva.preview_size(w, h, s)
            assert (pw, ph, ox, oy) == size_ref(w, h, s)
            assert pw % 8 == 0 and ph % 8 == 0 and 0 <= ox and ox + pw * s <= w and 0 <= oy and oy + ph * s <= h
    assert rva.preview_size(1920, 1080, 1) == (1920, 1080, 0, 0)   # s = 1: convert only


def test_preview_size_rejects(rva):
    for w, h, s in [(640, 480, 0), (640, 480, 9), (640, 480, -1), (72, 56, 8), (56, 72, 8), (7, 7, 1), (0, 0, 1)]:
        with pytest.raises(rva.JpegError) as e:
            rva.preview_size(w, h, s)
        assert e.value.code == -1


# ---- the image ----------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("size", [ODD, SMALL])
def test_preview_equals_the_definition(rva, size, fmt, s):
    w, h = size
    pw, ph, ox, oy = size_ref(w, h, s)
    if pw < 8 or ph < 8:
        with pytest.raises(rva.JpegError):
            rva.preview_host(make_frame(fmt, w, h), fmt_code(rva, fmt), s)
        return
    if size == ODD and s > 1:
        assert ox > 0 and oy > 0          # every one of these scales crops on both axes
    frame = make_frame(fmt, w, h, seed=s)
    before = frame.copy()
    got = rva.preview_host(frame, fmt_code(rva, fmt), s)
    assert got.shape == (ph, pw, 3) and np.array_equal(got, preview_ref(frame, fmt, s))
    assert np.array_equal(frame, before)
    if fmt == "yuyv":                     # the flat (H, 2 W) layout is the same frame
        assert np.array_equal(rva.preview_host(frame.reshape(h, 2 * w), fmt_code(rva, fmt), s), got)


def test_yuyv_spot_values(rva):
    def px(Y, U, V):
        f = np.empty((8, 8, 2), np.uint8)
        f[:, :, 0] = Y
        f[:, 0::2, 1] = U
        f[:, 1::2, 1] = V
        out = rva.preview_host(f, rva.AT_FMT_YUYV, 1)
        assert (out == out[0, 0]).all()
        return tuple(int(v) for v in out[0, 0])    # B, G, R

    assert px(16, 128, 128) == (0, 0, 0)
    assert px(235, 128, 128) == (255, 255, 255)
    assert px(126, 128, 128) == (128, 128, 128)
    assert px(255, 255, 255) == (255, 125, 255)    # G = (292233826 - 160335595) >> 20; B, R saturate at 255
    assert px(255, 255, 255) == tuple(int(v) for v in yuyv_to_bgr(np.array([[[255, 255], [255, 255]]], np.uint8))[0, 0])
    assert px(0, 0, 0) == (0, 154, 0)              # B, R saturate at 0
    assert px(0, 0, 0) == tuple(int(v) for v in yuyv_to_bgr(np.array([[[0, 0], [0, 0]]], np.uint8))[0, 0])
    # pixel x takes the U and V of its pair: one pair with colour in a gray row
    f = np.full((8, 8, 2), 128, np.uint8)
    f[0, 2, 1], f[0, 3, 1] = 60, 200
    out = rva.preview_host(f, rva.AT_FMT_YUYV, 1)
    assert np.array_equal(out[0, 2], out[0, 3]) and not np.array_equal(out[0, 2], out[0, 1])
    assert np.array_equal(out[0, 1], out[0, 4]) and np.array_equal(out, yuyv_to_bgr(f).astype(np.uint8))


# ---- annotations ----------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("fmt", ["bgr8", "yuyv"])
def test_annotations_equal_the_node_drawing_of_the_mapped_records(rva, nodelib, fmt, s):
    w, h = ODD
    pw, ph, ox, oy = size_ref(w, h, s)
    frame = make_frame(fmt, w, h, seed=40 + s)
    dets, boxes = records(rva, w, h)
    got = rva.preview_host(frame, fmt_code(rva, fmt), s, detections=dets, boxes=boxes)
    want = rva.preview_host(frame, fmt_code(rva, fmt), s)
    plain = want.copy()
    (arr, n), mb = mapped(rva, dets, boxes, s, ox, oy)
    nodelib.at_node_draw_boxes(want.ctypes.data, pw, ph, mb.ctypes.data, len(mb))                # boxes first
    nodelib.at_node_draw_detection_outlines(want.ctypes.data, pw, ph, C.addressof(arr), n)       # tags on top
    assert np.array_equal(got, want)
    changed = (got != plain).any(axis=2)
    assert changed.sum() > 200
    # clipped, not wrapped: the tag across the left edge leaves the right-hand columns alone
    # wherever nothing else was drawn
    only = rva.preview_host(frame, fmt_code(rva, fmt), s, detections=[dets[1]])
    ys, xs = np.nonzero((only != plain).any(axis=2))
    # its sides end at the mapped corners, its three glyphs (17.5 px apart, 20 px tall: fixed) around the centre
    mp, mc = (np.asarray(dets[1].p) - (ox, oy)) / s, (np.asarray(dets[1].c) - (ox, oy)) / s
    xmax, ymax = max(mp[:, 0].max(), mc[0] + 47.5 / 2) + 2, max(mp[:, 1].max(), mc[1] + 10) + 2
    assert len(xs) > 0 and xs.min() == 0 and ys.min() == 0 and xs.max() <= xmax and ys.max() <= ymax
    if s <= 2:
        assert xs.max() < pw // 2 and ys.max() < ph // 2
    far = rva.preview_host(frame, fmt_code(rva, fmt), s, detections=[dets[3]])
    assert np.array_equal(far, plain)


def test_lines_stay_two_pixels_and_glyphs_keep_their_size(rva):
    """Mapping happens before the segments are built: a horizontal side is as thick at s = 4
    as at s = 1, and the id's glyphs span the same pixels."""
    w, h = ODD
    frame = np.zeros((h, w), np.uint8)
    thick, glyph = [], []
    for s in (1, 4):
        pw, ph, ox, oy = size_ref(w, h, s)
        d = det_at(rva, 8, w / 2.0, h / 2.0, 96.0)   # (its sides clear of the glyph at either scale)
        out = rva.preview_host(frame, rva.AT_FMT_GRAY8, s, detections=[d])
        cx = int((w / 2.0 - ox) / s)
        col = out[:, cx].any(axis=1)
        top = np.nonzero(col)[0][0]
        thick.append(int(col[top:top + 6].sum()))
        text = (out == (255, 153, 0)).all(axis=2)
        ys, xs = np.nonzero(text)
        glyph.append((int(ys.max() - ys.min()), int(xs.max() - xs.min())))
    assert thick[0] == thick[1] and glyph[0] == glyph[1], (thick, glyph)


# ---- JPEG and the byte budget ---------------------------------------------------------------
def _decode(jpg):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))


@pytest.mark.parametrize("sampling", ["4:2:0", "4:2:2", "4:4:4"])
@pytest.mark.parametrize("fmt", FMTS)
def test_jpeg_is_the_host_encode_of_the_preview(rva, fmt, sampling):
    w, h = ODD
    frame = make_frame(fmt, w, h, seed=9)
    dets, boxes = records(rva, w, h)
    for s in (1, 3):
        img = rva.preview_host(frame, fmt_code(rva, fmt), s, detections=dets, boxes=boxes)
        jpg, used = rva.preview_jpeg_host(frame, fmt_code(rva, fmt), s, detections=dets, boxes=boxes, quality=70,
                                          sampling=sampling)
        assert used == 70 and jpg == rva.jpeg_encode_host(img, 70, sampling)
        assert _decode(jpg).shape == img.shape


@pytest.fixture(scope="module")
def budget_case(rva):
    """328 x 248 noise at s = 2: the preview, its size at q 90 and at q 1."""
    w, h = ODD
    frame = make_frame("bgr8", w, h, seed=77)
    img = rva.preview_host(frame, rva.AT_FMT_BGR8, 2)
    sizes = {q: len(rva.jpeg_encode_host(img, q, "4:2:0")) for q in (1, 90)}
    return frame, img, sizes


def test_budget_search_equals_the_rule(rva, budget_case):
    frame, img, sizes = budget_case
    assert sizes[1] < sizes[90] // 3
    budgets = [sizes[90], sizes[90] - 1, (sizes[1] + sizes[90]) // 2, sizes[90] // 3, sizes[1] + 40, sizes[1]]
    seen = set()
    for q0 in (90, 50, 2, 1):
        for budget in budgets:
            want, want_q, runs = search_ref(lambda q: rva.jpeg_encode_host(img, q, "4:2:0"), q0, budget)
            assert runs <= 2 + int(np.ceil(np.log2(max(q0 - 1, 1))))
            if want is None:
                with pytest.raises(rva.JpegError) as e:
                    rva.preview_jpeg_host(frame, rva.AT_FMT_BGR8, 2, quality=q0, max_bytes=budget)
                assert e.value.code == -3 and e.value.quality_used == 1 and e.value.needed == sizes[1]
                continue
            jpg, used = rva.preview_jpeg_host(frame, rva.AT_FMT_BGR8, 2, quality=q0, max_bytes=budget)
            assert used == want_q and jpg == want and len(jpg) <= budget
            assert jpg == rva.jpeg_encode_host(img, used, "4:2:0")
            seen.add(used)
    assert len(seen) >= 5 and 1 in seen and 90 in seen      # first try, bisection and quality 1 all occurred
    jpg, used = rva.preview_jpeg_host(frame, rva.AT_FMT_BGR8, 2, quality=90, max_bytes=0)
    assert used == 90 and len(jpg) == sizes[90]


def test_budget_below_the_header_is_capacity(rva, budget_case):
    frame, img, sizes = budget_case
    with pytest.raises(rva.JpegError) as e:
        rva.preview_jpeg_host(frame, rva.AT_FMT_BGR8, 2, quality=90, max_bytes=100)
    assert e.value.code == -3 and e.value.quality_used == 1 and e.value.needed == sizes[1]
    # `cap` too small for a stream the budget admits: the size needed, nothing written
    L = rva.load_library()
    out = np.full(4096, 0xA5, np.uint8)
    n, qu = C.c_size_t(), C.c_int()
    rc = L.at_preview_jpeg_host(frame.ctypes.data, rva.AT_FMT_BGR8, ODD[0], ODD[1], 2, None, 0, None, 0, 90, 0,
                                sizes[90], out.ctypes.data, 64, C.byref(n), C.byref(qu))
    assert rc == -3 and n.value == sizes[90] and qu.value == 90 and (out == 0xA5).all()


def test_rejected_arguments(rva):
    frame = make_frame("bgr8", *SMALL)
    for kw in ({"quality": 0}, {"quality": 101}, {"sampling": "4:1:1"}):
        with pytest.raises(rva.JpegError) as e:
            rva.preview_jpeg_host(frame, rva.AT_FMT_BGR8, 2, **kw)
        assert e.value.code == -1
    with pytest.raises(rva.JpegError):
        rva.preview_host(frame, 3, 2)                      # no such format
    with pytest.raises(rva.JpegError):
        rva.preview_host(frame, rva.AT_FMT_BGR8, 9)


def test_sanitized_standalone_program(tmp_path):
    """tests/preview_host_check.cpp + csrc/at_preview.cpp + csrc/at_mjpg.cpp built with the host
    compiler and -fsanitize=address,undefined (the runtimes linked statically), run as a child
    process: every format at the odd crops into exact-size heap buffers, records outside the
    crop, the search at budgets that fit first, midway and never."""
    exe = tmp_path / "preview_host_check"
    csrc = os.path.join(ROOT, "ros_vision_amd", "csrc")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-o", str(exe), os.path.join(ROOT, "tests", "preview_host_check.cpp"),
                    os.path.join(csrc, "at_preview.cpp"), os.path.join(csrc, "at_mjpg.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 2 sizes x 3 formats x 5 scales, less 72 x 56 at s = 8 (no preview of 8 x 8)
    assert r.stdout.split() == ["ok", str(2 * 27), str(4 * 27)]
