"""MJPG input, host side (no GPU): the JPEG front end in libat_hip.so
(csrc/at_mjpg.cpp -- marker parser, Huffman decode, the integer IDCT the kernel
shares) against Pillow's luma-only decode of the same bytes.  The target is
equality: libjpeg's integer "slow" IDCT is exactly specified.

Also: rejections, truncated / corrupted streams (in-process, and in a stand-alone
program built with the address and undefined-behaviour sanitizers), and the Python
node's "jpeg" encoding with a stand-in for the detector."""
import os
import subprocess
import time

import numpy as np
import pytest

import mjpg_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(328, 248), (24, 40)]   # 41 x 31 blocks: no multiple of 16 in either axis; 3 x 5 blocks
QUALITIES = [5, 30, 75, 95, 100]


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


@pytest.fixture(scope="module")
def boards():
    return {(w, h): mc.board(w, h, ntags=2 if w > 100 else 1, side_range=(40, 72) if w > 100 else (16, 20))
            for w, h in SIZES}


def _equal(rva, jpg):
    want = mc.pil_luma(jpg)
    got = rva.mjpg_decode_gray(jpg)
    assert got.shape == want.shape
    nd = int(np.count_nonzero(got != want))
    assert nd == 0, "%d pixels differ from Pillow's luma" % nd


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("sampling", list(mc.SAMPLINGS))
@pytest.mark.parametrize("size", SIZES)
def test_luma_equals_pillow(rva, boards, size, sampling, quality):
    _equal(rva, mc.encode(boards[size], quality, sampling))


def test_noise_q100_takes_the_dense_encoding(rva):
    """Every coefficient non-zero, long Huffman codes: sparse would be larger than
    2 B per pixel, so the frame travels dense -- and still decodes equal."""
    w, h = SIZES[0]
    jpg = mc.encode(mc.noise(w, h), 100, "444")
    _equal(rva, jpg)
    mode, nbytes = rva.mjpg_stream_mode(jpg, w, h)
    assert mode == "dense" and nbytes == 256 + 2 * w * h


def test_flat_q5_is_dc_only_and_sparse(rva):
    w, h = SIZES[0]
    jpg = mc.encode(np.full((h, w, 3), 93, np.uint8), 5, "422")
    _equal(rva, jpg)
    mode, nbytes = rva.mjpg_stream_mode(jpg, w, h)
    nb = (w // 8) * (h // 8)
    # the offset table and at most one (DC) token per block
    assert mode == "sparse" and nbytes <= 256 + 4 * (nb + 1) + 4 * nb


def test_board_is_sparse_and_smaller_than_yuyv(rva, boards):
    w, h = SIZES[0]
    mode, nbytes = rva.mjpg_stream_mode(mc.encode(boards[(w, h)], 80, "422"), w, h)
    assert mode == "sparse" and nbytes < 2 * w * h


@pytest.mark.parametrize("extra", [{"restart_marker_blocks": 1}, {"restart_marker_rows": 1}])
@pytest.mark.parametrize("sampling", ["422", "420", "gray"])
def test_restart_markers(rva, boards, sampling, extra):
    """More than 8 restart intervals either way: RSTn wraps from 7 to 0."""
    jpg = mc.encode(boards[SIZES[0]], 75, sampling, **extra)
    assert jpg.count(b"\xff\xd7") >= 1 and b"\xff\xdd" in jpg
    _equal(rva, jpg)


@pytest.mark.parametrize("sampling", ["422", "420", "gray"])
def test_stream_without_dht_uses_annex_k(rva, boards, sampling):
    """A non-optimised Pillow stream is coded with the Annex K tables and says so in
    its DHT segments; without them (UVC cameras) the built-in tables must be those."""
    jpg = mc.encode(boards[SIZES[0]], 75, sampling)
    bare = mc.strip_dht(jpg)
    assert b"\xff\xc4" not in bare[:bare.index(b"\xff\xda")]
    got = rva.mjpg_decode_gray(bare)
    assert np.array_equal(got, mc.pil_luma(jpg))


def test_annex_k_tables_are_what_pillow_writes():
    """The tables the library falls back to, read from its source as data, against
    the DHT segments of a non-optimised Pillow stream."""
    import re
    src = open(os.path.join(ROOT, "ros_vision_amd", "csrc", "at_mjpg.cpp")).read()

    def arr(name):
        body = re.search(r"%s\[\d+\] = \{(.*?)\};" % name, src, re.S).group(1)
        return bytes(int(v, 0) for v in body.replace("\n", " ").split(",") if v.strip())

    t = mc.dht_tables(mc.encode(mc.noise(32, 32), 80, "422"))
    assert t[(0, 0)] == (arr("kStdDcLumBits"), arr("kStdDcVals"))
    assert t[(0, 1)] == (arr("kStdDcChrBits"), arr("kStdDcVals"))
    assert t[(1, 0)] == (arr("kStdAcLumBits"), arr("kStdAcLumVals"))
    assert t[(1, 1)] == (arr("kStdAcChrBits"), arr("kStdAcChrVals"))


def test_avi1_app0_and_com_are_skipped(rva, boards):
    jpg = mc.encode(boards[SIZES[0]], 75, "422")
    uvc = mc.with_avi1_app0(mc.strip_dht(jpg))
    assert b"AVI1" in uvc
    assert np.array_equal(rva.mjpg_decode_gray(uvc), mc.pil_luma(jpg))


def test_optimised_tables_decode_too(rva, boards):
    _equal(rva, mc.encode(boards[SIZES[0]], 75, "420", optimize=True))


@pytest.mark.parametrize("name", ["colorimage.jpg", "grayimage.jpg"])
def test_reference_fixtures_equal_pillow(rva, golden_dir, name):
    """test/data/colorimage.jpg (1920x1080, 4:2:0: 1080 rows are no multiple of 16) and
    grayimage.jpg (1280x800, one component) of the reference."""
    jpg = open(os.path.join(golden_dir, name), "rb").read()
    _equal(rva, jpg)
    h, w = mc.pil_luma(jpg).shape
    assert rva.mjpg_stream_mode(jpg, w, h)[0] == "sparse"


def test_rejections(rva, boards):
    from ros_vision_amd.detector import AT_E_INVALID, AT_E_UNSUPPORTED, load_library
    w, h = SIZES[0]
    good = mc.encode(boards[(w, h)], 75, "422")
    assert rva.mjpg_stream_mode(good, w, h)[0] == "sparse"
    with pytest.raises(rva.MjpgError) as e:
        rva.mjpg_decode_gray(mc.encode(boards[(w, h)], 75, "422", progressive=True))
    assert e.value.code == AT_E_UNSUPPORTED == -6
    with pytest.raises(rva.MjpgError) as e:   # a size other than the detector's
        rva.mjpg_stream_mode(good, w + 8, h)
    assert e.value.code == AT_E_INVALID
    with pytest.raises(rva.MjpgError) as e:
        rva.mjpg_stream_mode(good, w, h - 8)
    assert e.value.code == AT_E_INVALID
    # 4:1:1 (luma 4x1) and 4:4:0 (luma 1x2) are sampled otherwise
    for hv in (0x41, 0x12):
        b = bytearray(good)
        sof = next(a for m, a, _ in mc.segments(good) if m == 0xC0)
        b[sof + 11] = hv
        with pytest.raises(rva.MjpgError) as e:
            rva.mjpg_decode_gray(bytes(b))
        assert e.value.code == AT_E_UNSUPPORTED
    b = bytearray(good)          # 12-bit precision
    b[sof + 4] = 12
    with pytest.raises(rva.MjpgError) as e:
        rva.mjpg_decode_gray(bytes(b))
    assert e.value.code == AT_E_UNSUPPORTED
    for junk in (b"", b"\xff", b"\xff\xd8", b"not a jpeg at all", good[2:]):
        with pytest.raises(rva.MjpgError) as e:
            rva.mjpg_decode_gray(junk)
        assert e.value.code == AT_E_INVALID
    assert b"unsupported JPEG" in load_library().at_strerror(AT_E_UNSUPPORTED)


def _damaged(boards):
    small = mc.encode(boards[SIZES[1]], 75, "420", restart_marker_blocks=2)
    return small, mc.truncations(small, 50) + mc.corruptions(small, 200)


def test_truncated_and_corrupted_streams_return(rva, boards):
    """50 truncations and 200 single-byte corruptions of a small stream: an error or a
    plane each, promptly."""
    small, cases = _damaged(boards)
    w, h = SIZES[1]
    t0 = time.perf_counter()
    planes = 0
    for jpg in cases:
        try:
            out = rva.mjpg_decode_gray(jpg)
        except rva.MjpgError as e:
            assert e.code in (-1, -6)
            continue
        assert out.dtype == np.uint8 and out.ndim == 2
        planes += 1
    assert time.perf_counter() - t0 < 5.0
    assert all(len(t) < len(small) for t in cases[:50])
    # a stream cut inside its headers is never a picture
    scan = small.index(b"\xff\xda")
    for jpg in cases[:50]:
        if len(jpg) <= scan:
            with pytest.raises(rva.MjpgError):
                rva.mjpg_stream_mode(jpg, w, h)
    assert planes > 0   # (many corruptions only change a coefficient)


def test_sanitized_standalone_program(boards, tmp_path):
    """tests/mjpg_host_check.cpp + csrc/at_mjpg.cpp built with the host compiler and
    -fsanitize=address,undefined, run as a child process over the same truncations and
    corruptions (and the good streams of every sampling) read from files."""
    exe = tmp_path / "mjpg_host_check"
    # (the sanitizer runtimes linked statically: the program then runs whatever else
    # the environment loads into every process)
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "mjpg_host_check.cpp"),
                    os.path.join(ROOT, "ros_vision_amd", "csrc", "at_mjpg.cpp")], check=True, timeout=300)
    small, cases = _damaged(boards)
    w, h = SIZES[1]
    cases = [small] + [mc.encode(boards[SIZES[1]], q, s) for s in mc.SAMPLINGS for q in (5, 100)] + \
            [mc.encode(mc.noise(w, h), 100, "444")] + cases
    files = []
    for i, jpg in enumerate(cases):
        p = tmp_path / ("case%03d.jpg" % i)
        p.write_bytes(jpg)
        files.append(str(p))
    r = subprocess.run([str(exe), str(w), str(h)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    decoded = int(r.stdout.split()[1])
    assert decoded >= 10   # the good streams at least


# ---- Python node: encoding "jpeg" ------------------------------------------------
class _StandInDetector:
    """Stands in for GpuDetector where the GPU would be needed: records what the node
    hands it and returns fixed detections / poses for either entry point."""

    def __init__(self, *a, **k):
        self.calls = []

    def _result(self):
        from ros_vision_amd.detector import Detection, Pose
        self._poses = [Pose(id=7, R=np.eye(3), t=np.array([0.3, -0.1, 2.0]), err=1e-6),
                       Pose(id=2, R=np.eye(3), t=np.array([0.0, 0.2, 1.0]), err=2e-6)]
        return [Detection(id=p.id, hamming=0, decision_margin=90.0, H=np.eye(3), c=np.zeros(2),
                          p=np.array([[5.0, 30.0], [30.0, 30.0], [30.0, 5.0], [5.0, 5.0]])) for p in self._poses]

    def detect(self, frame, fmt):
        self.calls.append(("detect", fmt, np.asarray(frame).shape))
        return self._result()

    def detect_mjpg(self, jpg):
        self.calls.append(("detect_mjpg", type(jpg), len(jpg)))
        return self._result()

    def poses(self, frame=0):
        return self._poses

    def close(self):
        pass


def test_node_jpeg_encoding_host_logic(monkeypatch, boards):
    """image_callback(encoding="jpeg") hands the compressed bytes to detect_mjpg and
    publishes the same pose records and tables as the GRAY8 ("mono8") path; no image."""
    from ros_vision_amd import node as N
    from ros_vision_amd.detector import AT_FMT_GRAY8
    monkeypatch.setattr(N, "GpuDetector", _StandInDetector)
    w, h = SIZES[0]
    jpg = mc.encode(boards[(w, h)], 85, "422")
    out = {}
    for enc, image in (("jpeg", jpg), ("mono8", mc.pil_luma(jpg))):
        got = {}
        node = N.ApriltagsDetectorNode(w, h, publishers={
            "camera/pose": lambda m, g=got: g.setdefault("pose", m),
            "camera/pose_camera": lambda m, g=got: g.setdefault("cam", m),
            "networktables": lambda m, g=got: g.setdefault("nt", m),
            "apriltags/images": lambda m, g=got: g.setdefault("img", m)})
        res = node.image_callback(image, stamp_s=12.25, encoding=enc)
        out[enc] = (res, got, node.detector.calls)
        node.close()
    rj, gj, cj = out["jpeg"]
    rm, gm, cm = out["mono8"]
    assert cj == [("detect_mjpg", bytes, len(jpg))]
    assert cm == [("detect", AT_FMT_GRAY8, (h, w))]
    assert rj.image is None and "img" not in gj
    assert rj.tag_detection_array == rm.tag_detection_array and [t[0] for t in rj.tag_detection_array] == [2, 7]
    assert rj.tag_detection_camera_array == rm.tag_detection_camera_array
    assert rj.networktables_pose_data == rm.networktables_pose_data and rj.proto_tags == rm.proto_tags
    assert gj["pose"] is rj.tag_detection_array and gj["nt"][0] == 12.25
