"""at_node::GamePieceCore (node/at_node.h) through node/gp_core_check, a small C++ driver
with a stand-in engine: frame -> HBM and the at_gp tensor -> infer -> at_gp_parse_device ->
boxes with class names, the frame with the boxes drawn on its staged copy, and its JPEG.
Boxes against at_gp_parse_host, the image against the host draw_boxes, the JPEG against
jpeg_encode_host of that image, the engine's input against the detector's own tensor."""
import ctypes as C
import fcntl
import json
import os
import subprocess

import numpy as np
import pytest

import gp_parse_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(ROOT, "node")
W, H = 640, 480


@pytest.fixture(scope="module")
def built():
    with open(os.path.join(NODE, ".build.lock"), "w") as lk:   # one make at a time, as tests/test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", NODE, "-s"], check=True)
    return NODE


def test_driver_builds_and_refuses_bad_arguments(built):
    r = subprocess.run([os.path.join(built, "gp_core_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
def test_game_piece_core_through_the_cpp_driver(built, tmp_path):
    import ros_vision_amd as rva
    P, nc, quality = 8400, 3, 90
    raw = gc.generate(P, nc, 12, seed=41)
    want = gc.checked(raw, orig=(W, H))
    gc.assert_same(rva.game_piece_parse_host(raw, 0.25, 0.45, (640, 640), (W, H), records=True), want)
    frame = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    frame.tofile(tmp_path / "frame.bgr")
    raw.tofile(tmp_path / "tensor.f32")
    r = subprocess.run([os.path.join(built, "gp_core_check"), str(W), str(H), str(tmp_path / "frame.bgr"),
                        str(tmp_path / "tensor.f32"), str(P), str(nc), str(quality), str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["boxes"] == len(want) and info["status"] == 0 and info["infer_calls"] == 2
    got = np.fromfile(tmp_path / "boxes.bin", gc.BOX)
    gc.assert_same(got, want)
    names = (tmp_path / "names.txt").read_text().split()
    assert names == [["coral", "algae", "unknown"][c] for c in want["cls"]] and "unknown" in names
    # the image: the host drawing of those boxes on the frame
    L = C.CDLL(os.path.join(built, "libat_node.so"))
    L.at_node_draw_boxes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.at_node_draw_boxes.restype = None
    drawn = frame.copy()
    L.at_node_draw_boxes(drawn.ctypes.data, W, H, np.ascontiguousarray(want).ctypes.data, len(want))
    assert (drawn != frame).any()
    assert np.array_equal(np.fromfile(tmp_path / "image.bgr", np.uint8).reshape(H, W, 3), drawn)
    jpg = (tmp_path / "image.jpg").read_bytes()
    assert len(jpg) == info["jpeg_bytes"] and jpg == rva.jpeg_encode_host(drawn, quality, "4:2:0")
    # the engine was handed preprocess_image's tensor of this frame
    det = rva.GpuDetector(W, H, tag_size=0.0)
    try:
        det.enable_game_piece_input(640, 640, 3)
        det.detect(frame, rva.AT_FMT_BGR8)
        tensor = det.game_piece_tensor(0)
    finally:
        det.close()
    seen = np.fromfile(tmp_path / "input.f32", np.float32).reshape(3, 640, 640)
    assert np.array_equal(seen.view(np.uint32), tensor.view(np.uint32))
