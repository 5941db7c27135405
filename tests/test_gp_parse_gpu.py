"""Game-piece output parse on the GPU: k_gp_cand + k_gp_nms (at_gp_parse_device) against the
CPU reference at_gp_parse_host, bit for bit -- every float field as uint32, the class, the
count and the order; the boxes drawn on the GPU against the node's host drawing, pixel for
pixel; and the Python node over a stand-in engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gp_parse_cases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(ROOT, "node")
F = np.float32
W, H = 640, 480          # the detector's geometry: what the boxes are scaled to
MAX_BATCH = 8


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    return rva


@pytest.fixture(scope="module")
def det(gpu):
    d = gpu.GpuDetector(W, H, max_batch=MAX_BATCH, tag_size=0.0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def nodelib():
    import fcntl
    from ros_vision_amd import detector
    with open(os.path.join(NODE, ".build.lock"), "w") as lk:   # one make at a time, as tests/test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", NODE, "-s"], check=True)
    detector.load_library()
    L = C.CDLL(os.path.join(NODE, "libat_node.so"))
    L.at_node_draw_boxes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.at_node_draw_boxes.restype = None
    return L


def _host(gpu, raw, conf_thr=0.25, iou_thr=0.45, orig=(W, H)):
    return gpu.game_piece_parse_host(raw, conf_thr, iou_thr, (640, 640), orig, records=True)


def _dev(frames, pad=0):
    """frames ([4 + C, P] each, same shape) in device memory, `pad` floats between them:
    (tensor that owns the memory, (ptr, nframes, C, P, frame_stride))."""
    import torch
    c4, p = frames[0].shape
    stride = c4 * p + pad
    buf = np.full((len(frames), stride), np.nan, F)    # the padding must never be read as a score
    for f, fr in enumerate(frames):
        buf[f, :c4 * p] = np.ascontiguousarray(fr, F).ravel()
    t = torch.from_numpy(buf).cuda()
    return t, (t.data_ptr(), len(frames), c4 - 4, p, stride)


def _parse(det, frames, conf_thr=0.25, iou_thr=0.45, pad=0, **kw):
    t, arg = _dev(frames, pad)
    return det.game_piece_parse(arg, conf_thr, iou_thr, (640, 640), records=True, **kw)


@pytest.mark.parametrize("name", sorted(gc.HAND))
def test_hand_built_equals_host(gpu, det, name):
    make, kw = gc.HAND[name]
    kw = {k: v for k, v in kw.items() if k != "orig"}     # the device call scales to the detector's geometry
    raw = make()
    want = _host(gpu, raw, **kw)
    gc.assert_same(_parse(det, [raw], **kw)[0], want, name)
    if name == "chain":
        assert [float(v) for v in want["conf"]] == [F(0.9), F(0.7)]
    if name in ("edge_at", "edge_below"):
        assert len(want) == (2 if name == "edge_at" else 1)
    if name == "everything":
        assert det.game_piece_parse_stats()["candidates"] == 77


@pytest.mark.parametrize("iou_thr", [0.45, 0.0, -1.0])
def test_odd_boxes_equal_host(gpu, det, iou_thr):
    frames = gc.odd_boxes_orders()
    got = _parse(det, frames, iou_thr=iou_thr)
    for f, raw in enumerate(frames):
        gc.assert_same(got[f], _host(gpu, raw, iou_thr=iou_thr), "order %d" % f)


def test_non_square_scaling(gpu):
    d = gpu.GpuDetector(1280, 720, tag_size=0.0)
    try:
        raw = gc.generate(1000, 3, 10, seed=11)
        want = _host(gpu, raw, orig=(1280, 720))
        gc.assert_same(_parse(d, [raw])[0], want)
        gc.assert_same(want, gc.checked(raw, orig=(1280, 720)))
    finally:
        d.close()


@pytest.mark.parametrize("nframes", [1, 3, 8])
@pytest.mark.parametrize("shape", gc.SHAPES, ids=lambda s: "P%d_C%d_G%d%s" % (s[0], s[1], s[2], "_l64" if s[3] else ""))
def test_generated_batches_equal_host(gpu, det, shape, nframes):
    """nframes different frames in one call, one of them empty, frame_stride > (4 + C) * P.
    P = 77 and 1000 are no multiples of 64 or 256: tail lanes."""
    P, C_, G, q = shape
    frames = [gc.generate(P, C_, G, seed=100 * f + P + C_, quantise=q) for f in range(nframes)]
    gc.checked(frames[0], orig=(W, H))
    if nframes > 1:
        frames[1][4:] = 0.1
    got = _parse(det, frames, pad=13)
    assert len(got) == nframes
    kept = cand = 0
    for f, raw in enumerate(frames):
        want = _host(gpu, raw)
        gc.assert_same(got[f], want, "frame %d" % f)
        kept += len(want)
        cand += int((~(np.where(raw[4:] > 0, raw[4:], 0).max(axis=0) < F(0.25))).sum())
    if nframes > 1:
        assert len(got[1]) == 0
    st = det.game_piece_parse_stats()
    assert st["boxes"] == kept and st["candidates"] == cand and st["kernels_ns"] == 0


def test_candidate_counts_around_the_sort_paths(gpu, det):
    """Up to 1024 candidates a frame is sorted by counting, beyond by the bitonic network
    (padded to a power of two); 64 candidates are one live word.  One call holds frames on
    both sides of each edge."""
    counts = [63, 64, 65, 1023, 1024, 1025, 2048, 2049]
    frames = [gc.with_candidates(n, seed=n) for n in counts]
    got = _parse(det, frames, pad=3)
    for f, n in enumerate(counts):
        st = {}
        want = gc.reference(frames[f], orig=(W, H), stats=st)
        assert st["candidates"] == n and 2 <= st["kept"] < n
        gc.assert_same(_host(gpu, frames[f]), want, "host, %d candidates" % n)
        gc.assert_same(got[f], want, "%d candidates" % n)
    assert det.game_piece_parse_stats()["candidates"] == sum(counts)


def test_torch_tensor_input(gpu, det):
    import torch
    frames = np.stack([gc.generate(1000, 3, 10, seed=s) for s in (1, 2, 3)])
    t = torch.from_numpy(frames).cuda()
    got = det.game_piece_parse(t, records=True)
    for f in range(3):
        gc.assert_same(got[f], _host(gpu, frames[f]))
    one = det.game_piece_parse(t[2])                         # [4 + C, P]: one frame, GamePieceBox objects
    assert len(one) == 1 and [b.cls for b in one[0]] == [int(c) for c in got[2]["cls"]]
    assert [F(b.x).view(np.uint32) for b in one[0]] == [v.view(np.uint32) for v in got[2]["x"]]


def test_exactly_4096_candidates(gpu, det):
    """The full sort and the longest sweep: 4096 equal confidences on disjoint boxes, all kept,
    in prediction order."""
    raw = gc.grid(4096)
    got = _parse(det, [raw])[0]
    assert len(got) == 4096 and det.game_piece_parse_stats()["max_candidates_per_frame"] == 4096
    gc.assert_same(got, _host(gpu, raw))


def test_4097_candidates_is_capacity(gpu, det):
    L = gpu.load_library()
    frames = [gc.generate(5000, 2, 30, seed=9), gc.grid(4097), gc.grid(4096)]
    t, (ptr, nf, nc, p, stride) = _dev(frames, pad=5)
    out = np.zeros((3, 4096), gc.BOX)
    n, status = (C.c_int * 3)(), (C.c_int * 3)(7, 7, 7)
    rc = L.at_gp_parse_device(det._h, C.c_void_p(ptr), stride, nf, p, nc, 0.25, 0.45, 640, 640, None,
                              out.ctypes.data, 4096, n, status)
    assert rc == 0 and list(status) == [0, -3, 0] and n[1] == 0          # AT_E_CAPACITY, zero boxes
    assert not out[1].view(np.uint32).any()                              # nothing written for it
    for f in (0, 2):                                                     # its neighbours are exact
        gc.assert_same(out[f, :n[f]], _host(gpu, frames[f]), "frame %d" % f)
    assert det.game_piece_parse_stats()["max_candidates_per_frame"] == 4097
    with pytest.raises(gpu.GamePieceCapacityError) as e:
        det.game_piece_parse((ptr, nf, nc, p, stride), records=True)
    assert e.value.frame == 1 and "frame 1" in str(e.value)
    loose = det.game_piece_parse((ptr, nf, nc, p, stride), records=True, strict=False)
    for f in range(3):
        gc.assert_same(loose[f], _host(gpu, frames[f]), "strict=False frame %d" % f)
    assert len(loose[1]) == 4097
    # ... and from a tensor
    import torch
    loose = det.game_piece_parse(torch.from_numpy(np.stack(frames)).cuda(), records=True, strict=False)
    assert len(loose[1]) == 4097 and gc.same(loose[1], _host(gpu, frames[1]))


def test_calls_in_a_row_leave_nothing_behind(gpu, det):
    a = [gc.generate(8400, 80, 40, seed=f) for f in range(2)]
    b = [gc.generate(77, 1, 3, seed=f) for f in range(5)]
    over = [gc.grid(4500)]
    want_a, want_b = [_host(gpu, r) for r in a], [_host(gpu, r) for r in b]
    for frames, want in ((a, want_a), (over, None), (b, want_b), (a, want_a), (b, want_b)):
        if want is None:
            with pytest.raises(gpu.GamePieceCapacityError):
                _parse(det, frames)
            continue
        got = _parse(det, frames)
        for f in range(len(frames)):
            gc.assert_same(got[f], want[f])


def test_cap_smaller_than_count(gpu, det):
    raw = gc.generate(1000, 3, 10, seed=3)
    want = _host(gpu, raw)
    L = gpu.load_library()
    t, (ptr, nf, nc, p, stride) = _dev([raw, raw])
    out = np.full((2, 3, 6), 0x7fc0dead, np.uint32)
    n = (C.c_int * 2)()
    rc = L.at_gp_parse_device(det._h, C.c_void_p(ptr), stride, 2, p, nc, 0.25, 0.45, 640, 640, None,
                              out.ctypes.data, 2, n, None)                # cap_per_frame 2, no status array
    assert rc == 0 and list(n) == [len(want)] * 2 and len(want) > 3
    rec = out.view(gc.BOX).reshape(2, 3)
    gc.assert_same(rec[0, :2], want[:2])
    gc.assert_same(rec[0, 2:3], want[:1])   # frame 1 starts at out + cap_per_frame
    gc.assert_same(rec[1, :1], want[1:2])
    assert (out[1, 1:] == 0x7fc0dead).all()
    assert [len(x) for x in det.game_piece_parse((ptr, nf, nc, p, stride), records=True, cap=3)] == [3, 3]


def test_invalid_arguments(gpu, det):
    L = gpu.load_library()
    raw = gc.chain()
    t, (ptr, nf, nc, p, stride) = _dev([raw])
    out = np.zeros(8, gc.BOX)
    n = (C.c_int * 16)()
    good = dict(d=det._h, raw=C.c_void_p(ptr), stride=stride, nf=1, P=p, C=nc, conf=0.25, iou=0.45, mw=640, mh=640,
                out=out.ctypes.data, cap=8, n=n)

    def call(**kw):
        a = dict(good, **kw)
        return L.at_gp_parse_device(a["d"], a["raw"], a["stride"], a["nf"], a["P"], a["C"], a["conf"], a["iou"],
                                    a["mw"], a["mh"], None, a["out"], a["cap"], a["n"], None)

    assert call() == 0 and n[0] == 2
    bad = [dict(d=None), dict(raw=None), dict(out=None), dict(n=None), dict(P=0), dict(C=0), dict(nf=0),
           dict(nf=MAX_BATCH + 1), dict(nf=-1), dict(stride=stride - 1), dict(conf=float("nan")),
           dict(iou=float("inf")), dict(mw=0), dict(mh=-1), dict(cap=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call() == 0 and n[0] == 2        # and the detector is none the worse for them


def test_producer_stream_orders_the_parse(gpu, det):
    """The tensor is written on another stream, behind a queue of long fills; the parse
    waits for that stream on the GPU (no host wait in between) and sees it."""
    import torch
    raw = gc.generate(8400, 2, 20, seed=21)
    want = gc.checked(raw, orig=(W, H))
    src = torch.from_numpy(raw).pin_memory()
    t = torch.zeros(raw.shape, dtype=torch.float32, device="cuda")
    big = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            big.add_(1.0)
        t.copy_(src, non_blocking=True)
    got = det.game_piece_parse(t, records=True, producer_stream=s)[0]
    gc.assert_same(got, want)
    got = det.game_piece_parse(t, records=True, producer_stream=s.cuda_stream)[0]   # the raw handle
    gc.assert_same(got, want)


def test_kernel_time_while_profiling(gpu, det):
    raw = gc.generate(8400, 1, 20, seed=4)
    det.set_profiling(True)
    try:
        got = _parse(det, [raw])[0]
        ns = det.game_piece_parse_stats()["kernels_ns"]
    finally:
        det.set_profiling(False)
    gc.assert_same(got, _host(gpu, raw))
    assert 0 < ns < 50_000_000
    _parse(det, [raw])
    assert det.game_piece_parse_stats()["kernels_ns"] == 0


# ---- boxes on the image -------------------------------------------------------------------
def _boxes():
    nan, inf = np.nan, np.inf
    b = [(100, 100, 80, 60, 0.9, 0), (300, 200, 120, 90, 0.8, 1), (320, 240, 100, 100, 0.8, 2),   # overlapping
         (5, 5, 40, 40, 0.7, 3), (635, 475, 60, 60, 0.7, 4), (320, -10, 700, 60, 0.6, 5),          # partly outside
         (-200, -200, 50, 50, 0.5, 6), (2000, 240, 50, 50, 0.5, 7), (320, 3000, 50, 50, 0.5, 11),  # wholly outside
         (200.7, 300.9, 33.3, 44.4, 0.4, 13), (400, 400, 0, 0, 0.4, 0), (450, 100, -30, 40, 0.3, 1),
         (nan, 100, 50, 50, 0.3, 2), (100, 100, inf, 50, 0.3, 3), (3e9, -3e9, 10, 10, 0.3, 4), (500, 300, 60, 80, 0.2, -1)]
    return np.array(b, gc.BOX)


def _host_drawn(nodelib, img, boxes):
    out = np.array(img, copy=True)
    boxes = np.ascontiguousarray(boxes)
    nodelib.at_node_draw_boxes(out.ctypes.data, out.shape[1], out.shape[0], boxes.ctypes.data if len(boxes) else None,
                               len(boxes))
    return out


def test_boxes_drawn_equal_host_drawing(gpu, det, nodelib):
    import torch
    img = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    boxes = _boxes()
    want = _host_drawn(nodelib, img, boxes)
    assert (want != img).any(axis=2).sum() > 2000
    assert tuple(want[100 - 30, 100]) == (0, 255, 0) and tuple(want[200 - 45, 300]) == (0, 165, 255)
    dev = torch.from_numpy(img).cuda()
    det.game_piece_draw_boxes_device(dev.data_ptr(), boxes)
    assert np.array_equal(dev.cpu().numpy(), want)
    dev = torch.from_numpy(img).cuda()                       # GamePieceBox objects, and no boxes at all
    det.game_piece_draw_boxes_device(dev.data_ptr(), gpu.game_piece_boxes(boxes[:6]))
    assert np.array_equal(dev.cpu().numpy(), _host_drawn(nodelib, img, boxes[:6]))
    det.game_piece_draw_boxes_device(dev.data_ptr(), [])
    assert np.array_equal(dev.cpu().numpy(), _host_drawn(nodelib, img, boxes[:6]))


# ---- the Python node over a stand-in engine -----------------------------------------------
class _Engine:
    """Stands in for the user's network: checks what it is handed and returns a generated
    output tensor [1, 4 + C, P] in device memory."""

    def __init__(self, raw):
        import torch
        self.out = torch.from_numpy(raw[None]).cuda()
        self.seen = None

    def __call__(self, x):
        assert x.is_cuda and tuple(x.shape) == (1, 3, 640, 640) and str(x.dtype) == "torch.float32"
        self.seen = x.clone()
        return self.out.clone()


@pytest.mark.parametrize("image_jpeg", [None, 90])
def test_python_node(gpu, nodelib, image_jpeg):
    from ros_vision_amd.node import GamePieceDetectorNode
    names = ["coral", "algae", "robot"]
    raw = gc.generate(8400, 3, 12, seed=31)
    frame = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
    eng = _Engine(raw)
    sent = {}
    topic = "game_piece_detector/images" + ("/compressed" if image_jpeg else "")
    node = GamePieceDetectorNode(W, H, eng, class_names=names, image_jpeg=image_jpeg,
                                 publishers={topic: lambda m: sent.setdefault("image", m),
                                             "game_piece_detector/detections": lambda m: sent.setdefault("boxes", m)})
    try:
        res = node.image_callback(frame, 1.0)
        want = gc.checked(raw, orig=(W, H))
        gc.assert_same(_host(gpu, raw), want)
        got = np.array([(b.x, b.y, b.w, b.h, b.conf, b.cls) for b in res.boxes], gc.BOX)
        gc.assert_same(got, want)
        assert [b.class_name for b in res.boxes] == [names[c] for c in want["cls"]] and sent["boxes"] is res.boxes
        # the engine saw preprocess_image's tensor of this frame: RGB, / 255, resized
        assert 0.0 <= float(eng.seen.min()) and float(eng.seen.max()) <= 1.0 and float(eng.seen.std()) > 0.01
        drawn = _host_drawn(nodelib, frame, want)
        assert (drawn != frame).any()
        if image_jpeg:
            assert res.image is None and res.image_jpeg == gpu.jpeg_encode_host(drawn, image_jpeg, "4:2:0")
            assert sent["image"] == res.image_jpeg
        else:
            assert res.image_jpeg is None and np.array_equal(res.image, drawn) and sent["image"] is res.image
        quiet = GamePieceDetectorNode(W, H, eng, class_names=names)      # no image topic bound: no image work
        try:
            r2 = quiet.image_callback(frame, 2.0)
            assert r2.image is None and r2.image_jpeg is None and len(r2.boxes) == len(want)
        finally:
            quiet.close()
    finally:
        node.close()
