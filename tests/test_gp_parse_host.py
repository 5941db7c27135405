"""Game-piece output parse, host side (no GPU): at_gp_parse_host -- the CPU reference of the
parse kernels over the arithmetic they share (csrc/at_gp.h) -- against the numpy
restatement of the contract in gp_parse_cases.py.  The target is equality bit for bit:
every float field as uint32, the class, the count and the order.

Also: rejected arguments, a short `out`, and a stand-alone program built with the address
and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gp_parse_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def _host(rva, raw, conf_thr=0.25, iou_thr=0.45, model=(640, 640), orig=None):
    return rva.game_piece_parse_host(raw, conf_thr, iou_thr, model, orig, records=True)


@pytest.mark.parametrize("shape", gc.SHAPES, ids=lambda s: "P%d_C%d_G%d%s" % (s[0], s[1], s[2], "_l64" if s[3] else ""))
def test_generated_equals_numpy(rva, shape):
    P, C_, G, q = shape
    raw = gc.generate(P, C_, G, seed=P + C_, quantise=q)
    want = gc.checked(raw)
    gc.assert_same(_host(rva, raw), want, str(shape))
    if q:  # the quantised case is there for its ties
        assert len(np.unique(want["conf"])) < len(want)


@pytest.mark.parametrize("name", sorted(gc.HAND))
def test_hand_built_equals_numpy(rva, name):
    make, kw = gc.HAND[name]
    raw = make()
    gc.assert_same(_host(rva, raw, **kw), gc.reference(raw, **kw), name)


def test_chain_keeps_a_and_c(rva):
    got = _host(rva, gc.chain())
    assert [float(v) for v in got["x"]] == [100.0, 160.0] and [float(v) for v in got["conf"]] == [F(0.9), F(0.7)]


def test_threshold_is_strict(rva):
    raw = gc.threshold_edge()
    assert len(_host(rva, raw, iou_thr=0.5)) == 2                                   # iou == thr: kept
    assert len(_host(rva, raw, iou_thr=float(np.nextafter(F(0.5), F(0))))) == 1      # one ulp lower: suppressed


def test_cross_class_keeps_all(rva):
    got = _host(rva, gc.cross_class())
    assert sorted(int(c) for c in got["cls"]) == [0, 1, 2]
    assert [int(c) for c in got["cls"]] == [0, 1, 2]  # 0.9 first, then the tie by index


def test_ties_go_by_index(rva):
    got = _host(rva, gc.ties())
    # 0.75: prediction 1 (x 100), then 2 (x 400); 4 (x 101) is suppressed by 1; then 0.5, 0.3
    assert [float(v) for v in got["x"]] == [100.0, 400.0, 500.0, 300.0]


def test_no_candidates(rva):
    assert len(_host(rva, gc.none())) == 0


def test_conf_thr_zero_takes_every_prediction(rva):
    raw = gc.everything()
    st = {}
    want = gc.reference(raw, conf_thr=0.0, stats=st)
    assert st["candidates"] == 77
    got = _host(rva, raw, conf_thr=0.0)
    gc.assert_same(got, want)
    dead = got[got["conf"] == 0]
    assert len(dead) >= 1 and (dead["cls"] == 0).all()


def test_odd_scores(rva):
    raw = gc.odd_scores()
    got = _host(rva, raw, conf_thr=0.0, iou_thr=2.0)   # nothing suppressed: one box per prediction
    assert len(got) == 12
    by_x = {float(b["x"]): b for b in got}
    want = {0: (1, 0.6), 1: (2, 0.7), 2: (0, np.inf), 3: (0, 0.0), 4: (0, 0.0), 5: (0, 0.0), 6: (0, 0.5),
            7: (2, np.inf), 8: (0, 1e-45), 9: (0, 0.25), 11: (2, 3e38)}
    for i, (cls, conf) in want.items():
        b = by_x[100.0 + 7 * i]
        assert int(b["cls"]) == cls and b["conf"] == F(conf), i
    kept = _host(rva, raw)                               # 0.25: exactly the threshold stays, one ulp below goes
    xs = sorted(float(v) for v in _host(rva, raw, iou_thr=2.0)["x"])
    assert 100.0 + 7 * 9 in xs and 100.0 + 7 * 10 not in xs and 100.0 + 7 * 3 not in xs
    gc.assert_same(kept, gc.reference(raw))


@pytest.mark.parametrize("order", range(4))
@pytest.mark.parametrize("iou_thr", [0.45, 0.0, -1.0])
def test_odd_boxes(rva, order, iou_thr):
    raw = gc.odd_boxes_orders()[order]
    st = {}
    want = gc.reference(raw, iou_thr=iou_thr, stats=st)
    assert st["candidates"] == 20
    gc.assert_same(_host(rva, raw, iou_thr=iou_thr), want)


def test_cap_smaller_than_count(rva):
    L = rva.load_library()
    raw = gc.generate(1000, 3, 10, seed=3)
    want = gc.checked(raw)
    n = C.c_int()
    out = np.full((4, 6), 0x7fc0dead, np.uint32)   # 4 records of junk
    rec = out.view(gc.BOX).reshape(-1)
    assert len(rec) == 4 and len(want) > 3
    rc = L.at_gp_parse_host(raw.ctypes.data, 1000, 3, 0.25, 0.45, 640, 640, 640, 640, rec.ctypes.data, 3, C.byref(n))
    assert rc == 0 and n.value == len(want)
    gc.assert_same(rec[:3], want[:3])
    assert (out[3] == 0x7fc0dead).all()          # nothing past cap
    rc = L.at_gp_parse_host(raw.ctypes.data, 1000, 3, 0.25, 0.45, 640, 640, 640, 640, None, 0, C.byref(n))
    assert rc == 0 and n.value == len(want)      # cap 0 counts


def test_non_square_scaling(rva):
    raw = gc.generate(1000, 3, 10, seed=11)
    at_model = _host(rva, raw)
    got = _host(rva, raw, orig=(1280, 720))
    gc.assert_same(got, gc.checked(raw, orig=(1280, 720)))
    assert np.array_equal(got["x"], at_model["x"] * F(2)) and np.array_equal(got["h"], at_model["h"] * (F(720) / F(640)))
    assert np.array_equal(got["conf"], at_model["conf"])


def test_invalid_arguments(rva):
    L = rva.load_library()
    raw = gc.chain()
    out = np.zeros(8, gc.BOX)
    n = C.c_int(7)
    good = dict(raw=raw.ctypes.data, P=3, C=1, conf=0.25, iou=0.45, mw=640, mh=640, ow=640, oh=640,
                out=out.ctypes.data, cap=8, n=C.byref(n))

    def call(**kw):
        a = dict(good, **kw)
        return L.at_gp_parse_host(a["raw"], a["P"], a["C"], a["conf"], a["iou"], a["mw"], a["mh"], a["ow"], a["oh"],
                                  a["out"], a["cap"], a["n"])

    assert call() == 0 and n.value == 2
    bad = [dict(raw=None), dict(n=None), dict(out=None), dict(P=0), dict(P=-1), dict(C=0), dict(cap=-1),
           dict(conf=float("nan")), dict(conf=float("inf")), dict(iou=float("nan")), dict(iou=float("-inf")),
           dict(mw=0), dict(mh=0), dict(ow=0), dict(oh=-3)]
    for kw in bad:
        n.value = 7
        assert call(**kw) == -1, kw                 # AT_E_INVALID
        if kw.get("n", 1) is not None:
            assert n.value == 0, kw
    with pytest.raises(RuntimeError):
        rva.game_piece_parse_host(np.zeros((4, 10), F))          # no class row
    with pytest.raises(RuntimeError):
        rva.game_piece_parse_host(np.zeros(10, F))


def test_python_wrapper_shapes(rva):
    raw = np.stack([gc.generate(77, 1, 3, seed=s) for s in (1, 2)])
    per_frame = rva.game_piece_parse_host(raw)
    assert len(per_frame) == 2
    one = rva.game_piece_parse_host(raw[1])
    assert [(b.x, b.y, b.w, b.h, b.conf, b.cls) for b in one] == [(b.x, b.y, b.w, b.h, b.conf, b.cls)
                                                                  for b in per_frame[1]]
    assert isinstance(one[0], rva.GamePieceBox) and one[0].conf >= one[-1].conf


def test_host_draw_boxes_and_box_layout(rva):
    """node/at_node.cpp's draw_boxes (what the device drawing must match): 2-px rectangle
    sides in the class colour, clamped to the image; at_gp_box as the compiled C consumer
    lays it out."""
    import fcntl
    import json
    node = os.path.join(ROOT, "node")
    with open(os.path.join(node, ".build.lock"), "w") as lk:   # one make at a time, as tests/test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", node, "-s"], check=True, timeout=600)
    rva.load_library()
    L = C.CDLL(os.path.join(node, "libat_node.so"))
    L.at_node_draw_boxes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.at_node_draw_boxes.restype = None
    img = np.zeros((48, 64, 3), np.uint8)
    boxes = np.array([(20, 20, 20, 10, 0.9, 1), (60, 40, 30, 30, 0.8, 8), (-50, -50, 10, 10, 0.5, 0)], gc.BOX)
    L.at_node_draw_boxes(img.ctypes.data, 64, 48, boxes.ctypes.data, 3)
    assert tuple(img[15, 20]) == tuple(img[25, 20]) == tuple(img[20, 10]) == tuple(img[20, 30]) == (0, 165, 255)
    assert tuple(img[20, 20]) == (0, 0, 0)                     # the inside stays
    assert tuple(img[14, 20]) == tuple(img[16, 20]) == (0, 165, 255)                 # within 1 px of the side
    assert tuple(img[13, 20]) == tuple(img[17, 20]) == (0, 0, 0)
    assert tuple(img[25, 47]) == (255, 0, 0) and tuple(img[40, 63]) == (255, 0, 0)   # cls 8 -> blue, clamped to x = 63
    assert tuple(img[0, 0]) == (0, 255, 0)                     # wholly outside: clamped to the corner, as the reference
    lay = json.loads(subprocess.run([os.path.join(node, "abi_check"), "layout"], check=True, capture_output=True,
                                    text=True, timeout=60).stdout)
    assert lay["sizeof.at_gp_box"] == rva.GP_BOX_DTYPE.itemsize == gc.BOX.itemsize == 24
    assert (lay["at_gp_box.x"], lay["at_gp_box.conf"], lay["at_gp_box.cls"]) == (0, 16, 20)
    assert rva.GP_BOX_DTYPE.fields["cls"][1] == 20 and rva.AT_GP_MAX_CANDIDATES == gc.MAX_CANDIDATES


def test_sanitized_standalone_program(tmp_path):
    """tests/gp_parse_host_check.cpp + csrc/at_gp.cpp built with the host compiler and
    -fsanitize=address,undefined (the runtimes linked statically), run as a child process:
    exact-size heap buffers for `out`, cap 0, P = 1, every prediction a candidate."""
    exe = tmp_path / "gp_parse_host_check"
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", str(exe), os.path.join(ROOT, "tests", "gp_parse_host_check.cpp"),
                    os.path.join(ROOT, "ros_vision_amd", "csrc", "at_gp.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[0] == "ok" and int(r.stdout.split()[1]) >= 6
