"""Ideal corners on the CPU (no GPU): at_undistort_points_host and at_ideal_detections_host against
the numpy restatement in tests/undistort_cases.py, bit for bit, on the deployed lenses
(tests/golden/lenses.json); what is flagged and what is not; the pose bias the mode removes; the
ABI.  The twins share their arithmetic with the kernels (csrc/at_undist.h), so what holds here is
what the device path is then held to in tests/test_undistort_gpu.py."""
import ctypes as C
import fcntl
import json
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import undistort_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENSES = uc.load_lenses()
TS = 0.1651


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def host_points(rva, ln, xy):
    cam, dist = uc.camera_of(rva, ln)
    return rva.undistort_points_host(xy, cam, dist)


def host_ideal(rva, ln, dets):
    cam, dist = uc.camera_of(rva, ln)
    return rva.ideal_detections_host(dets, cam, dist)


# ---- points -------------------------------------------------------------------------------------
def test_lens_fixture_holds_the_eight_lenses():
    assert sorted(LENSES) == sorted(uc.REGULAR + ("cam14",))
    assert all((ln.width, ln.height) == (1280, 800) for ln in LENSES.values())


@pytest.mark.parametrize("name", sorted(LENSES))
def test_points_equal_the_restatement_bit_for_bit(rva, name):
    ln = LENSES[name]
    xy = uc.grid(ln, 4)
    out, ok = host_points(rva, ln, xy)
    want, wok = uc.und_points_ref(ln, xy)
    assert np.array_equal(ok, wok)
    assert out.tobytes() == want.tobytes()
    assert np.array_equal(out[~ok], xy[~ok])                 # a flagged pixel comes back raw


@pytest.mark.parametrize("name", uc.REGULAR)
def test_regular_lenses_invert_every_pixel(rva, name):
    ln = LENSES[name]
    xy = uc.grid(ln, 4)
    out, ok = host_points(rva, ln, xy)
    assert ok.all()
    err = float(np.abs(uc.forward_pixels(ln, out) - xy).max())
    print("%s: forward(ideal) - raw, worst %.3g px; greatest shift %.1f px; least determinant %.3f"
          % (name, err, np.abs(out - xy).max(), uc.min_determinant(ln, out)))
    assert err <= 1e-9                                       # measured: 4.6e-13 on every lens
    assert uc.min_determinant(ln, out) >= 0.5


def test_cam14_folds_over_at_the_corners(rva):
    ln = LENSES["cam14"]
    _out, ok = host_points(rva, ln, [(0, 0), (40, 40), (1279, 0), (0, 799), (100, 60), (640, 400), (1279, 799)])
    assert ok.tolist() == [False, False, False, False, True, True, True]
    _out, ok = host_points(rva, ln, uc.grid(ln, 4))
    frac = 1.0 - ok.mean()
    print("cam14: %.2f %% of the 4-px grid flagged" % (100 * frac))
    assert 0.004 < frac < 0.012                              # about 0.7 % of the frame


def test_nan_and_infinity_are_flagged(rva):
    for ln in (LENSES["cam11"], LENSES["cam14"]):
        xy = np.array([[np.nan, 5.0], [5.0, np.nan], [np.inf, 5.0], [5.0, -np.inf], [np.nan, np.nan], [1e308, 1e308]])
        out, ok = host_points(rva, ln, xy)
        assert not ok.any()
        assert out.tobytes() == xy.tobytes()


def test_zero_coefficients_copy_bit_for_bit(rva):
    ln = uc.lens(905.495617, 907.909470, 609.916016, 352.682645, width=1280, height=800)
    rng = np.random.default_rng(3)
    xy = np.concatenate([uc.grid(ln, 16), rng.uniform(-50, 1400, (500, 2))])
    out, ok = host_points(rva, ln, xy)
    assert ok.all() and out.tobytes() == xy.tobytes()
    dets = _detections(ln, rng, 20)
    for d in dets:
        d.H = d.H + rng.normal(scale=1e-3, size=(3, 3))      # an H the corners do not give: it is copied, not recomputed
    got = host_ideal(rva, ln, dets)
    assert all(uc.same_detection(a, b) for a, b in zip(got, dets))


# ---- detections ---------------------------------------------------------------------------------
def _detection(H, tid=0, hamming=0, margin=50.0):
    H = np.asarray(H, np.float64).reshape(3, 3)
    p = np.array([(H @ [x, y, 1.0])[:2] / (H @ [x, y, 1.0])[2] for x, y in uc.CORNER_T])
    c = (H @ [0.0, 0.0, 1.0])[:2] / H[2, 2]
    return SimpleNamespace(id=tid, hamming=hamming, decision_margin=margin, H=H, c=c, p=p)


def _detections(ln, rng, n, lo=0.08, hi=0.92):
    """n detections of 20-90 px somewhere in the frame, turned and sheared a little."""
    out = []
    for k in range(n):
        cx, cy = rng.uniform(lo * ln.width, hi * ln.width), rng.uniform(lo * ln.height, hi * ln.height)
        h, a = rng.uniform(10, 45), rng.uniform(0, 2 * math.pi)
        M = h * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]) @ (np.eye(2) + rng.normal(scale=0.1, size=(2, 2)))
        H = np.array([[M[0, 0], M[0, 1], cx], [M[1, 0], M[1, 1], cy], [rng.normal(scale=1e-2), rng.normal(scale=1e-2), 1.0]])
        out.append(_detection(H, tid=k, hamming=k % 3, margin=float(np.float32(30.0 + k))))
    return out


@pytest.mark.parametrize("name", sorted(LENSES))
def test_ideal_detections_equal_the_restatement_bit_for_bit(rva, name):
    ln = LENSES[name]
    dets = _detections(ln, np.random.default_rng(11), 60, lo=0.0, hi=1.0)
    got = host_ideal(rva, ln, dets)
    want = [uc.ideal_detection_ref(ln, d) for d in dets]
    assert [g.id for g in got] == [w.id for w in want]
    assert all(uc.same_detection(a, b) for a, b in zip(got, want))
    flagged = sum(g.id < 0 for g in got)
    assert (flagged > 0) == (name == "cam14")
    worst = 0.0
    for g, d in zip(got, dets):
        if g.id < 0:
            assert uc.same_detection(g, SimpleNamespace(**{**vars(d), "id": -1}))        # raw values
            continue
        for (x, y), p in zip(uc.CORNER_T, g.p):
            q = g.H @ [x, y, 1.0]
            worst = max(worst, float(np.abs(q[:2] / q[2] - p).max()))
        worst = max(worst, float(np.abs(g.H[:2, 2] / g.H[2, 2] - g.c).max()))
        assert np.abs(uc.forward_pixels(ln, g.p) - d.p).max() <= 1e-6
    print("%s: H (+-1, +-1) - p, worst %.3g px; %d of %d not invertible" % (name, worst, flagged, len(got)))
    assert worst <= 1e-9


def test_one_flagged_corner_flags_the_detection(rva):
    ln = LENSES["cam14"]
    d = _detection([[35.0, 0.0, 70.0], [0.0, -35.0, 70.0], [0.0, 0.0, 1.0]], tid=7)   # corners (35, 35) .. (105, 105)
    _q, ok = host_points(rva, ln, d.p)
    assert 0 < ok.sum() < 4                                                       # some corners invert, some do not
    (g,) = host_ideal(rva, ln, [d])
    assert g.id == -1 and uc.same_detection(g, SimpleNamespace(**{**vars(d), "id": -1}))
    inner = _detection([[35.0, 0.0, 170.0], [0.0, -35.0, 170.0], [0.0, 0.0, 1.0]], tid=7)
    (g,) = host_ideal(rva, ln, [inner])
    assert g.id == 7 and np.abs(g.p - inner.p).max() > 1.0            # 100 px further in: ideal, and moved


# ---- the bias the mode removes ------------------------------------------------------------------
def _angle(A, B):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(A.T @ B) - 1.0) / 2.0))))


@pytest.mark.parametrize("centre,edge", [((619, 436), False), ((972, 611), False), ((1178, 747), True)])
def test_pose_bias_is_removed(rva, oracle_mod, centre, edge):
    """A 0.1651 m tag 2.5 m in front of cam11 (1280 x 800), facing the camera, its centre seen at the
    raw pixel `centre`; exact corners through the forward model.  estimate_tag_pose (the host path
    of tests/test_pose.py) on the raw corners and the H they give is off by 1.1 mm / 0.7 deg,
    4.8 mm / 1.3 deg and 30 mm / 6.4 deg at the three centres (measured here); on the ideal record
    it returns the pose."""
    ln = LENSES["cam11"]
    ci, ok = uc.und_points_ref(ln, [centre])
    assert ok.all()
    Z = 2.5
    t = np.array([(ci[0, 0] - ln.cx) / ln.fx * Z, (ci[0, 1] - ln.cy) / ln.fy * Z, Z])
    K = np.array([[ln.fx, 0, ln.cx], [0, ln.fy, ln.cy], [0, 0, 1]])
    H = K @ np.column_stack([[TS / 2, 0, 0], [0, TS / 2, 0], t])
    ideal = _detection(H / H[2, 2])
    raw_p = uc.forward_pixels(ln, ideal.p)
    raw = SimpleNamespace(id=3, hamming=0, decision_margin=50.0, H=uc.homography_ref(raw_p).reshape(3, 3),
                          c=raw_p.mean(0), p=raw_p)
    Rr, tr, _e, _es, _s = oracle_mod.estimate_tag_pose(raw.H, raw.p, ln.fx, ln.fy, ln.cx, ln.cy, TS)
    (g,) = host_ideal(rva, ln, [raw])
    assert g.id == 3
    Ri, ti, _e, _es, _s = oracle_mod.estimate_tag_pose(g.H, g.p, ln.fx, ln.fy, ln.cx, ln.cy, TS)
    print("centre %s: raw corners %.1f mm, %.2f deg off; ideal corners %.2e m, %.2e deg"
          % (centre, 1e3 * np.linalg.norm(tr - t), _angle(Rr, np.eye(3)), np.linalg.norm(ti - t), _angle(Ri, np.eye(3))))
    if edge:
        assert np.linalg.norm(tr - t) > 0.020
    assert np.linalg.norm(ti - t) <= 1e-6 and np.abs(Ri - np.eye(3)).max() <= 1e-6


# ---- the ABI ------------------------------------------------------------------------------------
def test_abi_version_and_layout_are_unchanged(rva):
    """The feature adds functions only: the version is still 8 and node/abi_check (the C11 consumer
    of include/at_api.h) reports the layout recorded before it (tests/golden/abi_layout_v8.json)."""
    assert rva.load_library().at_abi_version() == 8
    with open(os.path.join(ROOT, "node", ".build.lock"), "w") as lk:   # one make at a time, as test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", os.path.join(ROOT, "node"), "-s"], check=True, timeout=600)
    r = subprocess.run([os.path.join(ROOT, "node", "abi_check"), "layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(uc.GOLDEN, "abi_layout_v8.json")) as f:
        assert json.loads(r.stdout) == json.load(f)


def test_new_entry_points_are_exported(rva):
    from ros_vision_amd import detector as D
    L = rva.load_library()
    for name in ("at_set_undistort", "at_ideal_detections", "at_ideal_detections_host", "at_undistort_points",
                 "at_undistort_points_host", "at_undistort_stats"):
        assert name in D.EXPORTS and hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "at_api.h")).read()
    assert "#define AT_ABI_VERSION 8" in header


def test_refused_arguments(rva):
    from ros_vision_amd import detector as D
    L = rva.load_library()
    cam = D.AtCamera(fx=900.0, fy=900.0, cx=640.0, cy=400.0, k1=0.05)
    nofx = D.AtCamera(fx=0.0, fy=900.0, cx=640.0, cy=400.0)
    nofy = D.AtCamera(fx=900.0, fy=0.0, cx=640.0, cy=400.0)
    xy, out, ok = (C.c_double * 2)(1.0, 2.0), (C.c_double * 2)(), (C.c_uint8 * 1)()
    det, o = (D.AtDetection * 1)(), (D.AtDetection * 1)()
    bad = [L.at_undistort_points_host(None, xy, 1, out, ok), L.at_undistort_points_host(C.byref(nofx), xy, 1, out, ok),
           L.at_undistort_points_host(C.byref(nofy), xy, 1, out, ok), L.at_undistort_points_host(C.byref(cam), None, 1, out, ok),
           L.at_undistort_points_host(C.byref(cam), xy, 1, None, ok), L.at_undistort_points_host(C.byref(cam), xy, 1, out, None),
           L.at_undistort_points_host(C.byref(cam), xy, -1, out, ok),
           L.at_ideal_detections_host(None, det, 1, o), L.at_ideal_detections_host(C.byref(nofx), det, 1, o),
           L.at_ideal_detections_host(C.byref(cam), None, 1, o), L.at_ideal_detections_host(C.byref(cam), det, 1, None),
           L.at_ideal_detections_host(C.byref(cam), det, -1, o),
           # the detector-side calls refuse a NULL detector before any GPU call
           L.at_set_undistort(None, 1), L.at_ideal_detections(None, 0, o, 1), L.at_undistort_points(None, xy, 1, out, ok),
           L.at_undistort_stats(None, (C.c_uint64 * 2)(), 2)]
    assert bad == [D.AT_E_INVALID] * len(bad)
    assert L.at_undistort_points_host(C.byref(cam), None, 0, None, None) == 0
    assert L.at_ideal_detections_host(C.byref(cam), None, 0, None) == 0


# ---- the twins under sanitizers -------------------------------------------------------------------
def test_sanitized_standalone_program(tmp_path):
    """tests/undistort_host_check.cpp + csrc/at_undist.cpp built with the host compiler and
    -fsanitize=address,undefined (the runtimes linked statically), run as a child process: a grid of
    points through cam11 and through no lens from exact-size heap buffers, cam14's flagged corner,
    NaN and infinity, twelve detections marching into cam14's fold, the refused arguments."""
    exe = tmp_path / "undistort_host_check"
    csrc = os.path.join(ROOT, "ros_vision_amd", "csrc")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-o", str(exe), os.path.join(ROOT, "tests", "undistort_host_check.cpp"),
                    os.path.join(csrc, "at_undist.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "ok" and words[1] == "8004" and int(words[2]) + int(words[3]) == 12 and words[4] == "10"
