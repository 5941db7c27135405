"""The camera calibration on the CPU (no GPU): at_camcal_solve_host against the numpy restatement in
tests/camera_calib_cases.py bit for bit, the Jacobian against central differences, exact corners of
a real lens and its 20 board poses against scipy's least squares, the focal guess, the covariance
against the scatter of 400 noisy solves, the behaviour cases, refusals and the node's helpers.
at_camcal_solve_host shares its arithmetic with the k_cc_* kernels (csrc/at_camcal.h), so what holds
here is what the device path is then held to in tests/test_camera_calib_gpu.py."""
import ctypes as C
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import camera_calib_cases as cc
import field_pose_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = {0, 1, 4, 5}


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


# ---- the Jacobian ---------------------------------------------------------------------------------
# Worst relative difference measured (each column against its largest entry): 1.7e-9
# (the translation along z; the intrinsics' columns 3e-10 and less).
JACOBIAN_MEASURED = 1.7e-9


def test_jacobian_against_central_differences():
    """d(u, v)/d(intrinsics) (additive) and d(u, v)/d(w, dt) (R' = dR(w) R, t' = t + dt) of the
    restatement's own rows -- the expressions of cc_slot_rows -- against central differences of the
    forward model at the cam13 camera and its first four poses, step 1e-3 for an intrinsic value,
    1e-6 rad and 1e-5 units for the pose; each column is held to ten times the relative difference measured."""
    cam, poses = cc.cam13()
    X = np.concatenate([fc.tag_corners_field(Rt, tt, cc.CAM13_TAG) for _tid, Rt, tt in cc.CAM13_BOARD])
    scale = [1e3] * 9 + [1.0] * 3 + [10.0] * 3     # (the model is linear in each intrinsic value)
    worst, per = 0.0, np.zeros(15)
    for R, t in poses[:4]:
        uv, z = cc.project(cam, R, t, X)
        assert (z > 0).all()
        jpu, jpv, jiu, jiv, ru, rv = cc.rows(list(cam), cc.ALL, R, t, X, uv)
        assert np.abs(ru).max() < 1e-9 and np.abs(rv).max() < 1e-9
        for p in range(15):
            h = 1e-6 * scale[p]
            both = []
            for sgn in (1.0, -1.0):
                c, Rn, tn = cam.copy(), R, t
                if p < 9:
                    c[p] += sgn * h
                elif p < 12:
                    w = np.zeros(3)
                    w[p - 9] = sgn * h
                    Rn = cc.rodrigues(w) @ R
                else:
                    tn = t.copy()
                    tn[p - 12] += sgn * h
                both.append(cc.project(c, Rn, tn, X)[0])
            num = (both[0] - both[1]) / (2 * h)
            au, av = (jiu[:, p], jiv[:, p]) if p < 9 else (jpu[:, p - 9], jpv[:, p - 9])
            top = max(np.abs(au).max(), np.abs(av).max())
            per[p] = max(per[p], np.abs(num[:, 0] - au).max() / top, np.abs(num[:, 1] - av).max() / top)
    worst = per.max()
    print("calibration Jacobian: worst relative difference %.3g" % worst)
    assert worst <= 10 * JACOBIAN_MEASURED


# ---- the twin against the restatement ----------------------------------------------------------------
def check_against_restatement(rva, views, board, tag_size, **kw):
    cal = cc.calibrator(rva, views, board, tag_size, **kw)
    got = cal.solve_host()
    ref = cc.solve_ref(views, board, tag_size, *cc.CAM13_SIZE, **kw)
    assert cc.same_result(got, ref), (got, ref)
    assert cc.same_views(cal.views(), ref.views)
    return cal, got, ref


def test_host_equals_the_restatement_1_tag_3_views(rva):
    cam, views = cc.many_views(3, np.random.default_rng(766), noise_px=0.3, ids={5})
    _cal, got, _ref = check_against_restatement(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.FX | cc.FY,
                                                init=cc.off_start(cam))
    assert got.views_used == 3 and got.corners == 12 and got.accepted > 0 and np.array_equal(got.params[2:],
                                                                                            cc.off_start(cam)[2:])


@pytest.mark.parametrize("guess", [False, True])
def test_host_equals_the_restatement_4_tags_5_views_all_free(rva, guess):
    cam, views = cc.many_views(5, np.random.default_rng(767), noise_px=0.3, ids=FOUR)
    _cal, got, _ref = check_against_restatement(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.ALL,
                                                init=None if guess else cc.off_start(cam))
    assert got.views_used == 5 and got.cov_valid and got.accepted > 0 and got.rms_after < got.rms_before


def test_host_equals_the_restatement_33_views(rva):
    """A partial second chunk; view 17 is skipped."""
    cam, views = cc.many_views(33, np.random.default_rng(768), noise_px=0.3, ids=FOUR)
    views[17] = cc.behind_view(cc.CAM13_BOARD, cam, cc.CAM13_TAG)
    _cal, got, _ref = check_against_restatement(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.ALL & ~cc.K3,
                                                init=cc.off_start(cam), max_hamming=1)
    assert got.views_used == 32 and got.views_skipped == 1 and got.cov_valid and got.params[8] == 0.0


# ---- exact corners of a real lens ---------------------------------------------------------------------
# Measured (worst relative parameter error against the file's camera, all nine free):
#   start 15 % / 20 px off: the twin 5.9e-13, scipy 7.9e-13; from the focal guess: 4.9e-13, 6.2e-13.
# The focal guess alone lands 3.0 % (fx) and 4.3 % (fy) above the truth: its principal point is the
# frame's centre, 42 px from the lens's, and the corners are distorted.
def _scipy_fit(ref0, views, board, tag_size):
    """scipy.optimize.least_squares on the same residuals (cc.project minus the corners) from the
    same start: the restatement's start intrinsics and start poses (iters = 0), each pose moved by a
    rotation vector on the left and a translation."""
    from scipy.optimize import least_squares
    lay = {g[0]: (g[1], g[2]) for g in board}
    pts = [(np.concatenate([fc.tag_corners_field(*lay[d.id], tag_size) for d in dets]),
            np.concatenate([d.p for d in dets])) for dets in cc.stored_views(views, board)]
    R0 = [v.R for v in ref0.views]

    def resid(x):
        out = []
        for i, (X, uv) in enumerate(pts):
            px, _z = cc.project(x[:9], cc.rodrigues(x[9 + 6 * i:12 + 6 * i]) @ R0[i], x[12 + 6 * i:15 + 6 * i], X)
            out.append((px - uv).ravel())
        return np.concatenate(out)

    x0 = np.concatenate([ref0.start] + [np.concatenate([np.zeros(3), v.t]) for v in ref0.views])
    sol = least_squares(resid, x0, method="lm", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=20000)
    return sol.x[:9], 2.0 * sol.cost


@pytest.mark.parametrize("guess", [False, True])
def test_exact_corners_against_scipy(rva, guess):
    """The cam13 fixture: exact corners of all 20 views.  The twin's parameter error against the
    truth is no worse than max(10 x scipy's, 1e-9 relative), and its cost exceeds scipy's by no more
    than rounding: both costs are sums of about 2500 squared residuals of rounding size (1e-13 px
    each, a cost of order 1e-23), so `rounding` is that size, 1e-20, not a fraction of either."""
    cam, board, tag_size, views = cc.cam13_case()
    init = None if guess else cc.off_start(cam)
    cal = cc.calibrator(rva, views, board, tag_size, free=cc.ALL, init=init)
    got = cal.solve_host()
    ref0 = cc.solve_ref(views, board, tag_size, *cc.CAM13_SIZE, free=cc.ALL, init=init, iters=0)
    if guess:
        print("focal guess: fx %+.2f %%, fy %+.2f %% from the truth" % tuple(100 * (ref0.start[:2] - cam[:2]) / cam[:2]))
    sp, sp_cost = _scipy_fit(ref0, views, board, tag_size)
    e_twin, e_scipy = (np.abs(got.params - cam) / np.abs(cam)).max(), (np.abs(sp - cam) / np.abs(cam)).max()
    cost = got.rms_after ** 2 * got.corners
    print("worst relative error: twin %.3g, scipy %.3g; cost %.3g against %.3g" % (e_twin, e_scipy, cost, sp_cost))
    assert got.views_used == 20 and got.cov_valid
    assert e_twin <= max(10 * e_scipy, 1e-9)
    assert cost <= sp_cost + 1e-20


def test_the_guess_reaches_the_optimum_of_a_given_start(rva):
    """Noisy corners: the solve from the focal guess ends where the solve from the 15 % start ends
    (both at the one minimum: parameters to 1e-6 relative, costs to 1e-9)."""
    cam, board, tag_size, views = cc.cam13_case(rng=np.random.default_rng(5), noise_px=0.3)
    a = cc.calibrator(rva, views, board, tag_size, free=cc.ALL, init=cc.off_start(cam)).solve_host()
    b = cc.calibrator(rva, views, board, tag_size, free=cc.ALL, init=None).solve_host()
    assert np.allclose(a.params, b.params, rtol=1e-6, atol=1e-9) and abs(a.rms_after - b.rms_after) <= 1e-9 * a.rms_after


# ---- the reported variances ------------------------------------------------------------------------------
def test_covariance_matches_the_scatter(rva):
    """400 draws of 0.3 px corner noise on the first 10 cam13 views, all nine free, fixed seed: for
    every parameter the empirical variance of the error over the mean reported variance lies in
    [0.75, 1.3] -- the variance of 400 samples has a standard error of sqrt(2 / 399), about 7 %, so
    this is +-3 sigma with a little room."""
    cam, board, tag_size, views = cc.cam13_case(n_views=10)
    rng = np.random.default_rng(2026)
    cal = rva.CameraCalibrator(*cc.CAM13_SIZE, board, tag_size, free=cc.ALL, init=cc.off_start(cam))
    err, var = [], []
    for _ in range(400):
        cal.clear()
        for v in cc.renoise(views, rng, 0.3):
            assert cal.add(v)
        got = cal.solve_host()
        assert got.cov_valid and got.rms_after < got.rms_before
        err.append(got.params - cam)
        var.append(np.diag(got.cov))
    ratio = (np.array(err) ** 2).mean(0) / np.array(var).mean(0)
    print("variance ratios:", dict(zip(cc.NAMES, np.round(ratio, 3))))
    assert (ratio >= 0.75).all() and (ratio <= 1.3).all()


# ---- behaviour ----------------------------------------------------------------------------------------------
def test_free_mask_zero_scores_a_calibration(rva):
    """free_mask = 0: `init` comes back bit for bit and the cost is the sum of the per-view fits --
    each view alone gives the same cost (the views share only the damping and the accept rule; at
    the minimum the cost is flat to second order: 1e-9 relative)."""
    cam, views = cc.many_views(4, np.random.default_rng(31), noise_px=0.3, ids=FOUR)
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=0, init=cam)
    got = cal.solve_host()
    assert np.array_equal(got.params, cam) and got.cov_valid and not got.cov.any()
    alone = 0.0
    for v in views:
        one = cc.calibrator(rva, [v], cc.CAM13_BOARD, cc.CAM13_TAG, free=0, init=cam).solve_host()
        alone += one.rms_after ** 2 * one.corners
    assert abs(got.rms_after ** 2 * got.corners - alone) <= 1e-9 * alone
    assert all(abs(r.rms_px - 0.3) < 0.25 for r in cal.views())


@pytest.mark.parametrize("free", [cc.FX | cc.FY, cc.PINHOLE, cc.ALL & ~cc.K3, cc.K1 | cc.K2, cc.ALL & ~cc.CX])
def test_a_parameter_that_is_not_free_comes_back_bit_equal(rva, free):
    cam, views = cc.many_views(5, np.random.default_rng(32), noise_px=0.3, ids=FOUR)
    init = cc.off_start(cam)
    init[4:] = cam[4:] * 0.5
    got = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=free, init=init).solve_host()
    for p in range(9):
        if (free >> p) & 1:
            assert got.params[p] != init[p], cc.NAMES[p]
        else:
            assert got.params[p] == init[p] and not got.cov[p].any() and not got.cov[:, p].any(), cc.NAMES[p]


def test_a_skipped_view(rva):
    cam, views = cc.many_views(3, np.random.default_rng(33), noise_px=0.3, ids=FOUR)
    views.insert(1, cc.behind_view(cc.CAM13_BOARD, cam, cc.CAM13_TAG))
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.PINHOLE, init=cc.off_start(cam))
    got = cal.solve_host()
    recs = cal.views()
    assert len(cal) == 4 and got.views_used == 3 and got.views_skipped == 1 and got.corners == 48
    assert not recs[1].used and not recs[1].R.any() and recs[1].n_tags == 0 and all(recs[k].used for k in (0, 2, 3))
    assert cal.stats() == {"views_used": 3, "views_skipped": 1, "accepted_steps": got.accepted,
                           "rejected_steps": got.rejected, "kernel_ns": 0}


def test_the_seventeenth_tag_is_dropped(rva):
    board = cc.grid_board(3, 6, 0, 2.0, 2.6)
    cam, poses = cc.cam13()
    views = [cc.make_view(board, cam, R, t, 2.0, *cc.CAM13_SIZE, ids=set(range(17))) for R, t in poses[:3]]
    assert all(len(v) == 17 for v in views)
    cal = cc.calibrator(rva, views, board, 2.0, free=cc.PINHOLE, init=cc.off_start(cam))
    got = cal.solve_host()
    ref = cc.solve_ref([v[:16] for v in views], board, 2.0, *cc.CAM13_SIZE, free=cc.PINHOLE, init=cc.off_start(cam))
    assert got.corners == 4 * 16 * 3 and cc.same_result(got, ref)


def test_one_view_of_one_tag_has_no_covariance(rva):
    """8 residuals, 6 + 9 unknowns: the denominator is not positive."""
    cam, views = cc.many_views(1, np.random.default_rng(34), noise_px=0.3, ids={5})
    got = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.ALL, init=cc.off_start(cam)).solve_host()
    assert got.views_used == 1 and got.corners == 4 and not got.cov_valid and not got.cov.any()


def test_fronto_parallel_views_give_no_focal_guess(rva):
    cam = np.array([900.0, 900.0, 640.0, 400.0, 0, 0, 0, 0, 0])
    views = [cc.make_view(cc.CAM13_BOARD, cam, np.eye(3), np.array([-6.0, -6.0, z]), cc.CAM13_TAG, *cc.CAM13_SIZE)
             for z in (30.0, 40.0)]
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.PINHOLE, init=None)
    with pytest.raises(rva.FieldPoseError) as e:
        cal.solve_host()
    assert e.value.code == -1 and cc.solve_ref(views, cc.CAM13_BOARD, cc.CAM13_TAG, *cc.CAM13_SIZE, init=None) is None


def test_record_layouts(rva):
    from ros_vision_amd import detector as d
    assert C.sizeof(d.AtCamcalConfig) == 88 and C.sizeof(d.AtCamcalResult) == 72 + 648 + 16 + 24
    assert C.sizeof(d.AtCamcalView) == 112 and rva.AT_CAMCAL_MAX_VIEWS == cc.MAX_VIEWS == 4096
    assert rva.load_library().at_abi_version() == 8
    assert [getattr(rva, "AT_CAMCAL_" + n.upper()) for n in cc.NAMES] == [1 << p for p in range(9)]


def test_refused_arguments(rva):
    cam, views = cc.many_views(1, np.random.default_rng(5), ids=FOUR)
    board, ts = cc.CAM13_BOARD, cc.CAM13_TAG

    def refused(*a, **kw):
        with pytest.raises(rva.FieldPoseError) as e:
            rva.CameraCalibrator(*a, **kw)
        return e.value.code == -1

    assert refused(1280, 800, board, ts, free=512, init=cam) and refused(1280, 800, board, ts, free=-1, init=cam)
    assert refused(0, 800, board, ts, init=cam) and refused(1280, -1, board, ts, init=cam)
    assert refused(1280, 800, board, 0.0, init=cam) and refused(1280, 800, board, -1.0, init=cam)
    bad = cam.copy()
    bad[0] = 0.0
    assert refused(1280, 800, board, ts, init=bad)
    bad = cam.copy()
    bad[1] = -5.0
    assert refused(1280, 800, board, ts, init=bad)
    assert refused(1280, 800, board, ts, init=cam, max_hamming=-1)
    assert refused(1280, 800, [], ts, init=cam)
    assert refused(1280, 800, board + [board[0]], ts, init=cam)                          # an id twice
    assert refused(1280, 800, [(0, 2.0 * np.eye(3), np.zeros(3))], ts, init=cam)         # no rotation
    assert refused(1280, 800, [(1024, np.eye(3), np.zeros(3))], ts, init=cam)            # an id outside the table
    cal = rva.CameraCalibrator(1280, 800, board, ts, init=None)                          # (no camera needed with a guess)
    with pytest.raises(rva.FieldPoseError) as e:
        cal.solve_host()                                                                 # no stored view
    assert e.value.code == -1
    other = [SimpleNamespace(id=77, hamming=0, decision_margin=50.0, H=np.eye(3), c=np.zeros(2), p=np.zeros((4, 2)))]
    assert not cal.add(other) and not cal.add([]) and len(cal) == 0
    worse = [SimpleNamespace(id=d.id, hamming=2, decision_margin=50.0, H=d.H, c=d.c, p=d.p) for d in views[0]]
    assert not cal.add(worse) and cal.add(views[0]) and len(cal) == 1
    cal.clear()
    assert len(cal) == 0 and cal.views() == []


def test_the_4097th_view_is_refused(rva):
    cam, views = cc.many_views(1, np.random.default_rng(6), ids={5})
    cal = rva.CameraCalibrator(*cc.CAM13_SIZE, cc.CAM13_BOARD, cc.CAM13_TAG, init=cam)
    L = rva.load_library()
    from ros_vision_amd.detector import _detection_records
    arr, n = _detection_records(views[0])
    for _ in range(4096):
        assert L.at_camcal_add(cal._h, arr, n) == 1
    assert L.at_camcal_add(cal._h, arr, n) == -3 and len(cal) == 4096
    with pytest.raises(rva.FieldPoseError) as e:
        cal.add(views[0])
    assert e.value.code == -3


# ---- the node's helpers ----------------------------------------------------------------------------------
def test_save_camera_calibration_round_trip(tmp_path, rva):
    from ros_vision_amd import node
    cam, _poses = cc.cam13()
    res = rva.CameraCalibration(params=cam, cov=np.zeros((9, 9)), cov_valid=False, rms_before=1.0, rms_after=0.25,
                                views_used=20, views_skipped=0, corners=1264, accepted=10, rejected=20)
    path = node.save_camera_calibration(str(tmp_path), "cam13", res.camera_matrix, res.distortion_coefficients,
                                        res.rms_after, extra={"views": 20})
    assert os.path.basename(path) == "calibrationmatrix_cam13.json"
    cm, dc = node.load_camera_calibration(str(tmp_path), "cam13")
    assert cm == res.camera_matrix and dc == res.distortion_coefficients
    assert [cm.fx, cm.fy, cm.cx, cm.cy, dc.k1, dc.k2, dc.p1, dc.p2, dc.k3] == list(cam)
    with open(path) as f:
        data = json.load(f)
    assert data["method"] == "apriltag_board" and data["rmse_reprojection_error"] == 0.25 and data["views"] == 20
    assert len(data["disto"]) == 1 and len(data["disto"][0]) == 5 and data["matrix"][2] == [0.0, 0.0, 1.0]


def test_grid_board():
    from ros_vision_amd import node
    got = node.grid_board(2, 3, 10, 0.1, 0.14)
    want = cc.grid_board(2, 3, 10, 0.1, 0.14)
    assert [g[0] for g in got] == [10, 11, 12, 13, 14, 15]
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) for a, b in zip(got, want))
    assert np.array_equal(got[4][2], [0.14, 0.14, 0.0]) and np.array_equal(got[2][1], np.eye(3))
    for bad in ((0, 3, 0, 0.1, 0.14), (2, 3, -1, 0.1, 0.14), (2, 3, 0, 0.1, 0.1), (2, 3, 0, 0.0, 0.14)):
        with pytest.raises(ValueError):
            node.grid_board(*bad)


def test_the_collector_takes_every_nth_frame_up_to_max():
    from ros_vision_amd import node

    class Fake:
        def __init__(self):
            self.views = []

        def add(self, dets):
            self.views.append(dets)
            return True

        def __len__(self):
            return len(self.views)

    seen = [SimpleNamespace(id=3)]
    col = node.CameraCalibrationCollector(Fake(), every=3, max_frames=2)
    col.board_ids = {3}
    assert [col.offer(seen) for _ in range(2)] == [False, False] and not col.offer([SimpleNamespace(id=9)])
    assert [col.offer(seen) for _ in range(3)] == [False, False, True]          # the run started again
    assert not col.done and [col.offer(seen) for _ in range(3)] == [False, False, True] and col.done
    assert not col.offer(seen) and len(col.calibrator) == 2
    with pytest.raises(ValueError):
        node.CameraCalibrationCollector(Fake(), every=0)


# ---- the stand-alone sanitized program -------------------------------------------------------------------
def test_sanitized_standalone_program(tmp_path):
    """tests/camera_calib_host_check.cpp + csrc/at_camcal.cpp, at_fieldpose.cpp built with the host
    compiler and -fsanitize=address,undefined (the runtimes linked statically), run as a child
    process: 35 frames from exact-size heap buffers (one with only a foreign id, one empty), the host
    solve on exact corners of a distorted camera, the records, clear, the refused calls, and a
    second calibrator with the focal guess."""
    exe = tmp_path / "camera_calib_host_check"
    csrc = os.path.join(ROOT, "ros_vision_amd", "csrc")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-o", str(exe), os.path.join(ROOT, "tests", "camera_calib_host_check.cpp"),
                    os.path.join(csrc, "at_camcal.cpp"), os.path.join(csrc, "at_fieldpose.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "34", "2", "10"]
