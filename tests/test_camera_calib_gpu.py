"""The camera calibration on the GPU: at_camcal_solve (the k_cc_* kernels: one wave per view, one
lane per corner; the reduced 9 x 9 solve in one workgroup) against its CPU twin
at_camcal_solve_host over the same stored views, bit for bit on every record; that a solve leaves no
state behind and leaves a detector's pending batch alone; and rendered frames through a real
detector end to end.  The cases are tests/camera_calib_cases.py's, the ones the twin is held to the
numpy restatement on in tests/test_camera_calib_host.py."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import camera_calib_cases as cc
import field_pose_cases as fc
import tag_scenes as ts

pytestmark = pytest.mark.gpu

W, H = 640, 480
NO_DIST = SimpleNamespace(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)   # views are recorded with zero distortion
FOUR = {0, 1, 4, 5}


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def check_equal(cal):
    got = cal.solve()
    got_v = cal.views()
    want = cal.solve_host()
    assert cc.same_result(got, want), (got, want)
    assert cc.same_views(got_v, cal.views())
    return got


def noisy(n, seed, ids=None, noise_px=0.3):
    rng = np.random.default_rng(seed)
    cam, views = cc.many_views(n, rng, noise_px=noise_px, ids=ids)
    return cam, views


# ---- device against the CPU twin ------------------------------------------------------------------
@pytest.mark.parametrize("n, ids, free", [(1, FOUR, cc.FX | cc.FY), (3, {5}, cc.FX | cc.FY), (3, FOUR, cc.ALL),
                                          (31, FOUR, cc.ALL), (32, FOUR, cc.ALL), (33, None, cc.ALL),
                                          (65, FOUR, cc.ALL)])
def test_view_and_tag_counts_equal_the_twin(rva, n, ids, free):
    """1, 3, 31, 32 (a full chunk), 33 (a partial one) and 65 (a third) views of 1, 4 and 16 tags
    (every lane live)."""
    cam, views = noisy(n, 800 + n, ids)
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=free, init=cc.off_start(cam))
    assert len(cal) == n
    got = check_equal(cal)
    assert got.views_used == n and got.accepted > 0 and got.rms_after < got.rms_before
    assert got.corners == 4 * sum(len(v) for v in views)       # (a tag that leaves the frame is not drawn)
    assert max(v.n_tags for v in cal.views()) == (16 if ids is None else len(ids))


def test_the_seventeenth_tag_is_dropped(rva):
    """A 3 x 6 board, 17 of its tags offered: the 16 lowest ids are used."""
    board = cc.grid_board(3, 6, 0, 2.0, 2.6)
    cam, poses = cc.cam13()
    rng = np.random.default_rng(811)
    views = [cc.make_view(board, cam, R, t, 2.0, *cc.CAM13_SIZE, rng=rng, noise_px=0.3, ids=set(range(17)))
             for R, t in poses[:4]]
    assert all(len(v) == 17 for v in views)
    cal = cc.calibrator(rva, views, board, 2.0, free=cc.PINHOLE, init=cc.off_start(cam))
    got = check_equal(cal)
    assert got.corners == 4 * 16 * 4 and all(v.n_tags == 16 for v in cal.views())


def test_a_view_that_takes_no_part_in_the_middle_of_a_chunk(rva):
    cam, views = noisy(12, 812, FOUR)
    views[5] = cc.behind_view(cc.CAM13_BOARD, cam, cc.CAM13_TAG)
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.ALL, init=cc.off_start(cam))
    assert len(cal) == 12
    got = check_equal(cal)
    recs = cal.views()
    assert got.views_used == 11 and got.views_skipped == 1 and not recs[5].used and recs[4].used and recs[6].used
    assert not recs[5].R.any() and recs[5].rms_px == 0 and got.accepted > 0


@pytest.mark.parametrize("free", [0, cc.FX | cc.FY, cc.PINHOLE, cc.ALL, cc.ALL & ~cc.K3])
@pytest.mark.parametrize("guess", [False, True])
def test_masks_and_the_focal_guess_equal_the_twin(rva, free, guess):
    cam, views = noisy(6, 813, FOUR)
    start = cc.off_start(cam)
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=free, init=None if guess else start)
    got = check_equal(cal)
    begin = cc.solve_ref(views, cc.CAM13_BOARD, cc.CAM13_TAG, *cc.CAM13_SIZE, free=free, init=None if guess else start,
                         iters=0).start
    for p in range(9):
        if not (free >> p) & 1:
            assert got.params[p] == begin[p], cc.NAMES[p]
    assert got.rms_after <= got.rms_before and (got.accepted > 0 or not free)


def test_accepted_and_rejected_steps_equal_the_twin(rva):
    """6 noisy views: the solve converges in a few accepted steps, after which the cost no longer
    falls and the remaining iterations are rejected."""
    cam, views = noisy(6, 814, FOUR)
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.PINHOLE, init=cc.off_start(cam))
    got = check_equal(cal)
    assert got.accepted > 0 and got.rejected > 0 and got.accepted + got.rejected == cc.ITERS


# ---- no state left over ---------------------------------------------------------------------------
def test_two_solves_in_a_row_and_a_solve_after_clear(rva):
    cam, views = noisy(7, 815, FOUR)
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.ALL, init=cc.off_start(cam))
    first = cal.solve()
    first_v = cal.views()
    again = cal.solve()
    assert cc.same_result(first, again) and cc.same_views(first_v, cal.views())
    cal.clear()
    with pytest.raises(rva.FieldPoseError):
        cal.solve()
    for v in views[:4]:                                    # fewer, other views in the same buffers
        assert cal.add(v)
    four = check_equal(cal)
    assert four.views_used == 4 and not cc.same_result(four, first)
    for v in views[4:]:
        assert cal.add(v)
    assert cc.same_result(cal.solve(), first) and cc.same_views(cal.views(), first_v)


def test_solve_while_a_detector_has_a_batch_pending(rva):
    """The calibrator's stream is its own: a detector's batch enqueued before the solve and
    collected after it gives what it gives without a solve in between."""
    codes = ts.codes()
    frame = np.ascontiguousarray(cc.render_board_view(0, ts.draw_tag, codes, ts.blank))
    g = fc.GPU_CAM
    det = rva.GpuDetector(W, H, rva.CameraMatrix(fx=g.fx, cx=g.cx, fy=g.fy, cy=g.cy), NO_DIST, max_batch=1)

    def snapshot():
        return [(x.id, x.hamming, x.decision_margin, np.array(x.H).tobytes(), np.array(x.p).tobytes())
                for x in det.detections(0)]

    det.detect(frame, rva.AT_FMT_GRAY8)
    plain = snapshot()
    cam, views = noisy(5, 816, FOUR)
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.ALL, init=cc.off_start(cam))
    want = cal.solve_host()
    det.enqueue_host([frame.ctypes.data], rva.AT_FMT_GRAY8)
    got = cal.solve()
    det.collect()
    assert len(plain) == 6 and snapshot() == plain
    assert cc.same_result(got, want)
    det.close()


# ---- stats ------------------------------------------------------------------------------------------
def test_stats_report_the_kernel_time_while_profiling(rva):
    cam, views = noisy(4, 817, FOUR)
    cal = cc.calibrator(rva, views, cc.CAM13_BOARD, cc.CAM13_TAG, free=cc.ALL, init=cc.off_start(cam))
    got = cal.solve()
    assert cal.stats()["kernel_ns"] == 0
    cal.set_profiling(True)
    again = cal.solve()
    stats = cal.stats()
    print("calibration kernels, 4 views x 4 tags: %.1f us" % (stats["kernel_ns"] / 1e3))
    assert stats["kernel_ns"] > 0 and cc.same_result(got, again)
    assert stats["views_used"] == 4 and stats["views_skipped"] == 0
    assert stats["accepted_steps"] == got.accepted and stats["rejected_steps"] == got.rejected


# ---- end to end -------------------------------------------------------------------------------------
def test_rendered_frames_end_to_end(rva):
    """Six rendered views of a 2 x 3 board through a detector with zero distortion into the
    calibrator, the four pinhole values free, no initial camera.  The true camera with refitted
    poses is a feasible point of the problem minimised, so a converged solve cannot be worse than
    it: rms_after within 1 % (the iteration cap) of a free_mask = 0 run at the truth."""
    codes = ts.codes()
    g = fc.GPU_CAM
    det = rva.GpuDetector(W, H, rva.CameraMatrix(fx=g.fx, cx=g.cx, fy=g.fy, cy=g.cy), NO_DIST, max_batch=1)
    cal = rva.CameraCalibrator(W, H, cc.E2E_BOARD, cc.E2E_TAG, free=cc.PINHOLE, init=None)
    truth = rva.CameraCalibrator(W, H, cc.E2E_BOARD, cc.E2E_TAG, free=0, init=cc.E2E_CAM)
    for k in range(len(cc.E2E_VIEWS)):
        det.detect(np.ascontiguousarray(cc.render_board_view(k, ts.draw_tag, codes, ts.blank)), rva.AT_FMT_GRAY8)
        dets = det.detections(0)
        assert cal.add(dets) and truth.add(dets)
    det.close()
    got = check_equal(cal)
    ref = truth.solve()
    line = ("camera from %d rendered views (%d corners): fx %.3f fy %.3f cx %.3f cy %.3f against %.1f %.1f %.1f %.1f; "
            "rms %.4f -> %.4f px, %.4f px at the true camera; %d accepted, %d rejected"
            % (got.views_used, got.corners, *got.params[:4], *cc.E2E_CAM[:4], got.rms_before, got.rms_after,
               ref.rms_after, got.accepted, got.rejected))
    print(line)
    out = os.environ.get("AT_CAMCAL_E2E_OUT")
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
    assert got.views_used == len(cc.E2E_VIEWS) and got.cov_valid and ref.views_used == got.views_used
    assert np.array_equal(ref.params, cc.E2E_CAM)
    assert got.rms_after <= 1.01 * ref.rms_after
