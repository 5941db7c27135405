"""The rig calibration on the GPU: at_rigcal_solve (the k_cal_* kernels: one workgroup per instant,
one wave per camera; the reduced solve in one workgroup) against its CPU twin
at_rigcal_solve_host over the same stored instants, bit for bit on every record; that a solve
leaves no state behind and leaves a detector's pending batch alone; and rendered frames through
real detectors end to end.  The cases are tests/rig_calib_cases.py's, the ones the twin is held to
the numpy restatement on in tests/test_rig_calib_host.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import rig_calib_cases as cc
import rig_pose_cases as rc
import tag_scenes as ts

pytestmark = pytest.mark.gpu

W, H = 640, 480
NO_DIST = SimpleNamespace(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)   # the frames are drawn without lens distortion


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def both(cal):
    """(GPU result and instants, twin result and instants) of one calibrator."""
    got = cal.solve()
    got_i = cal.instants()
    want = cal.solve_host()
    return got, got_i, want, cal.instants()


def check_equal(cal):
    got, got_i, want, want_i = both(cal)
    assert cc.same_result(got, want), (got, want)
    assert cc.same_instants(got_i, want_i)
    return got


# ---- device against the CPU twin ------------------------------------------------------------------
def test_two_cameras_three_instants_equal_the_twin(rva):
    _true, start, instants = cc.two_camera_case(np.random.default_rng(766), 3, noise_px=0.3)
    cal, _kept = cc.calibrator(rva, start, instants)
    got = check_equal(cal)
    assert got.cov_valid and got.instants_used == 3 and got.accepted > 0 and got.rms_after < got.rms_before


@pytest.mark.parametrize("n", [33, 65])
def test_partial_and_third_chunk_equal_the_twin(rva, n):
    """33 instants: a partial last chunk; 65: a third chunk.  Camera 2 (free_rot only) sees nothing
    in instants 4, 17 and 32."""
    _true, start, instants = cc.three_camera_case(np.random.default_rng(767), n)
    cal, _kept = cc.calibrator(rva, start, instants, max_hamming=1)
    got = check_equal(cal)
    assert got.cov_valid and got.instants_used == n and got.accepted > 0


def test_an_instant_that_takes_no_part_in_the_middle_of_a_chunk(rva):
    """Instant 5 of 12 holds tags whose own poses all put a corner behind a camera: it is stored
    (two cameras have tags), gets no start and is skipped."""
    rng = np.random.default_rng(768)
    _true, start, instants = cc.two_camera_case(rng, 12, noise_px=0.3)
    for c in instants[5]:
        for p in c.poses:
            p.t = -np.asarray(p.t)
    cal, kept = cc.calibrator(rva, start, instants)
    assert len(kept) == 12
    got = check_equal(cal)
    recs = cal.instants()
    assert got.instants_used == 11 and got.instants_skipped == 1 and not recs[5].used and recs[4].used and recs[6].used
    assert not recs[5].R.any() and recs[5].rms_px == 0 and got.accepted > 0


def test_eight_cameras_equal_the_twin(rva):
    """Camera 3 sees nothing in instants 1 and 6, camera 5 is free_rot only, camera 6 free_trans only."""
    _true, start, instants = cc.eight_camera_case(np.random.default_rng(769), 9, noise_px=0.3, blind={1: [3], 6: [3]})
    cal, _kept = cc.calibrator(rva, start, instants)
    got = check_equal(cal)
    assert got.cov_valid and got.instants_used == 9 and got.accepted > 0
    assert np.array_equal(got.t[5], start[5].Et) and np.array_equal(got.R[6], start[6].ER)


def test_never_shared_camera_fails_the_factor_alike(rva):
    start, instants = cc.never_shared_case()
    cal, _kept = cc.calibrator(rva, start, instants)
    got = check_equal(cal)
    assert not got.cov_valid and got.accepted == 0 and got.rejected == cc.ITERS and not any(c.any() for c in got.cov)
    for R, t, c in zip(got.R, got.t, start):
        assert np.array_equal(R, c.ER) and np.array_equal(t, c.Et)


def test_accepted_and_rejected_steps_equal_the_twin(rva):
    start, instants = cc.accept_reject_case()
    cal, _kept = cc.calibrator(rva, start, instants)
    got = check_equal(cal)
    assert got.accepted > 0 and got.rejected > 0


# ---- no state left over ---------------------------------------------------------------------------
def test_two_solves_in_a_row_and_a_solve_after_clear(rva):
    rng = np.random.default_rng(770)
    _true, start, instants = cc.two_camera_case(rng, 7, noise_px=0.3)
    cal, kept = cc.calibrator(rva, start, instants)
    first = cal.solve()
    first_i = cal.instants()
    again = cal.solve()
    assert cc.same_result(first, again) and cc.same_instants(first_i, cal.instants())
    cal.clear()
    with pytest.raises(rva.FieldPoseError):
        cal.solve()
    for inst in kept[:4]:                                  # fewer, other instants in the same buffers
        assert cal.add(cc.as_add_args(inst))
    four = check_equal(cal)
    assert four.instants_used == 4 and not cc.same_result(four, first)
    for inst in kept[4:]:
        assert cal.add(cc.as_add_args(inst))
    assert cc.same_result(cal.solve(), first) and cc.same_instants(cal.instants(), first_i)


def test_solve_while_a_detector_has_a_batch_pending(rva):
    """The calibrator's stream is its own: a member detector's batch enqueued before the solve
    and collected after it gives what it gives without a solve in between."""
    codes = ts.codes()
    frame = np.ascontiguousarray(rc.render_view("front", ts.draw_tag, codes, ts.blank))
    cam = rc.VIEWS["front"][5]
    det = rva.GpuDetector(W, H, rva.CameraMatrix(fx=cam.fx, cx=cam.cx, fy=cam.fy, cy=cam.cy), NO_DIST, max_batch=1)

    def snapshot():
        return ([(x.id, x.hamming, x.decision_margin, np.array(x.H).tobytes(), np.array(x.p).tobytes())
                 for x in det.detections(0)], [(p.id, np.array(p.R).tobytes(), np.array(p.t).tobytes(), p.err)
                                               for p in det.poses(0)])

    det.detect(frame, rva.AT_FMT_GRAY8)
    plain = snapshot()
    _true, start, instants = cc.two_camera_case(np.random.default_rng(771), 5, noise_px=0.3)
    cal, _kept = cc.calibrator(rva, start, instants)
    want = cal.solve_host()
    det.enqueue_host([frame.ctypes.data], rva.AT_FMT_GRAY8)
    got = cal.solve()
    det.collect()
    assert len(plain[0]) == 3 and snapshot() == plain
    assert cc.same_result(got, want)
    det.close()


# ---- stats ------------------------------------------------------------------------------------------
def test_stats_report_the_kernel_time_while_profiling(rva):
    _true, start, instants = cc.two_camera_case(np.random.default_rng(772), 4, noise_px=0.3)
    cal, _kept = cc.calibrator(rva, start, instants)
    got = cal.solve()
    assert cal.stats()["kernel_ns"] == 0
    cal.set_profiling(True)
    again = cal.solve()
    stats = cal.stats()
    print("calibration kernels, 2 cameras x 4 instants: %.1f us" % (stats["kernel_ns"] / 1e3))
    assert stats["kernel_ns"] > 0 and cc.same_result(got, again)
    assert stats["instants_used"] == 4 and stats["instants_skipped"] == 0
    assert stats["accepted_steps"] == got.accepted and stats["rejected_steps"] == got.rejected


# ---- end to end -------------------------------------------------------------------------------------
# Robot position errors (mm) of RigSolver on the rendered instants, measured on the MI355X
# (profiles/rig_calib/end_to_end.txt): with the perturbed initial mounts, with the calibrated
# mounts, with the true mounts.  Only the rendering's quantisation separates runs, so the
# calibrated mounts are held to twice the error measured there.
E2E_CALIBRATED_MM = 2.482   # initial mounts 64.235 mm, calibrated 2.482 mm, true mounts 1.358 mm


def test_rendered_frames_end_to_end(rva):
    codes = ts.codes()
    views = list(cc.E2E_VIEWS)
    cams = [rc.VIEWS[v][5] for v in views]
    dets = [rva.GpuDetector(W, H, rva.CameraMatrix(fx=c.fx, cx=c.cx, fy=c.fy, cy=c.cy), NO_DIST, max_batch=1)
            for c in cams]
    rng = np.random.default_rng(773)
    true = [SimpleNamespace(cam=c, ER=rc.view_mount(v)[0], Et=rc.view_mount(v)[1], free_rot=True, free_trans=True)
            for c, v in zip(cams, views)]
    true[0] = cc.fixed(true[0])
    start = [true[0]] + [cc.perturbed(c, rng) for c in true[1:]]
    cal = rva.RigCalibrator(cc.as_create_args(start), rc.RIG_LAYOUT)
    frames = [[cc.render_mounted_view(v, robot, ts.draw_tag, codes, ts.blank) for v in views] for robot in cc.E2E_ROBOTS]
    for per in frames:
        for d, fr in zip(dets, per):
            d.detect(fr, rva.AT_FMT_GRAY8)
        assert cal.add([(d.detections(0), d.poses(0)) for d in dets])
    got = check_equal(cal)
    assert got.instants_used == len(frames) and got.cov_valid and got.rms_after < got.rms_before

    def robot_error(mounts):
        rig = rva.RigSolver(dets, mounts, rc.RIG_LAYOUT)
        worst = 0.0
        for per, robot in zip(frames, cc.E2E_ROBOTS):
            for d, fr in zip(dets, per):
                d.detect(fr, rva.AT_FMT_GRAY8)
            worst = max(worst, float(np.linalg.norm(rig.solve()[0].t - robot[1])))
        rig.close()
        return worst * 1e3

    e_start = robot_error([(c.ER, c.Et) for c in start])
    e_cal = robot_error(list(zip(got.R, got.t)))
    e_true = robot_error([(c.ER, c.Et) for c in true])
    line = "robot position error, worst of %d instants: initial mounts %.3f mm, calibrated %.3f mm, true %.3f mm; " \
           "rms %.3f -> %.3f px" % (len(frames), e_start, e_cal, e_true, got.rms_before, got.rms_after)
    print(line)
    for d in dets:
        d.close()
    assert e_cal < e_start
    assert e_cal <= 2.0 * E2E_CALIBRATED_MM
