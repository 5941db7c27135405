"""The rig track on the GPU: at_rigtrack_solve (the k_trk_* kernels: one workgroup per instant and one
wave per camera for the sums, one workgroup for the block-tridiagonal solve) against its CPU twin
at_rigtrack_solve_host over the same window, byte for byte on every record; the window sliding on
the device with the own starts kept there; that a solve leaves a detector's pending batch alone;
rendered frames through real detectors and the fuser end to end; the profiled kernel times.  The
cases are tests/rig_track_cases.py's, the ones the twin is held to the numpy restatement on in
tests/test_rig_track_host.py."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import rig_calib_cases as cc
import rig_pose_cases as rc
import rig_track_cases as tc
import tag_scenes as ts

pytestmark = pytest.mark.gpu

W, H = 640, 480
NO_DIST = SimpleNamespace(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)   # the frames are drawn without lens distortion


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def records(trk, solve):
    """(result, result record bytes, instant record bytes) of one solve."""
    got = solve()
    return got, bytes(trk.record), trk.instant_records()


def check_equal(trk):
    got, got_r, got_i = records(trk, trk.solve)
    want, want_r, want_i = records(trk, trk.solve_host)
    assert tc.same_result(got, want), (got, want)
    assert got_r == want_r and got_i == want_i
    return got


# ---- device against the CPU twin ------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 16])
def test_two_instants_one_camera_one_tag(rva, iters):
    rng = np.random.default_rng(901)
    win = tc.far_window(tc.far_walk(2, rng), rng)
    trk = tc.tracker(rva, [tc.FAR_CAM], win, layout=tc.FAR_LAYOUT, iters=iters)
    got = check_equal(trk)
    assert got.n == 2 and got.with_tags == 2 and got.cov_valid and got.accepted + got.rejected == iters


@pytest.mark.parametrize("iters", [1, 16])
def test_three_instants_two_cameras_tagless_middle(rva, iters):
    rng = np.random.default_rng(902)
    win = tc.make_window([0, 1], tc.walk(3, rng), rng, noise_px=0.3, tagless=(1,), noisy_odom=True)
    trk = tc.tracker(rva, tc.cameras([0, 1]), win, iters=iters)
    got = check_equal(trk)
    inst = trk.instants()
    assert got.with_tags == 2 and got.cov_valid and inst[1].n_tags == 0 and inst[1].R.any() and got.accepted > 0


@pytest.mark.parametrize("iters", [1, 16])
def test_the_cap_64_instants_8_cameras(rva, iters):
    """Mounts 0..3 twice; camera 2 sees nothing and camera 5 only a foreign tag in some instants; the
    first two and the last instant see nothing at all."""
    rng = np.random.default_rng(903)
    mounts = [0, 1, 2, 3, 0, 1, 2, 3]
    robots = tc.walk(tc.MAX_WINDOW, rng)
    win = tc.make_window(mounts, robots, rng, noise_px=0.3, tagless=(0, 1, 30, 63), blind={7: [2], 8: [2, 3], 40: [0]},
                         noisy_odom=True)
    for k in (5, 21):                                           # a foreign-only view
        win[k].cams[5] = rc.make_instant(["foreign"], rng, robot=robots[k])[0]
    trk = tc.tracker(rva, tc.cameras(mounts), win, iters=iters)
    got = check_equal(trk)
    inst = trk.instants()
    assert got.n == 64 and got.with_tags == 60 and got.cov_valid and got.accepted > 0
    assert inst[0].n_tags == 0 and inst[63].n_tags == 0 and inst[0].R.any() and inst[63].R.any()


def test_accepted_and_rejected_steps_equal_the_twin(rva):
    cams, win = tc.accept_reject_case()
    trk = tc.tracker(rva, cams, win, iters=16)
    got = check_equal(trk)
    assert got.accepted > 0 and got.rejected > 0


# ---- the window on the device ----------------------------------------------------------------------
def test_a_slide_solved_after_every_push(rva):
    """14 pushes through a window of 8, instants 3, 4 and 9 without a tag: the device keeps every
    stored instant and its own start in its slot of the ring; each solve equals the twin's."""
    rng = np.random.default_rng(904)
    win = tc.make_window([0, 1], tc.walk(14, rng), rng, noise_px=0.3, tagless=(3, 4, 9), noisy_odom=True)
    trk = rva.RigTracker(tc.as_create_args(tc.cameras([0, 1])), rc.RIG_LAYOUT, window=8, iters=4)
    for k, inst in enumerate(win):
        assert tc.push(trk, inst) == min(k + 1, 8)
        got = check_equal(trk)
        assert got.n == min(k + 1, 8) and got.stamp == inst.stamp
    first, first_r, first_i = records(trk, trk.solve)
    again, again_r, again_i = records(trk, trk.solve)          # two solves in a row
    assert first_r == again_r and first_i == again_i


def test_restart_and_clear(rva):
    rng = np.random.default_rng(905)
    win = tc.make_window([0, 1], tc.walk(7, rng), rng, noise_px=0.3, noisy_odom=True)
    trk = rva.RigTracker(tc.as_create_args(tc.cameras([0, 1])), rc.RIG_LAYOUT, window=5, iters=4)
    for inst in win[:4]:
        tc.push(trk, inst)
    check_equal(trk)
    win[4].odom = None                                          # odometry lost: a new chain
    assert tc.push(trk, win[4]) == 1 and tc.push(trk, win[5]) == 2
    got = check_equal(trk)
    assert got.n == 2
    trk.clear()
    with pytest.raises(rva.FieldPoseError):
        trk.solve()
    win[5].odom = None
    tc.push(trk, win[5])
    tc.push(trk, win[6])
    fresh = tc.tracker(rva, tc.cameras([0, 1]), [win[5], win[6]], window=5, iters=4)
    a, a_r, a_i = records(trk, trk.solve)
    b, b_r, b_i = records(fresh, fresh.solve)
    assert a_r == b_r and a_i == b_i
    check_equal(trk)


def test_solve_while_a_detector_has_a_batch_pending(rva):
    """The tracker's stream is its own: a detector's batch enqueued before the solve and collected
    after it gives what it gives without a solve in between."""
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
    rng = np.random.default_rng(906)
    win = tc.make_window([0, 1], tc.walk(5, rng), rng, noise_px=0.3, tagless=(2,), noisy_odom=True)
    trk = tc.tracker(rva, tc.cameras([0, 1]), win)
    want = trk.solve_host()
    det.enqueue_host([frame.ctypes.data], rva.AT_FMT_GRAY8)
    got = trk.solve()
    det.collect()
    assert len(plain[0]) == 3 and snapshot() == plain
    assert tc.same_result(got, want)
    det.close()


# ---- stats ------------------------------------------------------------------------------------------
def test_stats_report_the_kernel_times_while_profiling(rva):
    rng = np.random.default_rng(907)
    win = tc.make_window([0, 1], tc.walk(6, rng), rng, noise_px=0.3, tagless=(4,), noisy_odom=True)
    trk = tc.tracker(rva, tc.cameras([0, 1]), win)
    got = trk.solve()
    assert trk.stats()["kernel_ns"] == 0
    trk.set_profiling(True)
    again = trk.solve()
    stats = trk.stats()
    print("track kernels, 2 cameras x 6 instants: %.1f us (accumulate %.1f, solve %.1f)"
          % (stats["kernel_ns"] / 1e3, stats["accum_ns"] / 1e3, stats["solve_ns"] / 1e3))
    assert stats["kernel_ns"] > 0 and stats["accum_ns"] > 0 and stats["solve_ns"] > 0 and tc.same_result(got, again)
    assert stats["window"] == 6 and stats["tags_used"] == sum(i.n_tags for i in trk.instants())
    assert stats["accepted_steps"] == got.accepted and stats["rejected_steps"] == got.rejected


# ---- end to end -------------------------------------------------------------------------------------
def test_rendered_frames_through_the_fuser(rva, tmp_path):
    """Four rendered 640 x 480 instants of three cameras through ApriltagsDetectorNodes and
    RigPoseFuser(tracker=...), the third instant blank in every camera, exact odometry between the
    drawn robot poses: every instant is pushed, the tracked pose goes out on .../rig/tracked, the
    blank instant gets a pose from its odometry, and the device solve equals the twin."""
    from ros_vision_amd import node
    codes = ts.codes()
    views = list(cc.E2E_VIEWS)
    cfg = {"camera_mounted_positions": {v: {"location": v} for v in views},
           "extrinsics": {v: {"rotation": rc.view_mount(v)[0].tolist(), "offset": rc.view_mount(v)[1].tolist()}
                          for v in views}}
    (tmp_path / "system_config.json").write_text(json.dumps(cfg))
    for v in views:
        c = rc.VIEWS[v][5]
        (tmp_path / ("calibrationmatrix_%s.json" % v)).write_text(json.dumps(
            {"matrix": [[c.fx, 0, c.cx], [0, c.fy, c.cy], [0, 0, 1]], "disto": [[0.0] * 5]}))
    nodes = [node.ApriltagsDetectorNode(W, H, {"camera_serial": v}, str(tmp_path), str(tmp_path / "system_config.json"))
             for v in views]
    cams = [SimpleNamespace(cam=rc.VIEWS[v][5], ER=rc.view_mount(v)[0], Et=rc.view_mount(v)[1]) for v in views]
    trk = rva.RigTracker(tc.as_create_args(cams), rc.RIG_LAYOUT, window=4, iters=6)
    sent, rig_sent = [], []
    fuser = node.RigPoseFuser(nodes, rc.RIG_LAYOUT, publishers={"camera/pose/rig/tracked": sent.append,
                                                               "camera/pose/rig": rig_sent.append}, tracker=trk)
    assert fuser.tracked_pose_topic == "camera/pose/rig/tracked"
    robots = cc.E2E_ROBOTS[:4]
    blank = ts.blank()
    for k, robot in enumerate(robots):
        for n, v in zip(nodes, views):
            img = blank if k == 2 else cc.render_mounted_view(v, robot, ts.draw_tag, codes, ts.blank)
            n.image_callback(img, 0.0, encoding="mono8")
        od = None if k == 0 else tc.odom_between(robots[k - 1], robot)
        pose = fuser.publish(odometry=od, stamp_s=1.0 + k)
        assert (pose.n_tags == 0) == (k == 2) and fuser.tracked is not None and fuser.tracked.stamp == 1.0 + k
    assert len(sent) == 4 and len(rig_sent) == 3 and len(trk) == 4
    got = check_equal(trk)
    inst = trk.instants()
    errs = [tc.pose_error((i.R, i.t), r)[1] * 1e3 for i, r in zip(inst, robots)]
    print("tracked position errors: " + ", ".join("%.2f mm" % e for e in errs) + "; rms %.3f px" % got.rms_after)
    assert [i.n_tags > 0 for i in inst] == [True, True, False, True]
    assert np.array_equal(sent[-1][0], got.R) and np.array_equal(sent[-1][1], got.t) and np.array_equal(sent[-1][2], got.cov)
    # The rendering's quantisation leaves the rig pose of these frames 1.358 mm off at the true mounts
    # (profiles/rig_calib/end_to_end.txt); a tracked instant, the blank one hanging on its neighbours by
    # exact odometry, is held to twice that, as test_rig_calib_gpu.py holds its own end-to-end figure.
    # Measured on the MI355X: 0.66, 0.80, 0.82, 0.85 mm.
    assert max(errs) <= 2.0 * 1.358
    fuser.close()
    trk.close()
    for n in nodes:
        n.close()
