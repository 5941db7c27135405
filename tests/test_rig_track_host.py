"""The rig track on the CPU (no GPU): at_rigtrack_solve_host against the numpy restatement in
tests/rig_track_cases.py bit for bit, the odometry Jacobian against central differences, the final
cost against scipy, the covariance against the scatter of 400 noisy solves, dropouts, what smoothing
gains on a far tag, the window's mechanics, refusals, the fuser's new arguments and the host side
under sanitizers.  at_rigtrack_solve_host shares its arithmetic with the k_trk_* kernels
(csrc/at_rigtrack.h), so what holds here is what the device path is then held to in
tests/test_rig_track_gpu.py."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import field_pose_cases as fc
import rig_pose_cases as rc
import rig_track_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def records(trk, solve):
    got = solve()
    return got, bytes(trk.record), trk.instant_records()


# ---- the Jacobian ---------------------------------------------------------------------------------
def test_odometry_jacobian_against_central_differences():
    """d(rho, tau)/d(w, dt) of the restatement's own rows for both poses, R' = R dR(w), t' = t + dt,
    against central differences at step 1e-6, each column held to 1e-6 of its largest entry:
    test_rig_pose_host.py's Jacobian bound.  Its argument carries over: the residuals are O(1) per
    sigma, rounding in the difference is about 1e-16 / sigma / 2e-6 -- 1e-8 per unit against columns
    of 1 / sigma = 250 per unit -- and the truncation is of order h^2."""
    rng = np.random.default_rng(3)
    h = 1e-6
    worst = 0.0
    for _ in range(8):
        a = (fc.small_rotation(rng, 20.0) @ rc.ROBOT[0], rc.ROBOT[1] + rng.normal(scale=0.2, size=3))
        b = (fc.small_rotation(rng, 5.0) @ a[0], a[1] + rng.normal(scale=0.1, size=3))
        od = tc.odom_between(a, b, rng, 0.004, 0.004, noisy=True)
        od = (od[0] @ tc.rodrigues(rng.normal(scale=0.05, size=3)), od[1] + rng.normal(scale=0.03, size=3), 0.004, 0.003)
        _r, Ja, Jb = tc.odom_rows(a, b, od)
        for which, J in ((0, np.array(Ja)), (1, np.array(Jb))):
            for p in range(6):
                d = np.zeros(6)
                d[p] = h
                plus = [rc.apply_step(*x, d) if i == which else x for i, x in enumerate((a, b))]
                minus = [rc.apply_step(*x, -d) if i == which else x for i, x in enumerate((a, b))]
                num = (tc.odom_residual(*plus, od) - tc.odom_residual(*minus, od)) / (2 * h)
                worst = max(worst, np.abs(num - J[:, p]).max() / np.abs(J[:, p]).max())
    print("odometry Jacobian: worst relative difference %.3g" % worst)
    assert worst <= 1e-6


# ---- the twin against the restatement ----------------------------------------------------------------
def check_against_restatement(rva, cams, win, **kw):
    trk = tc.tracker(rva, cams, win, **kw)
    got = trk.solve_host()
    kw.pop("window", None)
    ref = tc.solve_track_ref(cams, win, **kw)
    assert tc.same_result(got, ref), (got, ref)
    assert tc.same_instants(trk.instants(), ref.instants)
    return trk, got


@pytest.mark.parametrize("iters", [1, 16])
def test_host_equals_the_restatement_2_cameras_tagless_middle(rva, iters):
    rng = np.random.default_rng(766)
    win = tc.make_window([0, 1], tc.walk(3, rng), rng, noise_px=0.3, tagless=(1,), noisy_odom=True)
    trk, got = check_against_restatement(rva, tc.cameras([0, 1]), win, iters=iters)
    inst = trk.instants()
    assert got.cov_valid and got.n == 3 and got.with_tags == 2 and got.accepted + got.rejected == iters
    assert inst[1].n_tags == 0 and inst[1].rms_px == 0 and inst[1].R.any() and inst[0].n_tags == 6


@pytest.mark.parametrize("iters", [1, 16])
def test_host_equals_the_restatement_3_cameras_two_leading_tagless(rva, iters):
    rng = np.random.default_rng(767)
    win = tc.make_window([0, 1, 2], tc.walk(5, rng), rng, noise_px=0.3, tagless=(0, 1), blind={3: [2]}, noisy_odom=True)
    trk, got = check_against_restatement(rva, tc.cameras([0, 1, 2]), win, iters=iters, max_hamming=1, sigma_px=0.3)
    inst = trk.instants()
    assert got.cov_valid and got.with_tags == 3 and [i.n_tags > 0 for i in inst] == [False, False, True, True, True]
    assert got.stamp == win[-1].stamp and [i.stamp for i in inst] == [w.stamp for w in win]


# ---- noise ------------------------------------------------------------------------------------------
def test_noisy_final_cost_against_scipy_least_squares(rva):
    """N = 6, 2 cameras, 0.3 px corner noise, noisy odometry, 16 iterations.  scipy.optimize.least_squares
    on the same residuals (pixels / sigma_px, the odometry rows) from the same start, parameters
    (w, dt) per pose.  Both are minima of one function: the relative excess of the twin's cost is held
    to test_field_map_host.py's bound, 1e-9."""
    from scipy import optimize as scipy_optimize
    rng = np.random.default_rng(11)
    cams = tc.cameras([0, 1])
    win = tc.make_window([0, 1], tc.walk(6, rng), rng, noise_px=0.3, noisy_odom=True)
    trk = tc.tracker(rva, cams, win, iters=16, sigma_px=0.3)
    got = trk.solve_host()
    start, _nt = tc.start_poses(cams, win)
    pts = tc.window_points(cams, win, rc.RIG_LAYOUT, 0, rc.TAG_SIZE)

    def fun(x):
        poses = [(start[k][0] @ tc.rodrigues(x[6 * k:6 * k + 3]), start[k][1] + x[6 * k + 3:6 * k + 6]) for k in range(6)]
        res = []
        for k in range(6):
            for c, (X, uv) in zip(cams, pts[k]):
                res.append(((rc.project_rig(c, *poses[k], X) - uv) / 0.3).reshape(-1))
            if k:
                res.append(tc.odom_residual(poses[k - 1], poses[k], win[k].odom))
        return np.concatenate(res)

    sol = scipy_optimize.least_squares(fun, np.zeros(36), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    scipy_cost = 2.0 * sol.cost
    excess = (got.cost_after - scipy_cost) / scipy_cost
    print("twin %.10f, scipy %.10f, relative excess %.3g; start %.6f" % (got.cost_after, scipy_cost, excess, got.cost_before))
    assert abs(float(np.sum(fun(np.zeros(36)) ** 2)) - got.cost_before) <= 1e-9 * got.cost_before
    assert got.cost_after < got.cost_before and excess <= 1e-9


def test_covariance_matches_the_scatter(rva):
    """400 draws of 0.3 px corner noise (sigma_px = 0.3) and of odometry noise at its stated sigmas on
    an N = 4 window of 2 cameras, fixed seed (test_rig_pose_host.py's
    test_covariance_matches_the_scatter: its repeats and its bounds): for each of the six parameters
    of the latest pose the empirical variance of the error (w from R_true^T R, robot frame; t in the
    field frame) over the mean reported variance lies in [0.7, 1.4].  The numpy restatement runs on
    the same 400 windows: it alone stays inside, and the twin's records equal its bit for bit."""
    rng = np.random.default_rng(2026)
    cams = tc.cameras([0, 1])
    robots = tc.walk(4, rng)
    trk = rva.RigTracker(tc.as_create_args(cams), rc.RIG_LAYOUT, window=4, iters=6, sigma_px=0.3)
    err, var, ref_err, ref_var = [], [], [], []
    for _ in range(400):
        win = tc.make_window([0, 1], robots, rng, noise_px=0.3, noisy_odom=True)
        win[0].odom = None
        for inst in win:
            tc.push(trk, inst)
        got = trk.solve_host()
        ref = tc.solve_track_ref(cams, win, iters=6, sigma_px=0.3)
        assert got.cov_valid and tc.same_result(got, ref)
        for res, e, v in ((got, err, var), (ref, ref_err, ref_var)):
            dR = robots[-1][0].T @ res.R
            w = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
            e.append(np.concatenate([w, res.t - robots[-1][1]]))
            v.append(np.diag(res.cov))
    ratio = (np.array(err) ** 2).mean(0) / np.array(var).mean(0)
    ref_ratio = (np.array(ref_err) ** 2).mean(0) / np.array(ref_var).mean(0)
    print("variance ratios (w, t):", np.round(ratio, 3), "restatement:", np.round(ref_ratio, 3))
    assert (ref_ratio >= 0.7).all() and (ref_ratio <= 1.4).all()
    assert (ratio >= 0.7).all() and (ratio <= 1.4).all()


# ---- what the feature is for ---------------------------------------------------------------------------
def test_dropout_instants_get_poses_from_odometry(rva):
    """N = 8 with instants 3..5 without a tag: they report n_tags = 0 and get poses; their position
    error is below that of holding the last fix (the rig pose of instant 2), the alternative without
    a tracker -- true by construction while the robot moves, so the ratio is printed, not bounded."""
    rng = np.random.default_rng(21)
    cams = tc.cameras([0, 1])
    robots = tc.walk(8, rng)
    win = tc.make_window([0, 1], robots, rng, noise_px=0.3, tagless=(3, 4, 5), noisy_odom=True)
    trk = tc.tracker(rva, cams, win, sigma_px=0.3)
    got = trk.solve_host()
    inst = trk.instants()
    hold = rva.rig_pose_host([(c.dets, c.poses, k.cam, (k.ER, k.Et)) for c, k in zip(win[2].cams, cams)], rc.RIG_LAYOUT)
    assert got.n == 8 and got.with_tags == 5 and hold.n_tags > 0
    tracked = [tc.pose_error((inst[k].R, inst[k].t), robots[k])[1] for k in (3, 4, 5)]
    held = [float(np.linalg.norm(hold.t - robots[k][1])) for k in (3, 4, 5)]
    print("dropout: tracked %s mm, last fix held %s mm, ratio of the means %.3f"
          % (np.round(np.array(tracked) * 1e3, 2), np.round(np.array(held) * 1e3, 2), np.mean(tracked) / np.mean(held)))
    assert all(inst[k].n_tags == 0 and inst[k].rms_px == 0 and abs(np.linalg.det(inst[k].R) - 1) < 1e-9 for k in (3, 4, 5))
    assert all(inst[k].n_tags > 0 for k in (0, 1, 2, 6, 7))
    assert np.mean(tracked) < np.mean(held)


def test_smoothing_helps_on_a_single_far_tag(rva):
    """200 seeded windows of N = 16, one camera, one tag 4.2 m away, 0.3 px noise, odometry noise at
    its stated sigmas: the mean position error of the tracked latest pose is below the rig pose's of
    the same instant.  The restatement runs on the first four windows and equals the twin bit for
    bit, so the twin's gain is the restatement's (the restatement alone over all 200 gave the same
    ratio when this was written: DESIGN 7l).  Nothing tighter than "below" is asserted."""
    rng = np.random.default_rng(77)
    trk = rva.RigTracker(tc.as_create_args([tc.FAR_CAM]), tc.FAR_LAYOUT, window=16, iters=6, sigma_px=0.3)
    e_trk, e_rig = [], []
    for i in range(200):
        robots = tc.far_walk(16, rng)
        win = tc.far_window(robots, rng)
        for inst in win:
            tc.push(trk, inst)
        got = trk.solve_host()
        if i < 4:
            assert tc.same_result(got, tc.solve_track_ref([tc.FAR_CAM], win, layout=tc.FAR_LAYOUT, iters=6, sigma_px=0.3))
        last = win[-1].cams[0]
        rig = rva.rig_pose_host([(last.dets, last.poses, tc.FAR_CAM.cam, (tc.FAR_CAM.ER, tc.FAR_CAM.Et))], tc.FAR_LAYOUT)
        assert rig.n_tags == 1
        e_trk.append(float(np.linalg.norm(got.t - robots[-1][1])))
        e_rig.append(float(np.linalg.norm(rig.t - robots[-1][1])))
    print("far tag: tracked %.2f mm, rig pose %.2f mm, ratio %.3f" % (np.mean(e_trk) * 1e3, np.mean(e_rig) * 1e3,
                                                                   np.mean(e_trk) / np.mean(e_rig)))
    assert np.mean(e_trk) < np.mean(e_rig)


# ---- the window -------------------------------------------------------------------------------------------
def test_sliding_keeps_the_newest_and_cached_starts_change_nothing(rva):
    """window + 6 pushes, a host solve after every push (so every own start is cached): the result
    equals that of a fresh tracker given only the surviving instants.  Instant 6, the oldest survivor,
    has no tag: its start came from its dropped predecessor while that was in the window and comes
    from its successor now."""
    rng = np.random.default_rng(31)
    cams = tc.cameras([0, 1])
    win = tc.make_window([0, 1], tc.walk(14, rng), rng, noise_px=0.3, tagless=(6, 9), noisy_odom=True)
    trk = rva.RigTracker(tc.as_create_args(cams), rc.RIG_LAYOUT, window=8, iters=4)
    for k, inst in enumerate(win):
        assert tc.push(trk, inst) == min(k + 1, 8) == len(trk)
        trk.solve_host()
    a, a_r, a_i = records(trk, trk.solve_host)
    fresh = tc.tracker(rva, cams, win[6:], window=8, iters=4)
    b, b_r, b_i = records(fresh, fresh.solve_host)
    assert a_r == b_r and a_i == b_i and a.n == 8 and a.stamp == win[-1].stamp
    assert [i.stamp for i in trk.instants()] == [w.stamp for w in win[6:]] and trk.instants()[0].n_tags == 0
    ref = tc.solve_track_ref(cams, win[6:], iters=4)
    assert tc.same_result(a, ref) and tc.same_instants(trk.instants(), ref.instants)


def test_lost_odometry_restarts_the_chain(rva):
    rng = np.random.default_rng(32)
    cams = tc.cameras([0, 1])
    win = tc.make_window([0, 1], tc.walk(6, rng), rng, noise_px=0.3, noisy_odom=True)
    trk = tc.tracker(rva, cams, win[:4], window=6)
    win[4].odom = None
    assert tc.push(trk, win[4]) == 1 and tc.push(trk, win[5]) == 2
    a, a_r, a_i = records(trk, trk.solve_host)
    fresh = tc.tracker(rva, cams, win[4:], window=6)
    b, b_r, b_i = records(fresh, fresh.solve_host)
    assert a.n == 2 and a_r == b_r and a_i == b_i
    trk.clear()
    assert len(trk) == 0
    with pytest.raises(rva.FieldPoseError) as e:
        trk.solve_host()
    assert e.value.code == -1


def test_both_accepted_and_rejected_steps(rva):
    cams, win = tc.accept_reject_case()
    _trk, got = check_against_restatement(rva, cams, win, iters=16)
    print("accepted %d rejected %d" % (got.accepted, got.rejected))
    assert got.accepted > 0 and got.rejected > 0 and got.accepted + got.rejected == 16


def test_a_window_without_any_tag_is_refused(rva):
    rng = np.random.default_rng(33)
    cams = tc.cameras([0, 1])
    robots = tc.walk(3, rng)
    win = tc.make_window([0, "foreign"], robots, rng, tagless=(0, 2))
    win[1].cams[0] = rc.make_instant([None], rng)[0]            # (instant 1: one blank, one foreign-only view)
    trk = tc.tracker(rva, cams, win)
    with pytest.raises(rva.FieldPoseError) as e:
        trk.solve_host()
    assert e.value.code == -1 and len(trk) == 3
    assert tc.solve_track_ref(cams, win) is None
    tc.push(trk, tc.make_window([0, 1], robots, rng)[1])        # one with tags: solved, the first three by odometry
    got = trk.solve_host()
    assert got.n == 3 and got.with_tags == 1


def test_the_17th_tag_of_a_camera_is_dropped(rva):
    """A camera with 17 layout tags in view: the 16 lowest ids are kept, as the rig pose selects."""
    rng = np.random.default_rng(34)
    layout = [fc.wall_a(i, -0.8 + 0.2 * (i % 9), -0.2 + 0.4 * (i // 9)) for i in range(17)]
    cam = SimpleNamespace(cam=rc.CAM_A, ER=np.eye(3), Et=np.zeros(3))
    win = []
    for k, robot in enumerate(tc.walk(2, rng)):
        Rc, tcam = rc.camera_in_field(*robot, cam.ER, cam.Et)
        dets, poses = fc.make_frame(layout, Rc, tcam, rng, cam=cam.cam, noise_px=0.3)
        win.append(SimpleNamespace(cams=[rc.rig_camera(dets, poses, cam.cam)], stamp=float(k), robot=robot,
                                   odom=None if k == 0 else tc.odom_between(win[0].robot, robot)))
    trk, got = check_against_restatement(rva, [cam], win, layout=layout)
    assert [i.n_tags for i in trk.instants()] == [16, 16] and got.cov_valid


# ---- records and refusals ---------------------------------------------------------------------------------
def test_record_layouts_and_abi_version(rva):
    from ros_vision_amd import detector as d
    assert rva.load_library().at_abi_version() == 8
    assert rva.AT_RIGTRACK_MAX_WINDOW == tc.MAX_WINDOW == 64
    assert C.sizeof(d.AtRigtrackCamera) == 168 and C.sizeof(d.AtRigtrackOdom) == 112
    assert C.sizeof(d.AtRigtrackResult) == 16 + 32 + 96 + 288 + 8 + 8 and d.AtRigtrackResult.cov.offset == 144
    assert C.sizeof(d.AtRigtrackInstant) == 120 and d.AtRigtrackInstant.n_tags.offset == 112


def test_refused_arguments(rva):
    rng = np.random.default_rng(5)
    cams = tc.cameras([0, 1])
    win = tc.make_window([0, 1], tc.walk(2, rng), rng)

    def refused(cs=cams, layout=rc.RIG_LAYOUT, **kw):
        with pytest.raises(rva.FieldPoseError) as e:
            rva.RigTracker(tc.as_create_args(cs), layout, **kw)
        return e.value.code == -1

    assert refused([]) and refused(cams * 5)                                   # n_cams outside 1..8
    assert refused(tag_size=0.0) and refused(max_hamming=-1) and refused(sigma_px=0.0) and refused(sigma_px=float("nan"))
    assert refused(window=1) and refused(window=65) and refused(iters=0) and refused(iters=17)
    assert refused(layout=[]) and refused(layout=rc.RIG_LAYOUT + [fc.wall_a(1024, 0, 0)])
    assert refused(layout=rc.RIG_LAYOUT + [fc.wall_a(3, 1.0, 1.0)])            # an id twice
    skew = SimpleNamespace(cam=cams[0].cam, ER=np.diag([1.0, 1.0, -1.0]), Et=cams[0].Et)
    assert refused([cams[0], skew])                                            # an R that is no rotation
    rva.RigTracker(tc.as_create_args(cams * 4), rc.RIG_LAYOUT, window=64, iters=16).close()
    rva.RigTracker(tc.as_create_args(cams[:1]), rc.RIG_LAYOUT, window=2, iters=1).close()

    trk = rva.RigTracker(tc.as_create_args(cams), rc.RIG_LAYOUT)
    with pytest.raises(rva.FieldPoseError) as e:                               # nothing stored
        trk.solve_host()
    assert e.value.code == -1
    tc.push(trk, win[0])
    R, t, sr, st = win[1].odom
    for bad in ((np.diag([1.0, 1.0, -1.0]), t, sr, st), (R, [0.0, np.inf, 0.0], sr, st), (R, t, 0.0, st),
                (R, t, sr, -1.0), (R, t, float("nan"), st)):
        with pytest.raises(rva.FieldPoseError) as e:
            trk.push([(c.dets, c.poses) for c in win[1].cams], bad)
        assert e.value.code == -1 and len(trk) == 1                            # (and the window is untouched)
    with pytest.raises(ValueError):
        trk.push([(c.dets, c.poses) for c in win[1].cams][:1], win[1].odom)
    L = rva.load_library()
    assert L.at_rigtrack_push(trk._h, 0.0, None, None) == -1 and L.at_rigtrack_count(None) == -1
    assert L.at_rigtrack_solve_host(trk._h, None) == -1 and L.at_rigtrack_instants(trk._h, None, 1) == -1
    assert tc.push(trk, win[1]) == 2 and trk.solve_host().n == 2


# ---- the node -----------------------------------------------------------------------------------------------
def test_fuser_pushes_every_instant_and_publishes_the_tracked_pose(rva, monkeypatch):
    """RigPoseFuser's new arguments with stand-ins for the solver, the nodes and the tracker: no GPU."""
    from ros_vision_amd import node

    class Solver:
        def __init__(self, *a):
            self.n_tags = 3

        def solve(self):
            return [SimpleNamespace(n_tags=self.n_tags, R=np.eye(3), t=np.zeros(3), cov=np.zeros((6, 6)))]

        def close(self):
            pass

    class Tracker:
        def __init__(self):
            self.pushed, self.fail = [], False

        def push(self, per, odometry=None, stamp=0.0):
            self.pushed.append((per, odometry, stamp))

        def solve(self):
            if self.fail:
                raise rva.FieldPoseError("at_rigtrack_solve", -1)
            return SimpleNamespace(R=2 * np.eye(3), t=np.ones(3), cov=np.eye(6), stamp=self.pushed[-1][2])

    monkeypatch.setattr(node, "RigSolver", Solver)
    det = SimpleNamespace(detections=lambda f: ["d%d" % f], poses=lambda f: ["p%d" % f])
    nodes = [SimpleNamespace(detector=det, extrinsic_rotation=np.eye(3), extrinsic_offset=np.zeros(3),
                             pose_topic="camera/pose", publishers={}) for _ in range(2)]
    sent, rig_sent = [], []
    pubs = {"camera/pose/rig/tracked": sent.append, "camera/pose/rig": rig_sent.append}
    plain = node.RigPoseFuser(nodes, rc.RIG_LAYOUT, publishers=pubs)
    assert plain.tracker is None and plain.publish().n_tags == 3 and len(rig_sent) == 1 and not sent
    trk = Tracker()
    fuser = node.RigPoseFuser(nodes, rc.RIG_LAYOUT, publishers=pubs, tracker=trk)
    assert fuser.tracked_pose_topic == "camera/pose/rig/tracked"
    fuser.publish()                                             # the existing call: a new chain at stamp 0
    assert trk.pushed[-1] == ([(["d0"], ["p0"])] * 2, None, 0.0) and len(sent) == 1 and len(rig_sent) == 2
    fuser.solver.n_tags = 0                                     # an instant without a tag is pushed all the same
    od = (np.eye(3), np.zeros(3), 0.01, 0.01)
    fuser.publish(odometry=od, stamp_s=2.5)
    assert trk.pushed[-1][1] is od and trk.pushed[-1][2] == 2.5 and len(sent) == 2 and len(rig_sent) == 2
    assert np.array_equal(sent[-1][0], 2 * np.eye(3)) and np.array_equal(sent[-1][2], np.eye(6)) and fuser.tracked.stamp == 2.5
    trk.fail = True                                             # no tag in the window yet: nothing goes out
    fuser.publish(odometry=od, stamp_s=3.0)
    assert len(trk.pushed) == 3 and len(sent) == 2 and fuser.tracked is None


# ---- the host side under sanitizers ----------------------------------------------------------------------
def test_sanitized_standalone_program(tmp_path):
    """tests/rig_track_host_check.cpp + csrc/at_rigtrack.cpp, at_rigpose.cpp, at_fieldpose.cpp built
    with the host compiler and -fsanitize=address,undefined (the runtimes linked statically), run
    as a child process: 2 cameras, nine pushes from exact-size heap buffers through a window of six
    (cameras that see nothing from NULL arrays), the host solve, the records, the refused calls, a
    restart and clear."""
    exe = tmp_path / "rig_track_host_check"
    csrc = os.path.join(ROOT, "ros_vision_amd", "csrc")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-o", str(exe), os.path.join(ROOT, "tests", "rig_track_host_check.cpp"),
                    os.path.join(csrc, "at_rigtrack.cpp"), os.path.join(csrc, "at_rigpose.cpp"),
                    os.path.join(csrc, "at_fieldpose.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "6", "4", "13"]
