"""The rig pose on the CPU (no GPU): at_rig_pose_host against the numpy restatement in
tests/rig_pose_cases.py bit for bit, the Jacobian against central differences, against the field
pose and the truth on exact corners, the covariance against the scatter of 400 noisy solves, and
the WPILib layout reader.  at_rig_pose_host shares its arithmetic with k_rig (csrc/at_rigpose.h),
so what holds here is what the device path is then held to in tests/test_rig_pose_gpu.py."""
import ctypes as C
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import field_pose_cases as fc
import rig_pose_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = 1e-9      # tests/test_pose.py's bound for exact data
EIGHT = [0, None, 1, "foreign", 2, None, 3, None]


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def host(rva, cams, layout=rc.RIG_LAYOUT, **kw):
    return rva.rig_pose_host(rc.as_host_args(cams), layout, **kw)


# ---- the twin against the restatement ------------------------------------------------------------
@pytest.mark.parametrize("mounts", [[0], [0, 1], [1, None, 2], EIGHT], ids=["1", "2", "3", "8"])
def test_host_equals_the_restatement_bit_for_bit(rva, mounts):
    """1, 2, 3 and 8 cameras, among them cameras that see nothing and one that sees only a foreign
    id; exact and noisy corners; a duplicate of a tag with a worse hamming in one camera."""
    rng = np.random.default_rng(766)
    for noise in (0.0, 0.3, 0.3, 1.0):
        cams = rc.make_instant(mounts, rng, noise_px=noise)
        if noise == 1.0:
            seen = next(c for c in cams if c.dets)
            bad = SimpleNamespace(**vars(seen.dets[0]))
            bad.p, bad.hamming = np.asarray(bad.p) + 25.0, 1
            seen.dets.insert(0, bad)
            seen.poses.insert(0, SimpleNamespace(**vars(seen.poses[0])))
        ref = rc.solve_rig_ref(cams, rc.RIG_LAYOUT, max_hamming=1)
        got = host(rva, cams, max_hamming=1)
        want_tags = [len(rc.mount(k)[0]) if isinstance(k, int) else 0 for k in mounts]
        assert got.tags_per_cam == want_tags + [0] * (8 - len(mounts)) and got.n_tags == sum(want_tags)
        assert got.n_cams_used == sum(1 for m in want_tags if m) and got.dropped == 0
        assert got.steps_taken == ref.steps_taken and got.rejected == ref.rejected == rc.ITERS - got.steps_taken
        assert rc.same_record(got, ref), (mounts, noise)
        assert got.cov_valid and np.abs(got.R @ got.R.T - np.eye(3)).max() <= 1e-12
        assert np.abs(got.cov - got.cov.T).max() <= 1e-9 * np.abs(got.cov).max()


def test_no_layout_tag_anywhere(rva):
    rng = np.random.default_rng(1)
    for mounts in ([None], [None, "foreign", None]):
        cams = rc.make_instant(mounts, rng)
        got = host(rva, cams)
        assert rc.same_record(got, rc.solve_rig_ref(cams, rc.RIG_LAYOUT))
        assert got.n_tags == 0 and got.n_cams_used == 0 and not got.R.any() and not got.t.any() and not got.cov.any()
        assert not got.cov_valid and got.rms_px == 0 and got.steps_taken == 0 and got.rejected == 0


# ---- the Jacobian ---------------------------------------------------------------------------------
def test_jacobian_against_central_differences():
    """d(u, v)/d(w, dt) of the restatement's own functions, R' = R dR(w), t' = t + dt, against
    central differences at step 1e-6.  Each column is held to 1e-6 of its largest entry: the
    difference quotient's rounding error is about eps |u| / h = 2e-16 * 600 / 1e-6 ~ 1e-7 px per
    unit, its truncation error of order h^2, against columns of 300 px per unit and more."""
    rng = np.random.default_rng(3)
    h = 1e-6
    worst = 0.0
    for k in range(4):
        ids, ER, Et, cam = rc.mount(k)
        c = rc.rig_camera([], [], cam, ER, Et)
        R, t = fc.small_rotation(rng, 4.0) @ rc.ROBOT[0], rc.ROBOT[1] + rng.normal(scale=0.05, size=3)
        where = {g[0]: g for g in rc.RIG_LAYOUT}
        X = np.concatenate([fc.tag_corners_field(where[i][1], where[i][2]) for i in ids])
        ju, jv, P = rc.jacobian_rows(c, R, t, X)
        assert (P[:, 2] > 0).all()
        for p in range(6):
            d = np.zeros(6)
            d[p] = h
            plus, minus = rc.project_rig(c, *rc.apply_step(R, t, d), X), rc.project_rig(c, *rc.apply_step(R, t, -d), X)
            num = (plus - minus) / (2 * h)
            for col, ana in ((num[:, 0], ju[:, p]), (num[:, 1], jv[:, p])):
                worst = max(worst, np.abs(col - ana).max() / max(np.abs(ju[:, p]).max(), np.abs(jv[:, p]).max()))
    print("Jacobian: worst relative difference %.3g" % worst)
    assert worst <= 1e-6


# ---- exact corners --------------------------------------------------------------------------------
def test_one_camera_agrees_with_the_field_pose(rva):
    """Identity extrinsics: the rig pose is the field pose inverted -- two parameterisations of
    one minimum, on exact corners."""
    rng = np.random.default_rng(11)
    for name in ("coplanar", "two_walls"):
        layout = fc.LAYOUTS[name]
        for _ in range(10):
            R, t = fc.random_camera(rng)
            dets, poses = fc.make_frame(layout, R, t, rng)
            fp = rva.field_pose_host(dets, poses, layout)
            got = host(rva, [rc.rig_camera(dets, poses, fc.CAM)], layout)
            assert got.n_tags == fp.n_tags == len(layout) and got.ids[0] == fp.ids
            assert np.abs(got.R - fp.R.T).max() <= EXACT and np.abs(got.t + fp.R.T @ fp.t).max() <= EXACT


@pytest.mark.parametrize("mounts", [[0, 1], [0, 1, 2, 3]], ids=["2", "4"])
def test_exact_corners_give_the_robot_pose(rva, mounts):
    """Every tag's own pose is 3 degrees and 3 cm off; 40 robot poses."""
    rng = np.random.default_rng(971)
    worst = np.zeros(3)
    for _ in range(40):
        robot = (fc.small_rotation(rng, 3.0) @ rc.ROBOT[0], rc.ROBOT[1] + rng.uniform(-0.04, 0.04, 3))
        got = host(rva, rc.make_instant(mounts, rng, robot=robot))
        assert got.n_cams_used == len(mounts)
        worst = np.maximum(worst, [np.abs(got.R - robot[0]).max(), np.abs(got.t - robot[1]).max(), got.rms_px])
    print(mounts, "worst |dR| %.3g |dt| %.3g rms %.3g" % tuple(worst))
    assert worst[0] <= EXACT and worst[1] <= EXACT and worst[2] < EXACT


# ---- the covariance -------------------------------------------------------------------------------
def test_covariance_matches_the_scatter(rva):
    """400 draws of 0.3 px corner noise, two cameras with three tags each, fixed seed: for each
    of the six parameters the empirical variance of the error (w from R_true^T R, robot frame; t
    in the field frame) over the mean reported variance lies in [0.7, 1.4] -- the sampling error
    of a variance over 400 draws is about 7 %.  solve_rig_ref alone on this scene and seed gives
    the same ratios (its records are the library's bit for bit; checked over all 400 draws)."""
    rng = np.random.default_rng(2026)
    Rr, tr = rc.ROBOT
    err, var = [], []
    for _ in range(400):
        got = host(rva, rc.make_instant([0, 1], rng, noise_px=0.3))
        assert got.cov_valid and got.tags_per_cam[:2] == [3, 3]
        dR = Rr.T @ got.R
        w = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
        err.append(np.concatenate([w, got.t - tr]))
        var.append(np.diag(got.cov))
    ratio = (np.array(err) ** 2).mean(0) / np.array(var).mean(0)
    print("variance ratios (w, t):", np.round(ratio, 3))
    assert (ratio >= 0.7).all() and (ratio <= 1.4).all()


# ---- the WPILib layout ----------------------------------------------------------------------------
WPILIB = os.path.join(ROOT, "tests", "golden", "rig", "wpilib_layout.json")


def test_wpilib_layout_rotation():
    """WPILib's tag frame is x out of the face, z up (y by right-handedness); at_pose's is x right,
    y down, z into the tag: x_at = +y_wpi, y_at = -z_wpi, z_at = -x_wpi."""
    from ros_vision_amd import node
    layout = {tid: (R, t) for tid, R, t in node.load_field_layout(WPILIB)}
    assert sorted(layout) == [1, 2, 3, 4, 5]
    R, t = layout[1]                                   # identity quaternion at the origin
    assert np.array_equal(R, np.array([[0.0, 0, -1], [1, 0, 0], [0, -1, 0]])) and not t.any()
    assert np.array_equal(R @ [1, 0, 0], [0, 1, 0]) and np.array_equal(R @ [0, 1, 0], [0, 0, -1])
    assert np.array_equal(R @ [0, 0, 1], [-1, 0, 0])
    for R, _t in layout.values():
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0
    R, t = layout[2]                                   # turned about z by 180 degrees: faces -x
    assert np.abs(R @ [0, 0, 1] - [1, 0, 0]).max() <= 1e-15 and np.array_equal(t, [4.0, 0.32, 0.5])
    # this project's own format still reads
    own = node.load_field_layout([(7, np.eye(3), [1, 2, 3])])
    assert own[0][0] == 7 and np.array_equal(own[0][2], [1.0, 2.0, 3.0])


def test_wpilib_layout_round_trip_through_a_rendered_scene(rva):
    """A frame drawn from the WPILib-frame description itself -- each tag's upright picture spans
    y (to the viewer's right) and z (up) of its WPILib frame, seen from +x -- through the CPU
    oracle's detector and pose, and the rig solve with the layout load_field_layout read: the
    robot's pose is the scene's.  Bound: 10 mm and 0.01 rad; the corners of rendered tags are
    found to about 0.3 px (the rms of the rendered GPU scenes), which is 1.5 mm of position
    standard deviation at this range by the solve's own covariance, while a wrong axis anywhere
    in the convention turns a tag by 90 degrees or more."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ao
    import tag_scenes as ts
    from ros_vision_amd import node
    cam = fc.GPU_CAM
    # the robot: x forward, y left, z up (WPILib's), 1.3 m in front of the wall x = 4, turned a little
    Rr = fc.rot_xyz(1.5, -2.0, 4.0)
    tr = np.array([2.6, 0.03, 0.55])
    ER, Et = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]]), np.array([0.1, 0.0, 0.06])   # camera z = robot x
    Rc, tc = rc.camera_in_field(Rr, tr, ER, Et)
    with open(WPILIB) as f:
        data = json.load(f)
    img = ts.blank()
    codes = ts.codes()
    h = fc.TAG_SIZE / 2 * fc.QUIET
    drawn = []
    for g in data["tags"]:
        if g["ID"] == 1:
            continue                                   # at the origin, behind the camera
        q, p = g["pose"]["rotation"]["quaternion"], g["pose"]["translation"]
        Rw = fc._quat_to_R(q["W"], q["X"], q["Y"], q["Z"])
        # TL, TR, BR, BL of the upright picture in the tag's WPILib frame
        corners = np.array([[0, -h, h], [0, h, h], [0, h, -h], [0, -h, -h]]) @ Rw.T + [p["x"], p["y"], p["z"]]
        px, z = fc.project(cam, Rc, tc, corners)
        assert (z > 0).all() and px.min() >= 0 and (px[:, 0] <= 639).all() and (px[:, 1] <= 479).all()
        ts.draw_tag(img, codes[g["ID"]], px)
        drawn.append(g["ID"])
    orc = ao.Oracle(640, 480)
    orc.detect(img, 2)
    dets = [SimpleNamespace(**d) for d in orc.detections()]
    assert [d.id for d in dets] == drawn == [2, 3, 4, 5]
    poses = []
    for d in dets:
        R, t, e, _both, _second = ao.estimate_tag_pose(d.H, d.p, cam.fx, cam.fy, cam.cx, cam.cy, fc.TAG_SIZE)
        poses.append(SimpleNamespace(id=d.id, R=R, t=t, err=e))
    got = host(rva, [rc.rig_camera(dets, poses, cam, ER, Et)], node.load_field_layout(WPILIB))
    dR = Rr.T @ got.R
    angle = math.acos(min(1.0, (np.trace(dR) - 1) / 2))
    print("WPILib round trip: |dt| %.2f mm, angle %.2g rad, rms %.2f px" % (np.linalg.norm(got.t - tr) * 1e3, angle,
                                                                           got.rms_px))
    assert got.n_tags == 4 and got.ids[0] == [2, 3, 4, 5]
    assert np.linalg.norm(got.t - tr) <= 0.010 and angle <= 0.01 and got.rms_px < 1.5


# ---- records and refusals ---------------------------------------------------------------------------
def test_record_layout(rva):
    from ros_vision_amd.detector import AtRigExtrinsics, AtRigHostCam, AtRigPose
    assert C.sizeof(AtRigExtrinsics) == 96 and C.sizeof(AtRigPose) == 960 and C.sizeof(AtRigHostCam) == 128
    assert AtRigPose.ids.offset == 40 and AtRigPose.R.offset == 552 and AtRigPose.cov.offset == 648
    assert AtRigPose.rms_px.offset == 936 and AtRigPose.dropped.offset == 956
    assert rva.load_library().at_abi_version() == 8


def test_refused_arguments(rva):
    rng = np.random.default_rng(5)
    cams = rc.make_instant([0, 1], rng)

    def refused(cams, layout=rc.RIG_LAYOUT, **kw):
        with pytest.raises(rva.FieldPoseError) as e:
            host(rva, cams, layout, **kw)
        return e.value.code == -1

    assert refused([]) and refused(cams * 5)                              # n_cams outside 1..8
    assert refused(cams, tag_size=0.0) and refused(cams, max_hamming=-1)
    assert refused(cams, []) and refused(cams, rc.RIG_LAYOUT + [fc.wall_a(1024, 0, 0)])
    assert refused(cams, rc.RIG_LAYOUT + [fc.wall_a(3, 1.0, 1.0)])        # an id twice
    assert refused(cams, rc.RIG_LAYOUT + [(9, 1.00001 * np.eye(3), np.zeros(3))])
    skew = rc.rig_camera(cams[0].dets, cams[0].poses, cams[0].cam, np.diag([1.0, 1.0, -1.0]), np.zeros(3))
    assert refused([skew, cams[1]])                                       # extrinsics that are no rotation
    assert host(rva, cams * 4).n_tags == 24                               # 8 cameras: the cap is fine


# ---- the twin under sanitizers ------------------------------------------------------------------
def test_sanitized_standalone_program(tmp_path):
    """tests/rig_pose_host_check.cpp + csrc/at_rigpose.cpp + csrc/at_fieldpose.cpp built with the
    host compiler and -fsanitize=address,undefined (the runtimes linked statically), run as a child
    process: the 8-camera instant (two cameras see nothing, from NULL arrays), the empty instant,
    one camera, from exact-size heap buffers; the refused calls."""
    exe = tmp_path / "rig_pose_host_check"
    csrc = os.path.join(ROOT, "ros_vision_amd", "csrc")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-o", str(exe), os.path.join(ROOT, "tests", "rig_pose_host_check.cpp"),
                    os.path.join(csrc, "at_rigpose.cpp"), os.path.join(csrc, "at_fieldpose.cpp")],
                   check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "3", "8"]
