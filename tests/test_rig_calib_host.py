"""The rig calibration on the CPU (no GPU): at_rigcal_solve_host against the numpy restatement in
tests/rig_calib_cases.py bit for bit, the camera Jacobian against central differences, exact
corners against the true mounts, the covariance against the scatter of 400 noisy solves, the
degenerate cases, refusals and save_extrinsics.  at_rigcal_solve_host shares its arithmetic with the
k_cal_* kernels (csrc/at_rigcal.h), so what holds here is what the device path is then held to in
tests/test_rig_calib_gpu.py."""
import ctypes as C
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import field_pose_cases as fc
import rig_calib_cases as cc
import rig_pose_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = 1e-9      # tests/test_pose.py's bound for exact data


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


# ---- the Jacobian ---------------------------------------------------------------------------------
def test_camera_jacobian_against_central_differences():
    """d(u, v)/d(we, de) of the restatement's own functions, E_R' = E_R dR(we), E_t' = E_t + de,
    against central differences at step 1e-6, each column held to 1e-6 of its largest entry: the
    argument of test_rig_pose_host.py's Jacobian test (rounding about 1e-7 px per unit, truncation
    of order h^2, columns of 300 px per unit and more) holds for these columns as it does there."""
    rng = np.random.default_rng(3)
    h = 1e-6
    worst = 0.0
    for k in range(4):
        ids, _ER, _Et, _cam = rc.mount(k)
        c = cc.true_camera(k)
        R, t = fc.small_rotation(rng, 4.0) @ rc.ROBOT[0], rc.ROBOT[1] + rng.normal(scale=0.05, size=3)
        where = {g[0]: g for g in rc.RIG_LAYOUT}
        X = np.concatenate([fc.tag_corners_field(where[i][1], where[i][2]) for i in ids])
        _jpu, _jpv, jcu, jcv, P = cc.camera_rows(c, R, t, X)
        assert (P[:, 2] > 0).all()
        for p in range(6):
            d = np.zeros(6)
            d[p] = h
            plus, minus = cc.project_ext(cc.apply_ext(c, d), R, t, X), cc.project_ext(cc.apply_ext(c, -d), R, t, X)
            num = (plus - minus) / (2 * h)
            for col, ana in ((num[:, 0], jcu[:, p]), (num[:, 1], jcv[:, p])):
                worst = max(worst, np.abs(col - ana).max() / max(np.abs(jcu[:, p]).max(), np.abs(jcv[:, p]).max()))
    print("camera Jacobian: worst relative difference %.3g" % worst)
    assert worst <= 1e-6


# ---- the twin against the restatement ----------------------------------------------------------------
def check_against_restatement(rva, start, instants, **kw):
    cal, kept = cc.calibrator(rva, start, instants, **kw)
    got = cal.solve_host()
    ref = cc.solve_cal_ref(start, kept, **kw)
    assert cc.same_result(got, ref), (got, ref)
    assert cc.same_instants(cal.instants(), ref.instants)
    return cal, got, ref


def test_host_equals_the_restatement_2_cameras_3_instants(rva):
    rng = np.random.default_rng(766)
    _true, start, instants = cc.two_camera_case(rng, 3, noise_px=0.3)
    _cal, got, _ref = check_against_restatement(rva, start, instants)
    assert got.cov_valid and got.instants_used == 3 and got.accepted + got.rejected == cc.ITERS


def test_host_equals_the_restatement_3_cameras_33_instants(rva):
    """A partial second chunk; camera 2 is free_rot only and sees nothing in three instants."""
    true, start, instants = cc.three_camera_case(np.random.default_rng(767), 33)
    _cal, got, _ref = check_against_restatement(rva, start, instants, max_hamming=1)
    assert got.cov_valid and got.instants_used == 33
    assert not got.cov[0].any() and not got.cov[2][3:].any() and not got.cov[2][:, 3:].any() and got.cov[2][:3, :3].any()
    assert np.array_equal(got.t[2], start[2].Et)


# ---- exact corners ----------------------------------------------------------------------------------
def mount_error(got, true):
    return max(max(np.abs(R - c.ER).max(), np.abs(t - c.Et).max()) for R, t, c in zip(got.R, got.t, true))


def start_as_result(start):
    return SimpleNamespace(R=[c.ER for c in start], t=[c.Et for c in start])


def test_exact_corners_give_the_mounts_2_cameras(rva):
    rng = np.random.default_rng(971)
    true, start, instants = cc.two_camera_case(rng, 8)
    cal, _kept = cc.calibrator(rva, start, instants)
    got = cal.solve_host()
    print("2 cameras: mount error %.3g, rms %.3g -> %.3g" % (mount_error(got, true), got.rms_before, got.rms_after))
    assert mount_error(start_as_result(start), true) > 0.01
    assert mount_error(got, true) <= EXACT and got.rms_after < EXACT < got.rms_before


def test_exact_corners_give_the_mounts_8_cameras(rva):
    rng = np.random.default_rng(972)
    true, start, instants = cc.eight_camera_case(rng, 8)
    cal, _kept = cc.calibrator(rva, start, instants)
    got = cal.solve_host()
    print("8 cameras: mount error %.3g, rms %.3g -> %.3g" % (mount_error(got, true), got.rms_before, got.rms_after))
    assert mount_error(got, true) <= EXACT and got.rms_after < EXACT < got.rms_before
    assert np.array_equal(got.t[5], true[5].Et) and np.array_equal(got.R[6], true[6].ER)


def test_fixed_camera_keeps_its_mount_bit_for_bit(rva):
    rng = np.random.default_rng(973)
    _true, start, instants = cc.two_camera_case(rng, 5, noise_px=0.3)
    start[0] = cc.fixed(cc.perturbed(start[0], rng, 1.0, 0.01))   # (fixed somewhere that is not the truth)
    cal, _kept = cc.calibrator(rva, start, instants)
    got = cal.solve_host()
    assert got.accepted > 0
    assert got.R[0].tobytes() == np.ascontiguousarray(start[0].ER).tobytes()
    assert got.t[0].tobytes() == np.ascontiguousarray(start[0].Et).tobytes()
    assert not got.cov[0].any()


# ---- noise ------------------------------------------------------------------------------------------
def test_noise_rms_falls_and_covariance_matches_the_scatter(rva):
    """400 draws of 0.3 px corner noise on 2 cameras x 8 instants, fixed seed
    (test_rig_pose_host.py's test_covariance_matches_the_scatter: its repeats and its margin): for
    each of the six parameters of the free camera the empirical variance of the error (we from
    E_R_true^T E_R, camera frame; de in the robot frame) over the mean reported variance lies in
    [0.7, 1.4]; in every draw the after-RMS is below the before-RMS."""
    rng = np.random.default_rng(2026)
    true, start, _ = cc.two_camera_case(rng, 8)
    robots = cc.robot_poses(8, rng)
    cal = rva.RigCalibrator(cc.as_create_args(start), rc.RIG_LAYOUT)
    err, var = [], []
    for _ in range(400):
        cal.clear()
        for inst in cc.make_instants([0, 1], robots, rng, noise_px=0.3):
            assert cal.add(cc.as_add_args(inst))
        got = cal.solve_host()
        assert got.cov_valid and got.rms_after < got.rms_before
        dR = true[1].ER.T @ got.R[1]
        w = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
        err.append(np.concatenate([w, got.t[1] - true[1].Et]))
        var.append(np.diag(got.cov[1]))
    ratio = (np.array(err) ** 2).mean(0) / np.array(var).mean(0)
    print("variance ratios (we, de):", np.round(ratio, 3))
    assert (ratio >= 0.7).all() and (ratio <= 1.4).all()


# ---- degenerate cases -----------------------------------------------------------------------------------
def test_free_camera_that_never_shares_an_instant(rva):
    """Camera 2 is free and sees nothing in any stored instant: its block of the reduced matrix is
    zero, the factor fails, every step is rejected and nothing moves."""
    start, instants = cc.never_shared_case()
    _cal, got, _ref = check_against_restatement(rva, start, instants)
    assert not got.cov_valid and got.accepted == 0 and got.rejected == cc.ITERS
    assert not any(c.any() for c in got.cov) and got.rms_after == got.rms_before
    for R, t, c in zip(got.R, got.t, start):
        assert np.array_equal(R, c.ER) and np.array_equal(t, c.Et)


def test_an_instant_of_one_camera_is_not_stored(rva):
    rng = np.random.default_rng(32)
    _true, start, instants = cc.two_camera_case(rng, 2)
    cal = rva.RigCalibrator(cc.as_create_args(start), rc.RIG_LAYOUT)
    lone = rc.make_instant([0, None], rng)
    foreign = rc.make_instant([0, "foreign"], rng)
    assert not cc.stored(lone) and not cc.stored(foreign) and cc.stored(instants[0])
    assert cal.add(cc.as_add_args(lone)) is False and cal.add(cc.as_add_args(foreign)) is False and len(cal) == 0
    assert cal.add(cc.as_add_args(instants[0])) is True and cal.add([None, None]) is False and len(cal) == 1


# ---- accepted and rejected steps ------------------------------------------------------------------------
def test_both_accepted_and_rejected_steps(rva):
    start, instants = cc.accept_reject_case()
    _cal, got, _ref = check_against_restatement(rva, start, instants)
    print("accepted %d rejected %d" % (got.accepted, got.rejected))
    assert got.accepted > 0 and got.rejected > 0 and got.accepted + got.rejected == cc.ITERS


# ---- records and refusals ---------------------------------------------------------------------------------
def test_record_layouts(rva):
    from ros_vision_amd import detector as d
    assert C.sizeof(d.AtRigcalCamera) == 176 and C.sizeof(d.AtRigcalFrame) == 24
    assert C.sizeof(d.AtRigcalCameraResult) == 384 and C.sizeof(d.AtRigcalResult) == 40 + 8 * 384
    assert C.sizeof(d.AtRigcalInstant) == 112 and d.AtRigcalResult.cams.offset == 40
    assert d.AtRigcalInstant.rms_px.offset == 96 and d.AtRigcalCamera.free_rot.offset == 168


def test_refused_arguments(rva):
    rng = np.random.default_rng(5)
    _true, start, instants = cc.two_camera_case(rng, 1)

    def refused(cams, layout=rc.RIG_LAYOUT, **kw):
        with pytest.raises(rva.FieldPoseError) as e:
            rva.RigCalibrator(cc.as_create_args(cams), layout, **kw)
        return e.value.code == -1

    free = cc.true_camera(1)
    assert refused(start[:1]) and refused([start[0]] + [free] * 8)             # n_cams outside 2..8
    assert refused([free, free])                                               # no camera held fully fixed
    assert refused([start[0], cc.fixed(free)])                                 # no free parameter at all
    assert refused([cc.true_camera(0, free_trans=False), free])                # (half fixed is not fixed)
    assert refused(start, tag_size=0.0) and refused(start, max_hamming=-1)
    assert refused(start, []) and refused(start, rc.RIG_LAYOUT + [fc.wall_a(1024, 0, 0)])
    assert refused(start, rc.RIG_LAYOUT + [fc.wall_a(3, 1.0, 1.0)])            # an id twice
    skew = SimpleNamespace(cam=free.cam, ER=np.diag([1.0, 1.0, -1.0]), Et=free.Et, free_rot=True, free_trans=True)
    assert refused([start[0], skew])                                           # an R that is no rotation
    rva.RigCalibrator(cc.as_create_args([start[0]] + [free] * 7), rc.RIG_LAYOUT).close()   # 8 cameras: fine
    cal = rva.RigCalibrator(cc.as_create_args(start), rc.RIG_LAYOUT)
    with pytest.raises(rva.FieldPoseError) as e:                               # nothing stored
        cal.solve_host()
    assert e.value.code == -1
    with pytest.raises(ValueError):
        cal.add(cc.as_add_args(instants[0])[:1])


def test_the_4097th_instant_is_refused(rva):
    rng = np.random.default_rng(6)
    _true, start, instants = cc.two_camera_case(rng, 1)
    cal = rva.RigCalibrator(cc.as_create_args(start), rc.RIG_LAYOUT)
    arr, _keep = cal._frames(cc.as_add_args(instants[0]))
    L = rva.load_library()
    assert rva.AT_RIGCAL_MAX_INSTANTS == cc.MAX_INSTANTS == 4096
    for _ in range(4096):
        assert L.at_rigcal_add(cal._h, arr) == 1
    assert len(cal) == 4096 and L.at_rigcal_add(cal._h, arr) == -3             # AT_E_CAPACITY
    with pytest.raises(rva.FieldPoseError) as e:
        cal.add(cc.as_add_args(instants[0]))
    assert e.value.code == -3 and len(cal) == 4096
    cal.clear()
    assert len(cal) == 0 and cal.add(cc.as_add_args(instants[0])) is True


# ---- files -------------------------------------------------------------------------------------------
def test_save_extrinsics_round_trip(tmp_path):
    from ros_vision_amd import node
    path = tmp_path / "system_config.json"
    before = {"camera_mounted_positions": {"SER1": {"location": "front_left"}, "SER2": "rear"},
              "extrinsics": {"rear": {"rotation": [[1, 0, 0], [0, 1, 0], [0, 0, 1]], "offset": [0.1, 0.2, 0.3]}},
              "other": {"keep": [1, 2, 3]}}
    path.write_text(json.dumps(before))
    R, t = fc.rot_xyz(3.0, -20.0, 1.0), np.array([0.25, -0.125, 0.0625])
    node.save_extrinsics(str(path), "front_left", R, t)
    R2, t2, location = node.load_extrinsics(str(path), "SER1")
    assert location == "front_left" and np.array_equal(R2, R) and np.array_equal(t2, t)
    after = json.loads(path.read_text())
    assert after["other"] == before["other"] and after["camera_mounted_positions"] == before["camera_mounted_positions"]
    assert after["extrinsics"]["rear"] == before["extrinsics"]["rear"]
    R3, t3, _loc = node.load_extrinsics(str(path), "SER2")
    assert np.array_equal(R3, np.eye(3)) and np.array_equal(t3, [0.1, 0.2, 0.3])
    node.save_extrinsics(str(path), "rear", R, t)                              # an entry that exists is replaced
    assert np.array_equal(node.load_extrinsics(str(path), "SER2")[0], R)


# ---- the host side under sanitizers ----------------------------------------------------------------------
def test_sanitized_standalone_program(tmp_path):
    """tests/rig_calib_host_check.cpp + csrc/at_rigcal.cpp, at_rigpose.cpp, at_fieldpose.cpp built
    with the host compiler and -fsanitize=address,undefined (the runtimes linked statically), run
    as a child process: 3 cameras (one free_rot only), 35 instants from exact-size heap buffers
    (cameras that see nothing from NULL arrays, one instant refused), the host solve, the records,
    clear, the refused calls."""
    exe = tmp_path / "rig_calib_host_check"
    csrc = os.path.join(ROOT, "ros_vision_amd", "csrc")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-o", str(exe), os.path.join(ROOT, "tests", "rig_calib_host_check.cpp"),
                    os.path.join(csrc, "at_rigcal.cpp"), os.path.join(csrc, "at_rigpose.cpp"),
                    os.path.join(csrc, "at_fieldpose.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "34", "1", "6"]
