"""The field pose on the CPU (no GPU): at_field_pose_host against ground truth and against the
numpy restatement in tests/field_pose_cases.py, the selection rule, at_robot_in_field and the
layout checks.  at_field_pose_host shares its arithmetic with k_field (csrc/at_fieldpose.h),
so what holds here is what the device path is then held to in tests/test_field_pose_gpu.py."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import field_pose_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = 1e-9      # tests/test_pose.py's bound for exact data


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


# ---- exact projections ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.LAYOUTS))
def test_exact_projections_give_the_camera_pose(rva, name):
    """100 random cameras; every tag's own pose is 3 degrees and 3 cm off."""
    layout = fc.LAYOUTS[name]
    rng = np.random.default_rng(766)
    worst = np.zeros(3)
    for _ in range(100):
        R, t = fc.random_camera(rng)
        dets, poses = fc.make_frame(layout, R, t, rng)
        fp = rva.field_pose_host(dets, poses, layout)
        assert fp.n_tags == len(layout) and fp.ids == sorted(g[0] for g in layout)
        worst = np.maximum(worst, [np.abs(fp.R - R).max(), np.abs(fp.t - t).max(), fp.rms_px])
    print(name, "worst |dR| %.3g |dt| %.3g rms %.3g" % tuple(worst))
    assert worst[0] <= EXACT and worst[1] <= EXACT and worst[2] < EXACT


# ---- noisy corners ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.LAYOUTS))
def test_noisy_corners_agree_with_the_restatement(rva, name):
    layout = fc.LAYOUTS[name]
    rng = np.random.default_rng(971)
    for _ in range(25):
        R, t = fc.random_camera(rng)
        dets, poses = fc.make_frame(layout, R, t, rng, noise_px=0.3)
        fp = rva.field_pose_host(dets, poses, layout)
        ref = fc.solve_ref(dets, poses, layout)
        assert np.abs(fp.R @ fp.R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(fp.R) > 0
        assert fp.ids == ref.ids and fp.n_tags == ref.n_tags and fp.steps_taken == ref.steps_taken
        assert np.abs(fp.R - ref.R).max() <= EXACT and np.abs(fp.t - ref.t).max() <= EXACT
        assert abs(fp.rms_px - ref.rms_px) <= EXACT
        # the cost (independently evaluated) does not exceed the start's
        cost = fc.cost_of(dets, layout, fp.R, fp.t, fp.ids)
        assert cost <= ref.start_cost * (1 + 1e-12)
        assert abs(np.sqrt(cost / (4 * fp.n_tags)) - fp.rms_px) <= EXACT
        assert fp.steps_taken >= 1


def test_more_tags_help(rva):
    """The point of it: with 0.3 px of corner noise the camera position from three tags is
    closer to the truth (median over 60 cameras) than from one."""
    rng = np.random.default_rng(5)
    err = {"one": [], "two_walls": []}
    for _ in range(60):
        R, t = fc.random_camera(rng)
        for name in err:
            dets, poses = fc.make_frame(fc.LAYOUTS[name], R, t, rng, noise_px=0.3)
            fp = rva.field_pose_host(dets, poses, fc.LAYOUTS[name])
            err[name].append(np.linalg.norm(-fp.R.T @ fp.t + R.T @ t))
    assert np.median(err["two_walls"]) < 0.5 * np.median(err["one"])


# ---- the selection rule -----------------------------------------------------------------------
def _frame(layout, seed=3, **kw):
    rng = np.random.default_rng(seed)
    R, t = fc.random_camera(rng)
    dets, poses = fc.make_frame(layout, R, t, rng, **kw)
    return R, t, dets, poses


def _spoiled(d, p, **fields):
    """A copy of detection d whose corners are 25 px off (and its pose with it): if it were
    selected the result would be far from the truth."""
    bad = SimpleNamespace(**vars(d))
    bad.p = np.asarray(d.p) + 25.0
    for k, v in fields.items():
        setattr(bad, k, v)
    return bad, SimpleNamespace(**vars(p))


def test_duplicate_id_keeps_lower_hamming_then_greater_margin(rva):
    layout = fc.LAYOUT_COPLANAR
    R, t, dets, poses = _frame(layout)
    for fields in [{"hamming": 1}, {"decision_margin": 20.0},
                   {"hamming": 1, "decision_margin": 99.0}]:
        for front in (True, False):          # the order of the two does not matter
            bad, badp = _spoiled(dets[1], poses[1], **fields)
            d2 = [bad] + dets if front else dets + [bad]
            p2 = [badp] + poses if front else poses + [badp]
            fp = rva.field_pose_host(d2, p2, layout, max_hamming=2)
            ref = fc.solve_ref(d2, p2, layout, max_hamming=2)
            assert fp.ids == [1, 4, 7] == ref.ids and fp.steps_taken == ref.steps_taken
            assert np.abs(fp.R - R).max() <= EXACT and np.abs(fp.t - t).max() <= EXACT
    # equal hamming and margin: the lower slot
    bad, badp = _spoiled(dets[1], poses[1])
    fp = rva.field_pose_host(dets + [bad], poses + [badp], layout)
    assert np.abs(fp.t - t).max() <= EXACT
    fp = rva.field_pose_host([bad] + dets, [badp] + poses, layout)
    assert fp.rms_px > 1.0


def test_id_outside_the_layout_is_dropped(rva):
    layout = fc.LAYOUT_COPLANAR
    R, t, dets, poses = _frame(layout)
    bad, badp = _spoiled(dets[0], poses[0], id=586)
    badp.id = 586
    fp = rva.field_pose_host([bad] + dets, [badp] + poses, layout)
    assert fp.ids == [1, 4, 7] and np.abs(fp.t - t).max() <= EXACT
    # nothing of the layout in view: no pose, everything zero
    fp = rva.field_pose_host([bad], [badp], layout)
    assert fp.n_tags == 0 and fp.ids == [] and not fp.R.any() and not fp.t.any() and fp.rms_px == 0
    assert fp.steps_taken == 0
    fp = rva.field_pose_host([], [], layout)
    assert fp.n_tags == 0


def test_max_hamming_filters(rva):
    layout = fc.LAYOUT_COPLANAR
    R, t, dets, poses = _frame(layout)
    dets[2].hamming = 2
    assert rva.field_pose_host(dets, poses, layout, max_hamming=1).ids == [1, 4]
    assert rva.field_pose_host(dets, poses, layout, max_hamming=2).ids == [1, 4, 7]
    assert rva.field_pose_host(dets, poses, layout).ids == [1, 4]
    assert fc.solve_ref(dets, poses, layout, max_hamming=1).ids == [1, 4]


def test_seventeen_tags_keep_the_sixteen_lowest_ids(rva):
    ids = [40, 3, 17, 100, 250, 8, 9, 61, 62, 63, 500, 12, 77, 78, 300, 5, 2]
    layout = [fc.wall_a(tid, -1.2 + 0.3 * (k % 9), -0.2 + 0.4 * (k // 9)) for k, tid in enumerate(ids)]
    R, t, dets, poses = _frame(layout, seed=8)
    order = np.random.default_rng(0).permutation(len(dets))
    dets, poses = [dets[i] for i in order], [poses[i] for i in order]
    fp = rva.field_pose_host(dets, poses, layout)
    assert fp.n_tags == 16 and fp.ids == sorted(ids)[:16] and 500 not in fp.ids
    assert np.abs(fp.R - R).max() <= EXACT and np.abs(fp.t - t).max() <= EXACT
    ref = fc.solve_ref(dets, poses, layout)
    assert ref.ids == fp.ids and ref.steps_taken == fp.steps_taken


def test_candidate_behind_the_camera_is_never_the_start(rva):
    """Tag 2's pose is the exact one mirrored through the camera centre (-R, -t): it reprojects
    every corner exactly, so it would win the start on cost alone -- and leave the solve at a
    reflection.  Every Z is negative under it, so it does not count."""
    layout = fc.LAYOUT_TWO_WALLS
    rng = np.random.default_rng(12)
    R, t = fc.random_camera(rng)
    dets, poses = fc.make_frame(layout, R, t, rng)
    exact = fc.make_frame(layout, R, t, rng, pose_rot_deg=0.0, pose_t_m=0.0)[1][0]
    poses[0] = SimpleNamespace(id=exact.id, R=-exact.R, t=-exact.t, err=0.0)
    Rm, tm = -exact.R @ layout[0][1].T, None
    tm = -exact.t - Rm @ layout[0][2]
    assert fc.cost_of(dets, layout, Rm, tm, [2, 5, 9]) < 1e-18       # the mirrored start would have cost 0
    fp = rva.field_pose_host(dets, poses, layout)
    ref = fc.solve_ref(dets, poses, layout)
    assert ref.start_cost > 1.0                                       # ... a perturbed one was taken
    assert np.linalg.det(fp.R) > 0 and np.abs(fp.R - R).max() <= EXACT and np.abs(fp.t - t).max() <= EXACT
    assert fp.steps_taken == ref.steps_taken
    # every pose mirrored: no start at all
    for p in poses[1:]:
        p.R, p.t = -np.asarray(p.R), -np.asarray(p.t)
    assert rva.field_pose_host(dets, poses, layout).n_tags == 0


# ---- at_robot_in_field ------------------------------------------------------------------------
def _fp(rva, R, t):
    return rva.FieldPose(n_tags=1, ids=[3], R=R, t=t, rms_px=0.0, steps_taken=1)


def test_robot_in_field(rva):
    R, t = fc.camera_pose((0.4, -0.2, -3.0), 5.0, -20.0, 3.0)
    cam_in_field = -R.T @ t
    # identity extrinsics: the camera's own pose in the field
    Rr, tr = rva.robot_in_field(_fp(rva, R, t))
    assert np.abs(Rr - R.T).max() <= 1e-15 and np.abs(tr - cam_in_field).max() <= 1e-15
    # a pure offset: the camera sits at `off` in the robot frame
    off = np.array([0.3, -0.1, 0.5])
    Rr, tr = rva.robot_in_field(_fp(rva, R, t), None, off)
    assert np.abs(Rr - R.T).max() <= 1e-15 and np.abs(tr + Rr @ off - cam_in_field).max() <= 1e-14
    # a 90 degree mount: camera z (forward) is robot x, camera x is robot -y, camera y is robot -z
    mount = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])
    Rr, tr = rva.robot_in_field(_fp(rva, R, t), mount, off)
    assert np.abs(Rr @ mount - R.T).max() <= 1e-15
    assert np.abs(Rr @ off + tr - cam_in_field).max() <= 1e-14        # the camera's place, through the robot
    with pytest.raises(rva.FieldPoseError):
        rva.robot_in_field(rva.FieldPose(0, [], np.zeros((3, 3)), np.zeros(3), 0.0, 0))


def test_robot_in_field_round_trip_with_tag_detections(rva):
    """A tag's position in the robot frame (at_tag_detections) carried into the field by the
    robot's field pose is where the layout says the tag is."""
    layout = fc.LAYOUT_TWO_WALLS
    R, t = fc.camera_pose((0.2, 0.1, -2.5), -6.0, 12.0, 4.0)
    rng = np.random.default_rng(1)
    dets, poses = fc.make_frame(layout, R, t, rng, pose_rot_deg=0.0, pose_t_m=0.0)
    mount, off = fc.rot_xyz(10.0, 80.0, -5.0), np.array([0.25, 0.0, 0.6])
    fp = rva.field_pose_host(dets, poses, layout)
    Rr, tr = rva.robot_in_field(fp, mount, off)
    where = {g[0]: g[2] for g in layout}
    for tag in rva.tag_detections([rva.Pose(p.id, p.R, p.t, 0.0) for p in poses], mount, off):
        assert np.abs(Rr @ tag.robot + tr - where[tag.id]).max() <= 1e-9


# ---- layout validation ------------------------------------------------------------------------
def test_layout_validation(rva):
    layout = fc.LAYOUT_COPLANAR
    _R, _t, dets, poses = _frame(layout)

    def refused(tags, **kw):
        with pytest.raises(rva.FieldPoseError) as e:
            rva.field_pose_host(dets, poses, tags, **kw)
        return e.value.code == -1

    assert refused(layout, tag_size=0.0)
    assert refused(layout, max_hamming=-1)
    assert refused(layout + [fc.wall_a(1024, 0, 0)])                 # ids are [0, 1024)
    assert refused(layout + [fc.wall_a(-1, 0, 0)])
    assert refused(layout + [fc.wall_a(4, 1.0, 1.0)])                # an id twice
    skew = np.eye(3)
    skew[0, 1] = 3e-6
    assert refused(layout + [(9, skew, np.zeros(3))])                # |R R^T - I| > 1e-6
    assert refused(layout + [(9, 1.00001 * np.eye(3), np.zeros(3))])
    assert refused(layout + [(9, np.diag([1.0, 1.0, -1.0]), np.zeros(3))])   # det < 0
    near = np.eye(3)
    near[0, 1] = 5e-7
    assert rva.field_pose_host(dets, poses, layout + [(9, near, np.zeros(3))]).n_tags == 3   # within 1e-6
    assert rva.field_pose_host(dets, poses, []).n_tags == 0          # an empty layout: nothing to use


def test_record_layout(rva):
    from ros_vision_amd.detector import AtFieldPose, AtFieldTag
    assert C.sizeof(AtFieldTag) == 104 and C.sizeof(AtFieldPose) == 184
    assert AtFieldPose.R.offset == 72 and AtFieldPose.steps_taken.offset == 176


# ---- the twin under sanitizers ------------------------------------------------------------------
def test_sanitized_standalone_program(tmp_path):
    """tests/field_pose_host_check.cpp + csrc/at_fieldpose.cpp built with the host compiler and
    -fsanitize=address,undefined (the runtimes linked statically), run as a child process: exact
    scenes of 1, 3 and 17 tags from exact-size heap buffers, 200 candidates in one frame, the
    refused layouts."""
    exe = tmp_path / "field_pose_host_check"
    csrc = os.path.join(ROOT, "ros_vision_amd", "csrc")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-o", str(exe), os.path.join(ROOT, "tests", "field_pose_host_check.cpp"),
                    os.path.join(csrc, "at_fieldpose.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "4", "8"]
