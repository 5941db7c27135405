"""The robust rig pose on the CPU (no GPU): at_rig_pose_robust_host against the numpy restatement in
tests/rig_robust_cases.py bit for bit, against the plain solve at infinite thresholds, on scenes
with displaced layout tags and moved corners, at its limits (starvation, the round cap, the 17th
tag), its covariance against the scatter of 400 noisy solves, and the refused calls.  The twin
shares its arithmetic with k_rig_robust (csrc/at_rigrobust.h), so what holds here is what the
device path is then held to in tests/test_rig_robust_gpu.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import field_pose_cases as fc
import rig_pose_cases as rc
import rig_robust_cases as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def robust(rva, cams, layout=rc.RIG_LAYOUT, cfg=rr.DEFAULT, raw=False, **kw):
    return rva.rig_pose_robust_host(rc.as_host_args(cams), layout, cfg, raw=raw, **kw)


def plain(rva, cams, layout=rc.RIG_LAYOUT, **kw):
    return rva.rig_pose_host(rc.as_host_args(cams), layout, **kw)


def plain_bytes(rva, cams, layout=rc.RIG_LAYOUT):
    """at_rig_pose_host's record as bytes."""
    from ros_vision_amd import detector as D
    arr, n, _keep = D._rig_host_cams(rc.as_host_args(cams))
    tarr, nt = D._field_tags(layout)
    out = D.AtRigPose()
    assert D.load_library().at_rig_pose_host(arr, n, tarr, nt, 0, rc.TAG_SIZE, C.byref(out)) == 0
    return bytes(out)


def move_corner(cam, det, corner, by):
    p = np.array(cam.dets[det].p, np.float64)
    p[corner] += by
    cam.dets[det].p = p


def cap_scene():
    """Four cameras, 0.3 px noise, five layout tags moved by up to 0.3 m each (a fixed draw): with
    min_keep = 1 every one of three rounds drops tags, and a tag beyond reject_px is still left."""
    rng = np.random.default_rng(5088)
    cams = rc.make_instant([0, 1, 2, 3], rng, noise_px=0.3)
    n = rng.integers(2, 6)
    ids = set(int(x) for x in rng.choice(8, size=n, replace=False))
    sh = {tid: rng.uniform(-1, 1, 3) * rng.choice([0.02, 0.05, 0.1, 0.2, 0.3]) for tid in ids}
    layout = [(tid, R, np.asarray(t, np.float64) + (sh[tid] if tid in ids else 0.0)) for tid, R, t in rc.RIG_LAYOUT]
    return cams, layout


def many_tags_scene(rng, bad=5):
    """One camera in front of 17 layout tags on wall A (ids 0..16, a 6 x 3 grid), tag `bad` of the
    layout displaced: the 17th id is beyond the per-camera cap."""
    layout = [fc.wall_a(i, -0.75 + 0.3 * (i % 6), -0.3 + 0.3 * (i // 6)) for i in range(17)]
    _ids, ER, Et, cam = rc.mount(0)
    Rc, tc = rc.camera_in_field(*rc.ROBOT, ER, Et)
    dets, poses = fc.make_frame(layout, Rc, tc, rng, cam=cam, noise_px=0.3)
    return [rc.rig_camera(dets, poses, cam, ER, Et)], rr.displaced(layout, {bad}), layout


# ---- the twin against the restatement -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.SCENES))
def test_host_equals_the_restatement_on_displaced_tags(rva, name):
    mounts, bad = rr.SCENES[name]
    rng = np.random.default_rng(31)
    layout = rr.displaced(rc.RIG_LAYOUT, bad)
    for _ in range(3):
        cams = rc.make_instant(mounts, rng, noise_px=0.3)
        got, info = robust(rva, cams, layout)
        ref, rinfo = rr.solve_robust_ref(cams, layout)
        assert rc.same_record(got, ref) and rr.same_info(info, rinfo), name
        assert info.n_rejected >= 1 and info.rounds >= 1 and got.dropped == 0


def test_host_equals_the_restatement_on_the_other_scenes(rva):
    """Clean and empty instants, 8 cameras with blank and foreign-only members, a moved corner
    (dropped / down-weighted), starvation, max_rounds 0, the round cap, 17 tags, infinite
    thresholds, a Huber threshold below the noise."""
    rng = np.random.default_rng(32)
    two = [g for g in rc.RIG_LAYOUT if g[0] in (0, 1)]
    eight = [0, None, 1, "foreign", 2, None, 3, None]
    far = rc.make_instant([0, 1, 2], rng, noise_px=0.3)
    move_corner(far[1], 1, 2, (15.0, -9.0))
    near = rc.make_instant([0, 1, 2], rng, noise_px=0.3)
    move_corner(near[1], 1, 2, (4.0, 0.0))
    many, many_layout, _true = many_tags_scene(rng)
    cases = [
        (rc.make_instant([0, 1, 2], rng, noise_px=0.3), rc.RIG_LAYOUT, rr.DEFAULT),
        (rc.make_instant([0, 1], rng), rc.RIG_LAYOUT, rr.DEFAULT),
        (rc.make_instant([None, "foreign"], rng), rc.RIG_LAYOUT, rr.DEFAULT),
        (rc.make_instant(eight, rng, noise_px=0.3), rr.displaced(rc.RIG_LAYOUT, {4}), rr.DEFAULT),
        (far, rc.RIG_LAYOUT, rr.DEFAULT),
        (near, rc.RIG_LAYOUT, rr.DEFAULT),
        (rc.make_instant([0], rng, noise_px=0.3), rr.displaced(two, {1}), rr.DEFAULT),
        (rc.make_instant([0, 1, 2], rng, noise_px=0.3), rr.displaced(rc.RIG_LAYOUT, {4}), rr.cfg(max_rounds=0)),
        (*cap_scene(), rr.cfg(min_keep=1)),
        (many, many_layout, rr.DEFAULT),
        (rc.make_instant([0, 1, 2], rng, noise_px=0.3), rr.displaced(rc.RIG_LAYOUT, {4}), rr.PLAIN),
        (rc.make_instant([0, 1, 2], rng, noise_px=0.3), rc.RIG_LAYOUT, rr.cfg(huber_px=0.25, reject_px=0.6)),
    ]
    for k, (cams, layout, cfg) in enumerate(cases):
        got, info = robust(rva, cams, layout, cfg)
        ref, rinfo = rr.solve_robust_ref(cams, layout, cfg)
        assert rc.same_record(got, ref), k
        assert rr.same_info(info, rinfo), k


# ---- infinite thresholds: the plain solve ---------------------------------------------------------
def test_infinite_thresholds_give_the_plain_record(rva):
    rng = np.random.default_rng(33)
    for seed in range(50):
        mounts = [[0, 1, 2], [0], [1, None, 2], [0, 1, 2, 3], [3, "foreign"]][seed % 5]
        layout = rr.displaced(rc.RIG_LAYOUT, {4}) if seed % 2 else rc.RIG_LAYOUT
        cams = rc.make_instant(mounts, rng, noise_px=(0.0, 0.3, 1.0)[seed % 3])
        got, info, rec, _raw = robust(rva, cams, layout, rr.PLAIN, raw=True)
        assert rec == plain_bytes(rva, cams, layout), seed
        assert info.n_rejected == 0 and info.rounds == 0 and not info.starved and info.n_downweighted == 0
        assert info.n_kept == got.n_tags and not any(info.rejected_mask)


# ---- displaced layout tags -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.SCENES))
def test_displaced_tags_are_dropped(rva, name):
    """20 seeds per scene, 0.3 px noise, the scene's layout tags displaced by (0.25, 0.10, 0) m:
    exactly the displaced tags' views are dropped, and the pose is within 1e-6 m and 1e-6 in R of
    the plain solve on the layout without those tags -- both are converged minima of one cost, and
    the margin over the prototype's 1.2e-9 is for LM convergence differences.
    Measured worst per scene (|dt| m, |dR|): tag0_3cams 6.7e-10, 4.8e-10; tag1_1cam 4.2e-9,
    3.1e-9; tag4_2cams 1.4e-9, 1.0e-9; tag4_3cams 1.5e-9, 1.1e-9; tags14_4cams 7.8e-10, 5.6e-10;
    tags46_3cams 1.7e-9, 1.3e-9."""
    mounts, bad = rr.SCENES[name]
    rng = np.random.default_rng(34)
    layout = rr.displaced(rc.RIG_LAYOUT, bad)
    worst = np.zeros(2)
    for seed in range(20):
        cams = rc.make_instant(mounts, rng, noise_px=0.3)
        got, info = robust(rva, cams, layout)
        assert rr.dropped_views(info, got) == rr.bad_views(mounts, bad), (name, seed)
        assert info.n_rejected == len(rr.bad_views(mounts, bad)) and info.n_kept == got.n_tags - info.n_rejected
        assert not info.starved and got.cov_valid
        want = plain(rva, cams, rr.without(rc.RIG_LAYOUT, bad))
        worst = np.maximum(worst, [np.abs(got.t - want.t).max(), np.abs(got.R - want.R).max()])
    print(name, "worst |dt| %.3g m, |dR| %.3g" % tuple(worst))
    assert worst[0] <= 1e-6 and worst[1] <= 1e-6


def test_the_plain_solve_is_poisoned_where_the_robust_one_is_not(rva):
    """What the feature is for, on tag4_3cams: the plain solve is more than 0.1 m from the solve
    with the true layout (183 to 434 mm over 20 seeds), the robust one within 5 mm of it -- the two
    differ by the nine other views' weight of tag 4's own 0.3 px noise."""
    rng = np.random.default_rng(34)
    cams = rc.make_instant([0, 1, 2], rng, noise_px=0.3)
    layout = rr.displaced(rc.RIG_LAYOUT, {4})
    clean = plain(rva, cams)
    assert np.linalg.norm(plain(rva, cams, layout).t - clean.t) > 0.1
    assert np.linalg.norm(robust(rva, cams, layout)[0].t - clean.t) < 0.005


# ---- moved corners ---------------------------------------------------------------------------------
def test_a_corner_moved_far_drops_its_tag(rva):
    rng = np.random.default_rng(35)
    for _ in range(10):
        cams = rc.make_instant([0, 1, 2], rng, noise_px=0.3)
        move_corner(cams[1], 1, 2, (15.0, -9.0))           # camera 1's second tag: id 3
        got, info = robust(rva, cams)
        assert rr.dropped_views(info, got) == [(1, 3)] and info.rounds == 1


def test_a_corner_moved_a_little_is_downweighted(rva):
    """4 px is beyond huber_px and far below a tag RMS of reject_px: the corner is down-weighted,
    nothing is dropped, and the robot's position is nearer the clean solve's than the plain solve's
    is (the issue's measure, distance).  The rotation is not asserted: the Huber weight shrinks the
    outlier's pull on the whole pose, not on each parameter, and in one of these ten draws the
    largest entry of R - R_clean is 9.1e-5 against the plain solve's 8.4e-5."""
    rng = np.random.default_rng(36)
    for _ in range(10):
        cams = rc.make_instant([0, 1, 2], rng, noise_px=0.3)
        clean = plain(rva, cams)
        move_corner(cams[1], 1, 2, (4.0, 0.0))
        off = plain(rva, cams)
        got, info = robust(rva, cams)
        assert info.n_rejected == 0 and info.rounds == 0 and info.n_downweighted >= 1
        assert np.linalg.norm(got.t - clean.t) < np.linalg.norm(off.t - clean.t)


# ---- clean scenes -----------------------------------------------------------------------------------
def test_clean_scenes_lose_nothing(rva):
    """200 seeds of three cameras at 0.3 px noise: no tag is dropped in any, and where no corner
    lies beyond huber_px at the end the record is the plain one byte for byte -- which must be so
    in at least 190 (measured: all 200).
    Byte equality needs every weight to be 1.0 on the whole path, not only at the end, so these
    scenes give each tag its true pose for the start: the start's corners are then 0.3 px noise
    away, inside huber_px.  With make_instant's default start (every tag's pose 3 degrees and 3 cm
    off, corners tens of pixels away) the first iterations run with weights below 1, the LM path
    differs and ends 1e-9 beside the plain one: byte equality in 0 of 200 seeds, while all 200
    have n_downweighted == 0.  That case is test_clean_scenes_from_a_far_start."""
    rng = np.random.default_rng(37)
    equal = 0
    for seed in range(200):
        cams = rc.make_instant([0, 1, 2], rng, noise_px=0.3, pose_rot_deg=0.0, pose_t_m=0.0)
        _got, info, rec, _raw = robust(rva, cams, raw=True)
        assert info.n_rejected == 0 and info.rounds == 0 and not info.starved, seed
        if info.n_downweighted == 0:
            assert rec == plain_bytes(rva, cams), seed
            equal += 1
    print("clean scenes equal to the plain record: %d of 200" % equal)
    assert equal >= 190


def test_clean_scenes_from_a_far_start(rva):
    """The same 200 seeds with make_instant's default start, 3 degrees and 3 cm off: no tag is
    dropped, no corner ends beyond huber_px in at least 190, and there the pose is within 1e-6 m
    and 1e-6 in R of the plain one -- two converged minima of one cost (the Huber cost is the plain
    cost wherever every corner is inside huber_px), the bound of test_displaced_tags_are_dropped.
    Measured: all 200, worst 1.6e-9."""
    rng = np.random.default_rng(37)
    near, worst = 0, 0.0
    for seed in range(200):
        cams = rc.make_instant([0, 1, 2], rng, noise_px=0.3)
        got, info = robust(rva, cams)
        assert info.n_rejected == 0 and info.rounds == 0 and not info.starved, seed
        if info.n_downweighted == 0:
            want = plain(rva, cams)
            worst = max(worst, np.abs(got.t - want.t).max(), np.abs(got.R - want.R).max())
            near += 1
    print("clean scenes, far start: %d of 200 without a down-weighted corner, worst %.3g" % (near, worst))
    assert near >= 190 and worst <= 1e-6


# ---- the limits of the rounds -------------------------------------------------------------------------
def test_starvation_keeps_the_huber_fit(rva):
    rng = np.random.default_rng(38)
    layout = rr.displaced([g for g in rc.RIG_LAYOUT if g[0] in (0, 1)], {1})
    cams = rc.make_instant([0], rng, noise_px=0.3)
    got, info, rec, _raw = robust(rva, cams, layout, raw=True)
    assert info.starved and info.n_rejected == 0 and info.rounds == 0 and info.n_kept == 2 == got.n_tags
    assert not any(info.rejected_mask) and max(info.tag_rms_px[0]) > rr.DEFAULT.reject_px
    fit, finfo, frec, _ = robust(rva, cams, layout, rr.cfg(max_rounds=0), raw=True)
    assert rec == frec and not finfo.starved                 # the record is the Huber fit's


def test_max_rounds_zero_drops_nothing(rva):
    rng = np.random.default_rng(39)
    cams = rc.make_instant([0, 1, 2], rng, noise_px=0.3)
    layout = rr.displaced(rc.RIG_LAYOUT, {4})
    got, info = robust(rva, cams, layout, rr.cfg(max_rounds=0))
    assert info.n_rejected == 0 and info.rounds == 0 and not info.starved and info.n_kept == got.n_tags == 10
    assert info.tag_rms_px[1][2] > rr.DEFAULT.reject_px and info.n_downweighted >= 1
    assert got.steps_taken + got.rejected == rc.ITERS
    one, oinfo = robust(rva, cams, layout, rr.cfg(max_rounds=1))
    assert oinfo.rounds == 1 and one.steps_taken + one.rejected == 2 * rc.ITERS


def test_rounds_stop_at_the_cap(rva):
    """cap_scene: rounds 1, 2 and 3 each drop tags, and after the third a kept tag is still beyond
    reject_px -- a fourth round would find a candidate, and is not run."""
    cams, layout = cap_scene()
    seen = []
    for rounds in (1, 2, 3):
        got, info = robust(rva, cams, layout, rr.cfg(max_rounds=rounds, min_keep=1))
        assert info.rounds == rounds and got.steps_taken + got.rejected == (rounds + 1) * rc.ITERS
        seen.append(info.n_rejected)
    assert seen[0] < seen[1] < seen[2]
    kept = [v for c in range(8) for j, v in enumerate(info.tag_rms_px[c]) if not info.rejected_mask[c] >> j & 1]
    assert len(kept) == info.n_kept and max(kept) > rr.DEFAULT.reject_px


def test_the_seventeenth_tag(rva):
    rng = np.random.default_rng(40)
    cams, layout, true_layout = many_tags_scene(rng)
    got, info = robust(rva, cams, layout)
    assert got.n_tags == 16 and got.dropped == 1 and got.ids[0] == list(range(16))
    assert rr.dropped_views(info, got) == [(0, 5)] and info.n_kept == 15 and len(info.tag_rms_px[0]) == 16
    want = plain(rva, cams, rr.without(true_layout, {5, 16}))
    assert np.abs(got.t - want.t).max() <= 1e-6 and np.abs(got.R - want.R).max() <= 1e-6


# ---- the covariance -----------------------------------------------------------------------------------
def test_covariance_matches_the_scatter(rva):
    """tests/test_rig_pose_host.py's check and band, on two cameras whose layout has tag 4
    displaced: 400 draws of 0.3 px noise, every one drops that view, and for each of the six
    parameters the empirical variance of the error over the mean reported variance lies in
    [0.7, 1.4]."""
    rng = np.random.default_rng(2026)
    Rr, tr = rc.ROBOT
    layout = rr.displaced(rc.RIG_LAYOUT, {4})
    err, var = [], []
    for _ in range(400):
        got, info = robust(rva, rc.make_instant([0, 1], rng, noise_px=0.3), layout)
        assert got.cov_valid and rr.dropped_views(info, got) == [(1, 4)]
        dR = Rr.T @ got.R
        w = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
        err.append(np.concatenate([w, got.t - tr]))
        var.append(np.diag(got.cov))
    ratio = (np.array(err) ** 2).mean(0) / np.array(var).mean(0)
    print("variance ratios (w, t):", np.round(ratio, 3))
    assert (ratio >= 0.7).all() and (ratio <= 1.4).all()


# ---- records and refusals ---------------------------------------------------------------------------
def test_record_layout(rva):
    from ros_vision_amd import detector as D
    assert C.sizeof(D.AtRigRobustConfig) == 24 and C.sizeof(D.AtRigRobustInfo) == 1088
    assert D.AtRigRobustInfo.rejected_mask.offset == 16 and D.AtRigRobustInfo.tag_rms_px.offset == 48
    assert D.AtRigRobustInfo.huber_cost.offset == 1072 and D.AtRigRobustInfo.n_downweighted.offset == 1080
    assert C.sizeof(D.AtRigPose) == 960                         # at_rig_pose is unchanged
    assert rva.load_library().at_abi_version() == 8
    for name in ("at_rig_solve_robust", "at_rig_pose_robust_host", "at_rig_robust_stats"):
        assert name in D.EXPORTS and hasattr(rva.load_library(), name)
    d = rva.RigRobust()
    assert (d.huber_px, d.reject_px, d.max_rounds, d.min_keep) == (2.0, 6.0, 3, 2)


def test_refused_arguments(rva):
    rng = np.random.default_rng(41)
    cams = rc.make_instant([0, 1], rng)

    def refused(cams=cams, layout=rc.RIG_LAYOUT, cfg=rr.DEFAULT, **kw):
        with pytest.raises(rva.FieldPoseError) as e:
            robust(rva, cams, layout, cfg, **kw)
        return e.value.code == -1

    assert refused(cfg=None)                                              # a NULL config
    for bad in (0.0, -1.0, math.nan, -math.inf):
        assert refused(cfg=rr.cfg(huber_px=bad)) and refused(cfg=rr.cfg(reject_px=bad))
    assert refused(cfg=rr.cfg(max_rounds=-1)) and refused(cfg=rr.cfg(max_rounds=4))
    assert refused(cfg=rr.cfg(min_keep=0)) and refused(cfg=rr.cfg(min_keep=-3))
    # what at_rig_pose_host refuses
    assert refused([]) and refused(cams * 5)
    assert refused(tag_size=0.0) and refused(max_hamming=-1)
    assert refused(layout=[]) and refused(layout=rc.RIG_LAYOUT + [fc.wall_a(1024, 0, 0)])
    assert refused(layout=rc.RIG_LAYOUT + [fc.wall_a(3, 1.0, 1.0)])
    skew = rc.rig_camera(cams[0].dets, cams[0].poses, cams[0].cam, np.diag([1.0, 1.0, -1.0]), np.zeros(3))
    assert refused([skew, cams[1]])
    # the edges that are fine
    for ok in (rr.cfg(huber_px=math.inf), rr.cfg(reject_px=math.inf), rr.cfg(max_rounds=0), rr.cfg(max_rounds=3),
               rr.cfg(min_keep=1), rr.cfg(huber_px=1e-3)):
        assert robust(rva, cams, cfg=ok)[0].n_tags == 6
    assert robust(rva, cams * 4)[0].n_tags == 24


# ---- the twin under sanitizers ------------------------------------------------------------------
def test_sanitized_standalone_program(tmp_path):
    """tests/rig_robust_host_check.cpp + csrc/at_rigpose.cpp + csrc/at_fieldpose.cpp built with the
    host compiler and -fsanitize=address,undefined (the runtimes linked statically), run as a child
    process, from exact-size heap buffers: a camera that sees nothing, a camera emptied by the
    rejection, 8 cameras of 16 tags, starvation; the refused calls."""
    exe = tmp_path / "rig_robust_host_check"
    csrc = os.path.join(ROOT, "ros_vision_amd", "csrc")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-o", str(exe), os.path.join(ROOT, "tests", "rig_robust_host_check.cpp"),
                    os.path.join(csrc, "at_rigpose.cpp"), os.path.join(csrc, "at_fieldpose.cpp")],
                   check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "4", "9"]
