"""Ideal corners on the GPU: the head of the pose stage (k_pose<false>, k_pose<true>, the pose wave
of k_decode<true>) and k_und_points against their CPU twins, bit for bit; the poses, the field pose
and the rig pose that follow from them; what stays raw; the mode's lifecycle; the end-to-end gain.

Frames: 640 x 480 GRAY8.  The scenes of tests/field_pose_cases.py are drawn without distortion and
then seen through GPU_LENS by undistort_cases.warp (an inverse-map remap with the restatement); the
detector is created with that lens.  The CPU oracle decodes every intended tag of every warped scene."""
import json
import os
import subprocess

import numpy as np
import pytest

import field_pose_cases as fc
import tag_scenes as ts
import undistort_cases as uc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(ROOT, "node")
W, H = 640, 480
POSE_TOL = 1e-4        # parity_util's tolerance for a device pose against the oracle's
NAMES = list(fc.GPU_SCENES)


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


@pytest.fixture(scope="module")
def flat():
    """name -> (gray without distortion, (R, t) of the camera, ids drawn)."""
    codes = ts.codes()
    out = {name: fc.render_scene(name, ts.draw_tag, codes, ts.blank) for name in NAMES}
    out["crowd"] = (uc.crowd_frame(ts.draw_tag, ts.square, codes, ts.blank), None, tuple(range(20, 38)))
    return out


@pytest.fixture(scope="module")
def scenes(flat):
    """name -> the scene seen through GPU_LENS."""
    return {name: uc.warp(flat[name][0], uc.GPU_LENS) for name in flat}


def make(rva, ln, max_batch, undistort=True, layout=True):
    cam, dist = uc.camera_of(rva, ln)
    d = rva.GpuDetector(W, H, cam, dist, max_batch=max_batch)
    if layout:
        d.set_field_layout(fc.GPU_LAYOUT)
    if undistort:
        d.set_undistort(True)
    return d


@pytest.fixture(scope="module")
def lat(rva):
    d = make(rva, uc.GPU_LENS, 1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def thr(rva):
    d = make(rva, uc.GPU_LENS, 16)
    yield d
    d.close()


@pytest.fixture(scope="module")
def lat_plain(rva):
    d = make(rva, uc.GPU_LENS, 1, undistort=False)
    yield d
    d.close()


@pytest.fixture(scope="module")
def thr_plain(rva):
    d = make(rva, uc.GPU_LENS, 16, undistort=False)
    yield d
    d.close()


def same_field(a, b):
    return (a.n_tags == b.n_tags and a.ids == b.ids and a.steps_taken == b.steps_taken and a.rms_px == b.rms_px
            and np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t))


def same_pose(a, b):
    return a.id == b.id and np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and (a.err == b.err)


def check_frame(rva, oracle_mod, det, plain, f, ln, want_ids):
    """Frame f of det's last batch (mode on) against the twins, the oracle's pose and `plain`'s
    frame f (the same frame through a detector without the mode).  Returns the ideal detections."""
    cam, dist = uc.camera_of(rva, ln)
    raw, ideal, poses = det.detections(f), det.ideal_detections(f), det.poses(f)
    assert [d.id for d in raw] == sorted(want_ids)
    twin = rva.ideal_detections_host(raw, cam, dist)
    assert len(ideal) == len(raw) == len(poses)
    for a, b in zip(ideal, twin):
        assert uc.same_detection(a, b), (f, a, b)
    for a, r in zip(ideal, raw):
        assert uc.same_detection(a, uc.ideal_detection_ref(ln, r))                      # ... and the restatement
    # the pose is the oracle's estimate on the ideal H and corners
    for d, p in zip(ideal, poses):
        assert d.id == p.id
        Re, te, _err, (e1, e2), _second = oracle_mod.estimate_tag_pose(d.H, d.p, ln.fx, ln.fy, ln.cx, ln.cy, fc.TAG_SIZE)
        if abs(e1 - e2) <= 1e-9 * max(e1, e2, 1e-30):
            continue
        assert np.abs(p.R - Re).max() <= POSE_TOL and np.abs(p.t - te).max() <= POSE_TOL, (f, d.id)
    # what stays raw
    assert det.frame_record_bytes(f) == plain.frame_record_bytes(f)
    # the field pose read the ideal records
    host = rva.field_pose_host(ideal, poses, fc.GPU_LAYOUT, camera_matrix=cam)
    assert same_field(det.field_poses()[f], host), f
    return ideal


# ---- the points kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_points_kernel_equals_the_twin(rva, n):
    ln = uc.load_lenses()["cam14"]
    cam, dist = uc.camera_of(rva, ln)
    det = rva.GpuDetector(W, H, cam, dist, max_batch=1)
    try:
        rng = np.random.default_rng(n)
        xy = rng.uniform(0.1, 0.9, (n, 2)) * [1280.0, 800.0]
        special = np.array([[0.0, 0.0], [np.nan, 7.0], [1279.0, 0.0], [40.0, 40.0], [np.inf, 1.0]])[:n]
        xy[n - len(special):] = special                               # cam14's flagged pixels, a NaN, an infinity: last
        got, ok = det.undistort_points(xy)
        want, wok = rva.undistort_points_host(xy, cam, dist)
        assert np.array_equal(ok, wok) and got.tobytes() == want.tobytes()
        assert not ok[n - len(special):].any() and ok[:n - len(special)].all()
    finally:
        det.close()


# ---- the four paths ------------------------------------------------------------------------------
def test_latency_detector_pose_wave(rva, oracle_mod, scenes, lat, lat_plain):
    """B = 1, nothing timed: the pose-fused k_decode<true>, both of its waves."""
    for name in NAMES:
        lat.detect(scenes[name], rva.AT_FMT_GRAY8)
        lat_plain.detect(scenes[name], rva.AT_FMT_GRAY8)
        ideal = check_frame(rva, oracle_mod, lat, lat_plain, 0, uc.GPU_LENS, fc.GPU_SCENES[name][0])
        st = lat.undistort_stats()
        assert st == {"ideal": len(ideal), "not_invertible": 0}
        if ideal:
            raw = lat.detections(0)
            assert max(np.abs(a.p - r.p).max() for a, r in zip(ideal, raw)) > 0.1      # the lens moved the corners (0.38 px for the tag at the centre)
    assert lat_plain.undistort_stats() == {"ideal": 0, "not_invertible": 0}


def test_latency_detector_profiled_k_pose_wave(rva, oracle_mod, scenes, lat, lat_plain):
    """Stage profiling runs k_pose<true> apart from k_decode: a wave per detection."""
    lat.set_profiling(True)
    try:
        for name in ("five", "foreign", "none"):
            lat.detect(scenes[name], rva.AT_FMT_GRAY8)
            lat_plain.detect(scenes[name], rva.AT_FMT_GRAY8)
            check_frame(rva, oracle_mod, lat, lat_plain, 0, uc.GPU_LENS, fc.GPU_SCENES[name][0])
    finally:
        lat.set_profiling(False)


def test_throughput_detector_three_frames_pose_wave(rva, oracle_mod, scenes, thr, thr_plain):
    names = ["three_two_walls", "none", "five"]
    thr.detect_batch([scenes[n] for n in names], rva.AT_FMT_GRAY8)
    thr_plain.detect_batch([scenes[n] for n in names], rva.AT_FMT_GRAY8)
    for f, n in enumerate(names):
        check_frame(rva, oracle_mod, thr, thr_plain, f, uc.GPU_LENS, fc.GPU_SCENES[n][0])


def test_throughput_detector_nine_frames_k_pose_quads(rva, oracle_mod, flat, scenes, thr, thr_plain):
    """Nine frames: k_pose<false>, four lanes per detection.  One frame is blank and one holds 18
    detections, so the 16 quads of a wave spill into the next."""
    names = ["five", "none", "crowd", "one", "two_coplanar", "three_coplanar", "three_two_walls", "foreign", "only_foreign"]
    thr.detect_batch([scenes[n] for n in names], rva.AT_FMT_GRAY8)
    thr_plain.detect_batch([scenes[n] for n in names], rva.AT_FMT_GRAY8)
    total = 0
    for f, n in enumerate(names):
        total += len(check_frame(rva, oracle_mod, thr, thr_plain, f, uc.GPU_LENS, flat[n][2]))
    assert len(thr.detections(2)) == 18 and total == 18 + 5 + 1 + 2 + 3 + 3 + 2 + 1
    assert thr.undistort_stats() == {"ideal": total, "not_invertible": 0}


def test_annotated_image_stays_raw(rva, scenes, lat, lat_plain):
    bgr = np.repeat(scenes["five"][:, :, None], 3, axis=2)
    lat.detect(bgr, rva.AT_FMT_BGR8)
    lat_plain.detect(bgr, rva.AT_FMT_BGR8)
    assert len(lat.detections(0)) == 5 and lat.frame_record_bytes(0) == lat_plain.frame_record_bytes(0)
    assert np.array_equal(lat.annotate_staged(0), lat_plain.annotate_staged(0))


# ---- the rig pose --------------------------------------------------------------------------------
def test_rig_mixes_members_with_the_mode_on_and_off(rva, scenes, lat, lat_plain):
    cam, _dist = uc.camera_of(rva, uc.GPU_LENS)
    ext = [(np.eye(3), np.zeros(3)), (fc.rot_y(20.0), np.array([0.1, 0.0, 0.05]))]
    rig = rva.RigSolver([lat, lat_plain], ext, fc.GPU_LAYOUT)
    try:
        lat.detect(scenes["five"], rva.AT_FMT_GRAY8)
        lat_plain.detect(scenes["three_two_walls"], rva.AT_FMT_GRAY8)
        got = rig.solve()[0]
        host = rva.rig_pose_host([(lat.ideal_detections(0), lat.poses(0), cam, ext[0]),
                                  (lat_plain.detections(0), lat_plain.poses(0), cam, ext[1])], fc.GPU_LAYOUT)
        assert got.n_tags == host.n_tags == 8 and got.ids == host.ids
        assert np.array_equal(got.R, host.R) and np.array_equal(got.t, host.t) and np.array_equal(got.cov, host.cov)
        assert got.rms_px == host.rms_px and got.steps_taken == host.steps_taken
        # ... and it is not what raw corners of the first member give
        rawhost = rva.rig_pose_host([(lat.detections(0), lat.poses(0), cam, ext[0]),
                                     (lat_plain.detections(0), lat_plain.poses(0), cam, ext[1])], fc.GPU_LAYOUT)
        assert not np.array_equal(rawhost.t, got.t)
    finally:
        rig.close()


# ---- a detection that is not invertible ----------------------------------------------------------
def test_detection_beyond_the_fold_is_passed_over(rva, oracle_mod):
    img = uc.fold_frame(ts.draw_tag, ts.square, ts.codes(), ts.blank)
    ln = uc.FOLD_LENS
    cam, dist = uc.camera_of(rva, ln)
    for max_batch, frames in ((1, 1), (16, 9)):
        det, plain = make(rva, ln, max_batch), make(rva, ln, max_batch, undistort=False)
        try:
            det.detect_batch([img] * frames, rva.AT_FMT_GRAY8)
            plain.detect_batch([img] * frames, rva.AT_FMT_GRAY8)
            for f in range(frames):
                raw, ideal = det.detections(f), det.ideal_detections(f)
                assert [d.id for d in raw] == [1, 2] and [d.id for d in ideal] == [-1, 2]
                for a, b in zip(ideal, rva.ideal_detections_host(raw, cam, dist)):
                    assert uc.same_detection(a, b)
                assert det.field_poses()[f].ids == [2] and plain.field_poses()[f].ids == [1, 2]
                # its own pose comes from its raw corners, as without the mode (the same kernel variant's)
                assert det.frame_record_bytes(f) == plain.frame_record_bytes(f)
                p_on, p_off = det.poses(f), plain.poses(f)
                assert [p.id for p in p_on] == [1, 2]
                assert np.abs(p_on[0].R - p_off[0].R).max() <= 1e-9 and np.abs(p_on[0].t - p_off[0].t).max() <= 1e-9
            assert det.undistort_stats() == {"ideal": frames, "not_invertible": frames}
        finally:
            det.close()
            plain.close()


# ---- lifecycle -----------------------------------------------------------------------------------
def test_mode_on_then_off_is_as_if_never_on(rva, scenes):
    import torch
    names = ["five", "three_two_walls"]
    for max_batch in (1, 16):
        det, plain = make(rva, uc.GPU_LENS, max_batch, undistort=False), make(rva, uc.GPU_LENS, max_batch, undistort=False)
        try:
            with pytest.raises(RuntimeError):
                det.ideal_detections(0)                                  # no batch yet
            det.set_undistort(True)
            det.detect(scenes["five"], rva.AT_FMT_GRAY8)
            plain.detect(scenes["five"], rva.AT_FMT_GRAY8)
            assert not all(same_pose(a, b) for a, b in zip(det.poses(0), plain.poses(0)))
            det.set_undistort(False)
            for _round in range(2):                                      # two batches in a row
                for n in names:
                    det.detect(scenes[n], rva.AT_FMT_GRAY8)
                    plain.detect(scenes[n], rva.AT_FMT_GRAY8)
                    assert det.frame_record_bytes(0) == plain.frame_record_bytes(0)
                    assert all(same_pose(a, b) for a, b in zip(det.poses(0), plain.poses(0)))
                    assert same_field(det.field_poses()[0], plain.field_poses()[0])
                    assert det.undistort_stats() == {"ideal": 0, "not_invertible": 0}
                    with pytest.raises(RuntimeError):
                        det.ideal_detections(0)                          # the last batch ran with the mode off
            # a switch while a batch is pending is refused, and leaves the mode as it was
            frame = torch.from_numpy(scenes["five"]).cuda()
            torch.cuda.synchronize()
            det.enqueue_device(frame.data_ptr(), W * H, 1, rva.AT_FMT_GRAY8)
            with pytest.raises(RuntimeError):
                det.set_undistort(True)
            det.collect()
            plain.detect(scenes["five"], rva.AT_FMT_GRAY8)
            assert all(same_pose(a, b) for a, b in zip(det.poses(0), plain.poses(0)))
        finally:
            det.close()
            plain.close()
    nopose = rva.GpuDetector(W, H, max_batch=1, tag_size=0.0)
    try:
        with pytest.raises(RuntimeError):
            nopose.set_undistort(True)                                   # tag_size 0: no pose stage
    finally:
        nopose.close()


# ---- end to end ----------------------------------------------------------------------------------
def test_field_pose_error_with_and_without_the_mode(rva, flat, scenes):
    """Scene "five" (five tags on two walls, from 122 to 540 px across the frame; camera pose known).
    The camera position error of the field pose:
      (a) mode on, the warped frame;  (b) mode off, the warped frame;
      (c) mode off, the scene drawn without distortion through a detector without distortion --
          what the pipeline achieves with no lens at all.
    Measured with the CPU oracle and the twins: (a) 0.5 mm, (b) 28.4 mm, (c) 3.2 mm; on the GPU the
    same to the digits shown (profiles/undistort/gpu_tests.txt)."""
    R, t = flat["five"][1]
    centre = -R.T @ t
    err = {}
    for key, ln, img, on in (("a", uc.GPU_LENS, scenes["five"], True), ("b", uc.GPU_LENS, scenes["five"], False),
                             ("c", uc.NO_LENS, flat["five"][0], False)):
        det = make(rva, ln, 1, undistort=on)
        try:
            det.detect(img, rva.AT_FMT_GRAY8)
            fp = det.field_poses()[0]
            assert fp.ids == [0, 1, 2, 3, 4]
            err[key] = float(np.linalg.norm(-fp.R.T @ fp.t - centre))
        finally:
            det.close()
    print("field pose, camera position error: (a) on %.4f m, (b) off %.4f m, (c) no lens %.4f m" % (err["a"], err["b"], err["c"]))
    assert err["a"] < err["b"]
    assert err["a"] <= 2.0 * err["c"]


# ---- the nodes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def node_config(tmp_path_factory):
    d = tmp_path_factory.mktemp("und_cfg")
    g = uc.GPU_LENS
    (d / "calibrationmatrix_U1.json").write_text(json.dumps(
        {"matrix": [[g.fx, 0, g.cx], [0, g.fy, g.cy], [0, 0, 1]], "disto": [[g.k1, g.k2, g.p1, g.p2, g.k3]]}))
    rot = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]
    (d / "system_config.json").write_text(json.dumps(
        {"camera_mounted_positions": {"U1": "front"},
         "extrinsics": {"front": {"rotation": rot, "offset": [0.2, 0.0, 0.5]}}}))
    return d


def test_python_node_switch(rva, scenes, node_config, lat):
    from ros_vision_amd import node as N
    kw = dict(parameters={"camera_serial": "U1"}, calibration_dir=str(node_config),
              system_config_path=str(node_config / "system_config.json"), field_layout=fc.GPU_LAYOUT)
    on, off = N.ApriltagsDetectorNode(W, H, undistort=True, **kw), N.ApriltagsDetectorNode(W, H, **kw)
    try:
        assert on.undistort and on.detector.undistort and not off.undistort and not off.detector.undistort
        r_on = on.image_callback(scenes["five"], 1000.0, encoding="mono8")
        r_off = off.image_callback(scenes["five"], 1000.0, encoding="mono8")
        lat.detect(scenes["five"], rva.AT_FMT_GRAY8)
        assert same_field(r_on.field_pose, lat.field_poses()[0])
        assert not same_field(r_off.field_pose, r_on.field_pose)
        assert on.detector.frame_record_bytes(0) == off.detector.frame_record_bytes(0)
        with pytest.raises(RuntimeError):
            off.detector.ideal_detections(0)
    finally:
        on.close()
        off.close()


def test_rig_fuser_hands_ideal_records_on(rva, scenes, node_config):
    from ros_vision_amd import node as N
    kw = dict(parameters={"camera_serial": "U1"}, calibration_dir=str(node_config),
              system_config_path=str(node_config / "system_config.json"))
    on, off = N.ApriltagsDetectorNode(W, H, undistort=True, **kw), N.ApriltagsDetectorNode(W, H, **kw)
    fuser = N.RigPoseFuser([on, off], fc.GPU_LAYOUT, publishers={})
    try:
        on.image_callback(scenes["five"], 1000.0, encoding="mono8")
        off.image_callback(scenes["three_two_walls"], 1000.0, encoding="mono8")
        frames = fuser.frames()
        for a, b in zip(frames[0][0], on.detector.ideal_detections(0)):
            assert uc.same_detection(a, b)
        for a, b in zip(frames[1][0], off.detector.detections(0)):
            assert uc.same_detection(a, b)
        assert not any(uc.same_detection(a, b) for a, b in zip(frames[0][0], on.detector.detections(0)))
        fuser.publish()
    finally:
        fuser.close()
        on.close()
        off.close()


def test_mock_node_undistort_switch(rva, scenes, node_config, lat):
    import fcntl
    with open(os.path.join(NODE, ".build.lock"), "w") as lk:   # one make at a time, as tests/test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", NODE, "-s"], check=True)
    d = node_config
    (d / "layout.txt").write_text("".join(
        "%d %s\n" % (tid, " ".join(repr(float(v)) for v in list(R.reshape(9)) + list(t))) for tid, R, t in fc.GPU_LAYOUT))
    names = ["five", "three_two_walls"]
    np.stack([scenes[n] for n in names]).tofile(d / "frames.raw")
    cmd = [os.path.join(NODE, "at_mock_node"), "--width", str(W), "--height", str(H), "--format", "gray",
           "--frames", str(d / "frames.raw"), "--camera-serial", "U1", "--calibration-dir", str(d),
           "--system-config", str(d / "system_config.json"), "--field-layout", str(d / "layout.txt")]
    runs = {}
    for key, extra in (("on", ["--undistort"]), ("off", [])):
        out = subprocess.run(cmd + extra, check=True, capture_output=True, text=True, timeout=120).stdout
        runs[key] = [json.loads(l) for l in out.splitlines()]
    assert runs["on"][0].get("undistort") is True and "undistort" not in runs["off"][0]
    for k, n in enumerate(names):
        lat.detect(scenes[n], rva.AT_FMT_GRAY8)
        fp, f_on, f_off = lat.field_poses()[0], runs["on"][1 + k]["field"], runs["off"][1 + k]["field"]
        assert f_on["ids"] == f_off["ids"] == fp.ids
        assert np.abs(np.array(f_on["R"]).reshape(3, 3) - fp.R).max() <= 1e-9 and np.abs(np.array(f_on["t"]) - fp.t).max() <= 1e-9
        assert np.abs(np.array(f_off["t"]) - fp.t).max() > 1e-3                # raw corners: centimetres away
