"""The field pose on the GPU: k_field against its CPU twin (at_field_pose_host fed the same
frame's detections() and poses()), in latency and throughput mode, alone and in a mixed batch;
the layout's lifecycle; accuracy against the per-tag poses; the nodes.

Frames: 640 x 480 GRAY8, a layout on two walls projected through a known camera and every tag
drawn with tests/tag_scenes.draw_tag (tests/field_pose_cases.py: GPU_SCENES; the CPU oracle
decodes every intended tag of every scene, and the smallest tag side is 71 px)."""
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import field_pose_cases as fc
import tag_scenes as ts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = os.path.join(ROOT, "node")
W, H = 640, 480
PARITY = 1e-9          # tests/test_gpu_parity.py's bound for the device pose against the host on equal inputs
NAMES = list(fc.GPU_SCENES)          # 8 scenes: the mixed batch holds each once
NO_DIST = SimpleNamespace(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)   # the frames are drawn without lens distortion
LAYOUT_TAGS = {name: [i for i in fc.GPU_SCENES[name][0] if i != 11] for name in NAMES}


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


@pytest.fixture(scope="module")
def cam(rva):
    g = fc.GPU_CAM
    return rva.CameraMatrix(fx=g.fx, cx=g.cx, fy=g.fy, cy=g.cy)


@pytest.fixture(scope="module")
def scenes():
    codes = ts.codes()
    return {name: fc.render_scene(name, ts.draw_tag, codes, ts.blank) for name in NAMES}


@pytest.fixture(scope="module")
def lat(rva, cam):
    d = rva.GpuDetector(W, H, cam, NO_DIST, max_batch=1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def thr(rva, cam):
    d = rva.GpuDetector(W, H, cam, NO_DIST, max_batch=8)
    yield d
    d.close()


def same_record(a, b):
    return (a.n_tags == b.n_tags and a.ids == b.ids and a.steps_taken == b.steps_taken and a.rms_px == b.rms_px
            and np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t))


def close_record(a, b):
    """The same tags and, within PARITY, the same pose: for records whose single-tag start poses
    come from different k_pose variants (a wave or four lanes per tag: equal within 1e-9,
    tests/test_gpu_parity.py), where the last accept / reject decisions may differ."""
    if a.n_tags != b.n_tags or a.ids != b.ids:
        return False
    return a.n_tags == 0 or max(np.abs(a.R - b.R).max(), np.abs(a.t - b.t).max(), abs(a.rms_px - b.rms_px)) <= PARITY


def check_against_twin(rva, cam, det, frame, fp, want_ids):
    """fp, the device record of `frame` of det's last batch, against the CPU twin on that frame's
    detections and poses.  Returns the worst difference."""
    host = rva.field_pose_host(det.detections(frame), det.poses(frame), fc.GPU_LAYOUT, camera_matrix=cam)
    assert fp.n_tags == host.n_tags == len(want_ids) and fp.ids == host.ids == list(want_ids)
    assert fp.steps_taken == host.steps_taken
    if not want_ids:
        assert not fp.R.any() and not fp.t.any() and fp.rms_px == 0 and fp.steps_taken == 0
        return 0.0
    worst = max(np.abs(fp.R - host.R).max(), np.abs(fp.t - host.t).max(), abs(fp.rms_px - host.rms_px))
    assert worst <= PARITY
    assert np.abs(fp.R @ fp.R.T - np.eye(3)).max() <= 1e-12
    return float(worst)


@pytest.fixture(scope="module")
def alone(rva, cam, scenes, lat):
    """Every scene alone through the latency-mode detector: name -> (record, detections, poses)."""
    lat.set_field_layout(fc.GPU_LAYOUT)
    out = {}
    for name in NAMES:
        lat.detect(scenes[name][0], rva.AT_FMT_GRAY8)
        out[name] = (lat.field_poses()[0], lat.detections(0), lat.poses(0), lat.field_stats())
    return out


# ---- device against the CPU twin ------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_latency_mode_equals_the_twin(rva, cam, scenes, lat, alone, name):
    fp, dets, poses, stats = alone[name]
    assert [d.id for d in dets] == sorted(fc.GPU_SCENES[name][0])         # every drawn tag decodes
    host = rva.field_pose_host(dets, poses, fc.GPU_LAYOUT, camera_matrix=cam)
    want = LAYOUT_TAGS[name]
    assert fp.n_tags == host.n_tags == len(want) and fp.ids == host.ids == want
    assert fp.steps_taken == host.steps_taken
    worst = 0.0
    if want:
        worst = max(np.abs(fp.R - host.R).max(), np.abs(fp.t - host.t).max(), abs(fp.rms_px - host.rms_px))
        assert np.abs(fp.R @ fp.R.T - np.eye(3)).max() <= 1e-12 and 0 < fp.rms_px < 1.5 and fp.steps_taken >= 1
    else:
        assert not fp.R.any() and not fp.t.any() and fp.rms_px == 0 and fp.steps_taken == 0
    print("%s: device - twin, worst |difference| %.3g" % (name, worst))
    assert worst <= PARITY
    assert stats["frames_solved"] == (1 if want else 0) and stats["tags_used"] == len(want)
    assert stats["dropped_by_cap"] == 0
    assert stats["rejected_steps"] == (fc.ITERS - fp.steps_taken if want else 0)


def test_throughput_batch_mixes_every_scene(rva, cam, scenes, thr, alone):
    """The 8 scenes as one batch of the throughput-mode detector: every frame against the twin,
    the batch's counters, and frame k's record equal to the one frame k gives alone: bit for bit
    with seven empty frames around it or anywhere else in the batch (the same kernels), within
    PARITY as a batch of one and through the latency-mode detector (another k_pose variant)."""
    thr.set_field_layout(fc.GPU_LAYOUT)
    thr.detect_batch([scenes[n][0] for n in NAMES], rva.AT_FMT_GRAY8)
    recs = thr.field_poses()
    assert len(recs) == 8
    worst = max(check_against_twin(rva, cam, thr, k, recs[k], LAYOUT_TAGS[n]) for k, n in enumerate(NAMES))
    stats = thr.field_stats()
    print("mixed batch: device - twin, worst |difference| %.3g" % worst)
    assert stats["frames_solved"] == 6 and stats["tags_used"] == 15 and stats["dropped_by_cap"] == 0
    assert stats["rejected_steps"] == sum(fc.ITERS - r.steps_taken for r in recs if r.n_tags) and stats["kernel_ns"] == 0
    empty = scenes["none"][0]
    for k, n in enumerate(NAMES):
        thr.detect_batch([scenes[n][0]] + [empty] * 7, rva.AT_FMT_GRAY8)
        padded = thr.field_poses()
        assert same_record(padded[0], recs[k]) and all(r.n_tags == 0 for r in padded[1:]), n
        thr.detect_batch([scenes[n][0]], rva.AT_FMT_GRAY8)
        one = thr.field_poses()
        assert len(one) == 1 and close_record(one[0], recs[k]), n
        assert close_record(alone[n][0], recs[k]), n
    # ... and wherever it stands in the batch
    order = [5, 2, 7, 0, 4, 6, 1, 3]
    thr.detect_batch([scenes[NAMES[i]][0] for i in order], rva.AT_FMT_GRAY8)
    moved = thr.field_poses()
    for pos, i in enumerate(order):
        assert same_record(moved[pos], recs[i])


# ---- accuracy against the existing path ---------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NAMES if len(LAYOUT_TAGS[n]) >= 3])
def test_camera_position_beats_the_single_tag_poses(scenes, alone, name):
    """With three or more tags the camera position from the field pose is no further from the
    truth than the median of the positions each tag's own k_pose pose gives through the layout."""
    fp, _dets, poses, _stats = alone[name]
    R, t = scenes[name][1]
    centre = -R.T @ t
    lay = {g[0]: g for g in fc.GPU_LAYOUT}
    single = []
    for p in poses:
        Rj = p.R @ lay[p.id][1].T
        single.append(np.linalg.norm(-Rj.T @ (p.t - Rj @ lay[p.id][2]) - centre))
    err = np.linalg.norm(-fp.R.T @ fp.t - centre)
    print("%s: camera position error %.4f m; single tags %s, median %.4f m"
          % (name, err, ["%.4f" % s for s in single], np.median(single)))
    assert err <= np.median(single)


# ---- lifecycle -------------------------------------------------------------------------------------------
def test_layout_lifecycle(rva, cam, scenes):
    img = scenes["three_two_walls"][0]
    plain = rva.GpuDetector(W, H, cam, NO_DIST, max_batch=1)
    det = rva.GpuDetector(W, H, cam, NO_DIST, max_batch=1)
    try:
        plain.detect(img, rva.AT_FMT_GRAY8)
        assert [f.n_tags for f in plain.field_poses()] == [0]              # never had a layout
        det.set_field_layout(fc.GPU_LAYOUT)
        det.detect(img, rva.AT_FMT_GRAY8)
        first = det.field_poses()[0]
        assert first.ids == [0, 1, 3]
        # replaced: tag 3 gone, the whole field moved by (1, 2, 3)
        shift = np.array([1.0, 2.0, 3.0])
        det.set_field_layout([(tid, R, t + shift) for tid, R, t in fc.GPU_LAYOUT if tid != 3])
        det.detect(img, rva.AT_FMT_GRAY8)
        second = det.field_poses()[0]
        assert second.ids == [0, 1]
        c1, c2 = -first.R.T @ first.t, -second.R.T @ second.t
        assert np.abs(c2 - c1 - shift).max() < 0.05
        # cleared: no field pose, and everything else as if there had never been one
        det.set_field_layout(None)
        det.detect(img, rva.AT_FMT_GRAY8)
        assert det.field_poses()[0].n_tags == 0 and det.field_stats()["frames_solved"] == 0
        assert det.frame_record_bytes(0) == plain.frame_record_bytes(0)
        for a, b in zip(det.poses(0), plain.poses(0)):
            assert a.id == b.id and np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and a.err == b.err
        # set again
        det.set_field_layout(fc.GPU_LAYOUT)
        det.detect(img, rva.AT_FMT_GRAY8)
        assert same_record(det.field_poses()[0], first)
        assert det.frame_record_bytes(0) == plain.frame_record_bytes(0)     # ... with a layout too
    finally:
        det.close()
        plain.close()


def test_invalid_calls(rva, cam, scenes):
    import torch
    det = rva.GpuDetector(W, H, cam, NO_DIST, max_batch=1)
    nopose = rva.GpuDetector(W, H, cam, NO_DIST, max_batch=1, tag_size=0.0)
    try:
        with pytest.raises(rva.FieldPoseError) as e:
            nopose.set_field_layout(fc.GPU_LAYOUT)                           # tag_size 0: no k_pose to start from
        assert e.value.code == -1
        for bad in ([fc.wall_a(1024, 0, 0)], [fc.wall_a(1, 0, 0), fc.wall_a(1, 1, 0)],
                    [(1, np.diag([1.0, 1.0, -1.0]), np.zeros(3))], [(1, 1.001 * np.eye(3), np.zeros(3))]):
            with pytest.raises(rva.FieldPoseError) as e:
                det.set_field_layout(bad)
            assert e.value.code == -1
        frame = torch.from_numpy(scenes["one"][0]).cuda()
        torch.cuda.synchronize()
        det.enqueue_device(frame.data_ptr(), W * H, 1, rva.AT_FMT_GRAY8)
        with pytest.raises(rva.FieldPoseError) as e:
            det.set_field_layout(fc.GPU_LAYOUT)                              # a batch not yet collected
        assert e.value.code == -1
        with pytest.raises(rva.FieldPoseError):
            det.field_poses()
        det.collect()
        assert det.field_poses()[0].n_tags == 0                             # the refused layout never took effect
        det.set_field_layout(fc.GPU_LAYOUT)
        det.enqueue_device(frame.data_ptr(), W * H, 1, rva.AT_FMT_GRAY8)
        det.collect()
        assert det.field_poses()[0].ids == [1]
    finally:
        det.close()
        nopose.close()


def test_kernel_time_is_reported_while_profiling(rva, scenes, lat, alone):
    lat.set_profiling(True)
    try:
        lat.detect(scenes["five"][0], rva.AT_FMT_GRAY8)
        fp, stats = lat.field_poses()[0], lat.field_stats()
        assert close_record(fp, alone["five"][0])       # (profiling runs k_pose apart from k_decode: another variant)
        assert 0 < stats["kernel_ns"] < 50_000_000
        names, _batches = lat.stage_times()
        assert list(names)[-1] == "k_pose" and "k_field" not in names
    finally:
        lat.set_profiling(False)
    lat.detect(scenes["five"][0], rva.AT_FMT_GRAY8)
    assert lat.field_stats()["kernel_ns"] == 0


# ---- the nodes ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def node_config(tmp_path_factory):
    d = tmp_path_factory.mktemp("field_cfg")
    g = fc.GPU_CAM
    (d / "calibrationmatrix_F1.json").write_text(json.dumps(
        {"matrix": [[g.fx, 0, g.cx], [0, g.fy, g.cy], [0, 0, 1]], "disto": [[0, 0, 0, 0, 0]]}))
    rot = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]
    (d / "system_config.json").write_text(json.dumps(
        {"camera_mounted_positions": {"F1": "front"},
         "extrinsics": {"front": {"rotation": rot, "offset": [0.2, 0.0, 0.5]}}}))
    (d / "layout.json").write_text(json.dumps(
        {"tags": [{"id": tid, "R": R.reshape(9).tolist(), "t": t.tolist()} for tid, R, t in fc.GPU_LAYOUT]}))
    (d / "layout.txt").write_text("# id r00 .. r22 tx ty tz\n" + "".join(
        "%d %s\n" % (tid, " ".join(repr(float(v)) for v in list(R.reshape(9)) + list(t))) for tid, R, t in fc.GPU_LAYOUT))
    return d, np.array(rot, float), np.array([0.2, 0.0, 0.5])


def test_python_node_publishes_the_robot_field_pose(rva, cam, scenes, node_config):
    from ros_vision_amd import node as N
    d, rot, off = node_config
    got = []
    node = N.ApriltagsDetectorNode(W, H, parameters={"camera_serial": "F1"}, calibration_dir=str(d),
                                   system_config_path=str(d / "system_config.json"),
                                   field_layout=str(d / "layout.json"),
                                   publishers={"camera/pose/field": got.append})
    try:
        for name in ("five", "none", "foreign"):
            res = node.image_callback(scenes[name][0], 1000.0, encoding="mono8")
            want = LAYOUT_TAGS[name]
            assert res.field_pose.ids == want
            if not want:
                assert res.robot_in_field is None
                continue
            host = rva.field_pose_host(node.detector.detections(0), node.detector.poses(0), fc.GPU_LAYOUT,
                                       camera_matrix=cam)
            Rr, tr = rva.robot_in_field(host, rot, off)
            assert np.abs(res.robot_in_field[0] - Rr).max() <= PARITY and np.abs(res.robot_in_field[1] - tr).max() <= PARITY
            assert got[-1] is res.robot_in_field
            # the camera sits at `off` in the robot frame: the robot pose puts it where the scene's camera is
            R, t = scenes[name][1]
            assert np.abs(Rr @ off + tr - (-R.T @ t)).max() < 0.03
        assert len(got) == 2                                              # nothing for the frame without a pose
        listed = N.ApriltagsDetectorNode(W, H, field_layout=fc.GPU_LAYOUT[:2])
        assert [g[0] for g in listed.field_layout] == [0, 1]
        listed.close()
    finally:
        node.close()


def test_mock_node_prints_the_same_record(rva, cam, scenes, node_config, lat, alone):
    import fcntl
    with open(os.path.join(NODE, ".build.lock"), "w") as lk:   # one make at a time, as tests/test_node_cpp.py
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-C", NODE, "-s"], check=True)
    d, rot, off = node_config
    names = ["three_two_walls", "only_foreign", "two_coplanar"]
    np.stack([scenes[n][0] for n in names]).tofile(d / "frames.raw")
    out = subprocess.run([os.path.join(NODE, "at_mock_node"), "--width", str(W), "--height", str(H), "--format", "gray",
                          "--frames", str(d / "frames.raw"), "--camera-serial", "F1", "--calibration-dir", str(d),
                          "--system-config", str(d / "system_config.json"), "--field-layout", str(d / "layout.txt")],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    lines = [json.loads(l) for l in out.splitlines()][1:]
    assert len(lines) == 3
    for rec, n in zip(lines, names):
        f, fp = rec["field"], alone[n][0]
        assert rec["field_pose_topic"] == "camera/pose/field"
        mock = rva.FieldPose(f["n_tags"], f["ids"], np.array(f["R"]).reshape(3, 3), np.array(f["t"]), f["rms_px"],
                             f["steps"])
        assert close_record(mock, fp), n
        if fp.n_tags:
            Rr, tr = rva.robot_in_field(mock, rot, off)
            assert np.abs(np.array(f["robot_R"]).reshape(3, 3) - Rr).max() <= 1e-15
            assert np.abs(np.array(f["robot_t"]) - tr).max() <= 1e-15
        else:
            assert "robot_R" not in f
