"""The robust rig pose on the GPU: k_rig_robust (one workgroup per instant, one wave per camera)
against its CPU twin (at_rig_pose_robust_host fed the same members' detections() and poses()),
record and info byte for byte; that it is the plain solve at infinite thresholds, drops displaced
layout tags, leaves the plain solve and the members alone; the refused calls; the node.

Frames: the 640 x 480 GRAY8 views of tests/rig_pose_cases.py.  A "displaced" tag is moved by
rig_robust_cases.SHIFT in the layout the solver is given, while the views are drawn from the
true layout."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import rig_pose_cases as rc
import rig_robust_cases as rr
import tag_scenes as ts

pytestmark = pytest.mark.gpu

W, H = 640, 480
LAYOUT = rc.RIG_LAYOUT
NO_DIST = SimpleNamespace(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
EIGHT = ["front", "foreign", "right", "blank", "left", "blank", "blank", "blank"]


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


@pytest.fixture(scope="module")
def frames():
    codes = ts.codes()
    return {name: rc.render_view(name, ts.draw_tag, codes, ts.blank) for name in rc.VIEWS}


@pytest.fixture(scope="module")
def pool(rva):
    """Detectors made on demand and kept for the module (tests/test_rig_pose_gpu.py's)."""
    made = {}

    def get(key, cam, max_batch=1):
        key = (key, cam.fx, cam.fy, cam.cx, cam.cy, max_batch)
        if key not in made:
            cm = rva.CameraMatrix(fx=cam.fx, cx=cam.cx, fy=cam.fy, cy=cam.cy)
            made[key] = rva.GpuDetector(W, H, cm, NO_DIST, max_batch=max_batch)
        return made[key]

    yield get
    for d in made.values():
        d.close()


def view_cam(name):
    return rc.VIEWS[name][5]


def cfg_of(rva, c):
    return rva.RigRobust(c.huber_px, c.reject_px, c.max_rounds, c.min_keep)


def twin(rva, dets, views, layout, cfg, frame=0):
    """(RigPose, RigRobustInfo, record bytes, info bytes) of at_rig_pose_robust_host on frame
    `frame` of every member's last collected batch."""
    return rva.rig_pose_robust_host([(d.detections(frame), d.poses(frame), view_cam(v), rc.view_mount(v))
                                     for d, v in zip(dets, views)], layout, cfg_of(rva, cfg), raw=True)


def run_rig(rva, pool, frames, views, layout, tag=""):
    """One latency-mode detector per view, each given its view; returns (detectors, solver)."""
    dets = [pool("%s%d" % (tag, i), view_cam(v)) for i, v in enumerate(views)]
    for d, v in zip(dets, views):
        d.detect(frames[v], rva.AT_FMT_GRAY8)
    return dets, rva.RigSolver(dets, [rc.view_mount(v) for v in views], layout)


def solve_both(rva, pool, frames, views, layout, cfg=rr.DEFAULT, tag=""):
    """solve_robust on the device and the twin, asserted equal byte for byte; returns the device's
    (RigPose, RigRobustInfo)."""
    dets, rig = run_rig(rva, pool, frames, views, layout, tag)
    got = rig.solve_robust(cfg_of(rva, cfg), raw=True)
    rig.close()
    assert len(got) == 1
    want = twin(rva, dets, views, layout, cfg)
    assert got[0][2] == want[2], "record"
    assert got[0][3] == want[3], "info"
    return got[0][0], got[0][1]


# ---- device against the CPU twin ------------------------------------------------------------------
def test_infinite_thresholds_are_the_plain_solve(rva, pool, frames):
    views = ["front", "right"]
    for layout in (LAYOUT, rr.displaced(LAYOUT, {4})):
        dets, rig = run_rig(rva, pool, frames, views, layout)
        plain = rig.solve()[0]
        plain_bytes = bytes(rig._buf[0])
        got, info, rec, _raw = rig.solve_robust(cfg_of(rva, rr.PLAIN), raw=True)[0]
        rig.close()
        assert rec == plain_bytes and rc.same_record(got, plain) and got.n_tags == 6
        assert info.n_kept == 6 and info.n_rejected == 0 and info.rounds == 0 and not info.starved
        assert info.n_downweighted == 0 and not any(info.rejected_mask)
        assert (rec, _raw) == twin(rva, dets, views, layout, rr.PLAIN)[2:]


def test_a_displaced_tag_is_dropped(rva, pool, frames):
    """Front + right, layout tag 4 displaced: the right camera's tag 4 is dropped, and the pose is
    within 1e-6 of the plain solve of a rig created without tag 4 (two converged minima of one
    cost; tests/test_rig_robust_host.py's bound)."""
    views = ["front", "right"]
    got, info = solve_both(rva, pool, frames, views, rr.displaced(LAYOUT, {4}))
    assert rr.dropped_views(info, got) == [(1, 4)] and info.dropped[1] == [4] and info.rounds == 1
    assert got.n_tags == 6 and info.n_kept == 5 and info.n_rejected == 1 and not info.starved
    assert got.steps_taken + got.rejected == 2 * rc.ITERS and got.cov_valid
    assert info.tag_rms_px[1][2] > 50 and max(info.tag_rms_px[0] + info.tag_rms_px[1][:2]) < 1.5
    dets, rig = run_rig(rva, pool, frames, views, rr.without(LAYOUT, {4}))
    want = rig.solve()[0]
    rig.close()
    print("tag 4 displaced: |dt| %.3g, |dR| %.3g, tag rms %s" % (np.abs(got.t - want.t).max(), np.abs(got.R - want.R).max(),
                                                             np.round(info.tag_rms_px[1], 2)))
    assert np.abs(got.t - want.t).max() <= 1e-6 and np.abs(got.R - want.R).max() <= 1e-6
    assert abs(got.rms_px - want.rms_px) <= 1e-6


def test_a_tag_seen_twice_is_dropped_twice(rva, pool, frames):
    views = ["front", "right", "left"]
    got, info = solve_both(rva, pool, frames, views, rr.displaced(LAYOUT, {0}))
    assert rr.dropped_views(info, got) == [(0, 0), (2, 0)] and info.n_rejected == 2 and info.n_kept == 8
    assert info.rejected_mask[:3] == [1, 0, 1] and info.rounds == 1


def test_a_wave_left_without_a_slot(rva, pool, frames):
    """Front + right on a layout without tags 2 and 3 and with tag 4 displaced: the right camera
    sees tag 4 alone, and once that is dropped its wave holds no valid slot and adds +0.0 to every
    sum of the second fit.
    With the default reject_px = 6 this scene starves: one bad tag of three pulls the Huber fit
    into a compromise in which all three are candidates (the twin on the CPU oracle's detections:
    tag RMS 10.8, 20.8 and 26.4 px), which is asserted too.  reject_px = 24 singles tag 4 out."""
    views = ["front", "right"]
    layout = rr.displaced(rr.without(LAYOUT, {2, 3}), {4})
    got, info = solve_both(rva, pool, frames, views, layout, rr.cfg(reject_px=24.0))
    print("a wave left empty: tag rms after", info.tag_rms_px[:2])
    assert got.tags_per_cam[:2] == [2, 1] and rr.dropped_views(info, got) == [(1, 4)]
    assert info.n_kept == 2 and info.rounds == 1 and got.cov_valid and max(info.tag_rms_px[0]) < 1.5
    got, info = solve_both(rva, pool, frames, views, layout)
    assert info.starved and info.n_rejected == 0 and info.rounds == 0 and min(info.tag_rms_px[0]) > 6.0


def test_eight_cameras(rva, pool, frames):
    """The cap: every LDS row and the whole camera-order sum of the counts; blank and foreign-only
    members, tag 4 displaced."""
    got, info = solve_both(rva, pool, frames, EIGHT, rr.displaced(LAYOUT, {4}))
    assert got.tags_per_cam == [3, 0, 3, 0, 4, 0, 0, 0] and rr.dropped_views(info, got) == [(2, 4)]
    assert info.n_kept == 9 and info.rejected_mask == [0, 0, 4, 0, 0, 0, 0, 0]
    assert [len(x) for x in info.tag_rms_px] == got.tags_per_cam


def test_mixed_batch(rva, pool, frames):
    """Four instants of two throughput-mode members, tag 4 displaced; the right camera's member
    sees its view at instants 1 and 3 and a blank frame at 0 and 2: only instants 1 and 3 have a
    tag to drop and run a second fit -- workgroups of one launch with different numbers of rounds."""
    views = ["front", "right"]
    layout = rr.displaced(LAYOUT, {4})
    a, b = pool("thr_a", rc.CAM_A, 8), pool("thr_b", rc.CAM_B, 8)
    a.detect_batch([frames["front"]] * 4, rva.AT_FMT_GRAY8)
    b.detect_batch([frames[n] for n in ("blank", "right", "blank", "right")], rva.AT_FMT_GRAY8)
    rig = rva.RigSolver([a, b], [rc.view_mount(v) for v in views], layout)
    got = rig.solve_robust(cfg_of(rva, rr.DEFAULT), raw=True)
    stats = rig.robust_stats()
    rig.close()
    assert len(got) == 4
    assert [g[1].rounds for g in got] == [0, 1, 0, 1] and [g[1].n_rejected for g in got] == [0, 1, 0, 1]
    assert [g[0].n_tags for g in got] == [3, 6, 3, 6]
    assert [g[0].steps_taken + g[0].rejected for g in got] == [rc.ITERS, 2 * rc.ITERS] * 2
    for f in range(4):
        assert got[f][2:] == twin(rva, [a, b], views, layout, rr.DEFAULT, f)[2:], f
    assert stats == {"instants_solved": 4, "tags_dropped": 2, "rounds": 2, "starved": 0, "kernel_ns": 0}


def test_starvation_and_no_rounds(rva, pool, frames):
    two = rr.displaced([g for g in LAYOUT if g[0] in (0, 1)], {1})
    got, info = solve_both(rva, pool, frames, ["front"], two)
    assert info.starved and info.n_rejected == 0 and info.n_kept == 2 == got.n_tags
    assert max(info.tag_rms_px[0]) > rr.DEFAULT.reject_px
    got, info = solve_both(rva, pool, frames, ["front", "right"], rr.displaced(LAYOUT, {4}), rr.cfg(max_rounds=0))
    assert info.rounds == 0 and info.n_rejected == 0 and not info.starved and info.n_downweighted >= 1
    assert info.tag_rms_px[1][2] > rr.DEFAULT.reject_px and got.steps_taken + got.rejected == rc.ITERS


# ---- the plain solve and the members are left alone ---------------------------------------------------
def test_the_plain_solve_is_left_alone(rva, pool, frames):
    views = ["front", "right"]
    dets, rig = run_rig(rva, pool, frames, views, rr.displaced(LAYOUT, {4}))
    rig.solve()
    before, stats = bytes(rig._buf[0]), rig.stats()
    _got, info = rig.solve_robust(rva.RigRobust())[0]
    assert info.n_rejected == 1
    assert rig.stats() == stats                       # at_rig_stats still speaks of the plain solve
    rig.solve()
    assert bytes(rig._buf[0]) == before and rig.stats() == stats
    rig.close()


def _snapshot(d):
    return ([(x.id, x.hamming, x.decision_margin, np.array(x.H), np.array(x.c), np.array(x.p))
             for x in d.detections(0)],
            [(p.id, np.array(p.R), np.array(p.t), p.err) for p in d.poses(0)])


def _equal(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def test_solve_while_pending_leaves_the_members_alone(rva, pool, frames):
    views = ["front", "right"]
    layout = rr.displaced(LAYOUT, {4})
    dets = [pool("pend%d" % i, view_cam(v)) for i, v in enumerate(views)]
    for d, v in zip(dets, views):                      # without a rig
        d.detect(frames[v], rva.AT_FMT_GRAY8)
    plain = [_snapshot(d) for d in dets]
    rig = rva.RigSolver(dets, [rc.view_mount(v) for v in views], layout)
    keep = [np.ascontiguousarray(frames[v]) for v in views]
    for d, fr in zip(dets, keep):                      # the rig solves before the members are collected
        d.enqueue_host([fr.ctypes.data], rva.AT_FMT_GRAY8)
    got = rig.solve_robust(rva.RigRobust(), raw=True)[0]
    for d in dets:
        d.collect()
    assert _equal([_snapshot(d) for d in dets], plain)
    assert got[2:] == twin(rva, dets, views, layout, rr.DEFAULT)[2:] and got[1].n_rejected == 1
    assert rig.solve_robust(rva.RigRobust(), raw=True)[0][2:] == got[2:]     # ... and again after they were
    rig.close()


# ---- refused calls ----------------------------------------------------------------------------------
def test_invalid_calls(rva, pool, frames):
    views = ["front", "right"]
    dets, rig = run_rig(rva, pool, frames, views, LAYOUT)

    def refused(cfg, solver=rig):
        with pytest.raises(rva.FieldPoseError) as e:
            solver.solve_robust(cfg)
        return e.value.code == -1

    assert refused(None)                                                  # a NULL config
    for bad in (0.0, -2.0, math.nan, -math.inf):
        assert refused(rva.RigRobust(huber_px=bad)) and refused(rva.RigRobust(reject_px=bad))
    assert refused(rva.RigRobust(max_rounds=-1)) and refused(rva.RigRobust(max_rounds=4))
    assert refused(rva.RigRobust(min_keep=0))
    for ok in (rva.RigRobust(math.inf, 6.0), rva.RigRobust(2.0, math.inf), rva.RigRobust(max_rounds=0),
               rva.RigRobust(min_keep=1)):
        assert rig.solve_robust(ok)[0][0].n_tags == 6
    rig.close()
    # what at_rig_solve refuses: members that have run no batch, then batches of different sizes
    fresh = [rva.GpuDetector(W, H, max_batch=8), rva.GpuDetector(W, H, max_batch=8)]
    eye = (np.eye(3), np.zeros(3))
    rig = rva.RigSolver(fresh, [eye, eye], LAYOUT)
    assert refused(rva.RigRobust(), rig)
    fresh[0].detect_batch([frames["front"]] * 3, rva.AT_FMT_GRAY8)
    assert refused(rva.RigRobust(), rig)
    fresh[1].detect_batch([frames["right"]] * 3, rva.AT_FMT_GRAY8)
    full = rig.solve_robust(rva.RigRobust(), raw=True)
    assert len(full) == 3 and rig.instants == 3
    part = rig.solve_robust(rva.RigRobust(), cap=2, raw=True)             # cap below the number of instants
    assert rig.instants == 3 and len(part) == 2 and all(x[2:] == y[2:] for x, y in zip(part, full))
    rig.close()
    for d in fresh:
        d.close()


# ---- the node ---------------------------------------------------------------------------------------
class _Sink:
    """Stands in for a RigCalibrator / RigTracker: keeps what it is handed."""

    def __init__(self):
        self.got = []

    def add(self, frames):
        self.got.append(frames)

    def push(self, frames, odometry, stamp_s):
        self.got.append(frames)

    def solve(self):
        raise rva_error("no tag")


def rva_error(what):
    import ros_vision_amd
    return ros_vision_amd.FieldPoseError(what, -1)


def test_rig_pose_fuser_publishes_the_robust_record(rva, frames, tmp_path):
    import json

    from ros_vision_amd import node
    views = ["front", "right"]
    layout = rr.displaced(LAYOUT, {4})
    cfg = {"camera_mounted_positions": {v: {"location": v} for v in views},
           "extrinsics": {v: {"rotation": rc.view_mount(v)[0].tolist(), "offset": rc.view_mount(v)[1].tolist()}
                          for v in views}}
    (tmp_path / "system_config.json").write_text(json.dumps(cfg))
    for v in views:
        c = view_cam(v)
        (tmp_path / ("calibrationmatrix_%s.json" % v)).write_text(json.dumps(
            {"matrix": [[c.fx, 0, c.cx], [0, c.fy, c.cy], [0, 0, 1]], "disto": [[0.0] * 5]}))
    sent = []
    nodes = [node.ApriltagsDetectorNode(W, H, {"camera_serial": v}, str(tmp_path), str(tmp_path / "system_config.json"))
             for v in views]
    cal, trk = _Sink(), _Sink()
    fuser = node.RigPoseFuser(nodes, layout, publishers={"camera/pose/rig": sent.append}, calibrator=cal, tracker=trk,
                              robust=rva.RigRobust())
    for n, v in zip(nodes, views):
        n.image_callback(frames[v], 0.0, encoding="mono8")
    pose = fuser.publish()
    want = twin(rva, [n.detector for n in nodes], views, layout, rr.DEFAULT)
    assert rc.same_record(pose, want[0]) and rr.same_info(fuser.robust_info, want[1])
    assert fuser.robust_info.dropped[1] == [4] and pose.n_tags == 6
    assert len(sent) == 1 and np.array_equal(sent[0][0], want[0].R) and np.array_equal(sent[0][1], want[0].t)
    assert np.array_equal(sent[0][2], want[0].cov)
    # the calibrator and the tracker get the frames without the dropped view, poses in step
    for sink in (cal, trk):
        assert len(sink.got) == 1
        handed = sink.got[0]
        assert [[d.id for d in dets] for dets, _p in handed] == [[0, 1, 3], [2, 3]]
        assert [[p.id for p in poses] for _d, poses in handed] == [[0, 1, 3], [2, 3]]
    # robust=None: every detection is handed on, and the plain record published
    plain = node.RigPoseFuser(nodes, layout, publishers={}, calibrator=_Sink())
    off = plain.publish()
    assert [[d.id for d in dets] for dets, _p in plain.calibrator.got[0]] == [[0, 1, 3], [2, 3, 4]]
    assert np.linalg.norm(off.t - pose.t) > 0.01 and plain.robust_info is None
    plain.close()
    fuser.close()
    for n in nodes:
        n.close()


# ---- stats ------------------------------------------------------------------------------------------
def test_stats_report_the_kernel_time_while_profiling(rva, pool, frames):
    views = ["front", "right"]
    dets, rig = run_rig(rva, pool, frames, views, rr.displaced(LAYOUT, {4}), tag="prof")
    rig.solve_robust(rva.RigRobust())
    assert rig.robust_stats()["kernel_ns"] == 0
    dets[1].set_profiling(True)
    for d, v in zip(dets, views):
        d.detect(frames[v], rva.AT_FMT_GRAY8)
    rig.solve_robust(rva.RigRobust())
    stats = rig.robust_stats()
    dets[1].set_profiling(False)
    rig.close()
    print("k_rig_robust, two cameras, one round: %.1f us" % (stats["kernel_ns"] / 1e3))
    assert stats["kernel_ns"] > 0 and stats["instants_solved"] == 1 and stats["tags_dropped"] == 1
    assert stats["rounds"] == 1 and stats["starved"] == 0
