"""The rig pose on the GPU: k_rig (one workgroup per instant, one wave per camera) against its
CPU twin (at_rig_pose_host fed the same members' detections() and poses()), bit for bit; that a
rig leaves its members alone; accuracy against the members' own field poses; the refused calls;
the node.

Frames: 640 x 480 GRAY8 views of tests/rig_pose_cases.py (VIEWS: walls A, B and C seen by cameras
of three intrinsics looking three ways; the CPU oracle decodes every drawn tag of every view, and
the smallest tag side is 70 px)."""
from types import SimpleNamespace

import numpy as np
import pytest

import field_pose_cases as fc
import rig_pose_cases as rc
import tag_scenes as ts

pytestmark = pytest.mark.gpu

W, H = 640, 480
LAYOUT = rc.RIG_LAYOUT
NO_DIST = SimpleNamespace(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)   # the frames are drawn without lens distortion


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
    """Detectors made on demand and kept for the module: pool(name, intrinsics, max_batch) is the
    detector of that name with those intrinsics."""
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


def twin(rva, dets, views, frame=0):
    """at_rig_pose_host on frame `frame` of every member's last collected batch; member i has the
    intrinsics and the mount of views[i]."""
    return rva.rig_pose_host([(d.detections(frame), d.poses(frame), view_cam(v), rc.view_mount(v))
                              for d, v in zip(dets, views)], LAYOUT)


def same(a, b):
    return rc.same_record(a, b) and a.dropped == b.dropped


def run_rig(rva, pool, frames, views, tag=""):
    """One detector per view (latency mode), each given its view; returns (detectors, solver)."""
    dets = [pool("%s%d" % (tag, i), view_cam(v)) for i, v in enumerate(views)]
    for d, v in zip(dets, views):
        d.detect(frames[v], rva.AT_FMT_GRAY8)
    return dets, rva.RigSolver(dets, [rc.view_mount(v) for v in views], LAYOUT)


# ---- device against the CPU twin ------------------------------------------------------------------
def test_two_cameras_equal_the_twin(rva, pool, frames):
    """Different intrinsics and extrinsics; two waves: the smallest shape with a cross-wave sum."""
    views = ["front", "right"]
    dets, rig = run_rig(rva, pool, frames, views)
    got = rig.solve()
    rig.close()
    assert len(got) == 1
    want = twin(rva, dets, views)
    print("two cameras: rms %.3f px, steps %d, sigma_t %s mm" % (got[0].rms_px, got[0].steps_taken,
                                                                  np.sqrt(np.diag(got[0].cov)[3:]) * 1e3))
    assert got[0].n_tags == 6 and got[0].tags_per_cam[:2] == [3, 3] and got[0].ids[:2] == [[0, 1, 3], [2, 3, 4]]
    assert got[0].cov_valid and got[0].steps_taken >= 1 and 0 < got[0].rms_px < 1.5
    assert same(got[0], want)


def test_eight_cameras_equal_the_twin(rva, pool, frames):
    """The cap: every LDS slot and the whole camera-order sum.  Three cameras see tags, one only
    the foreign id, four a blank frame."""
    views = ["front", "foreign", "right", "blank", "left", "blank", "blank", "blank"]
    dets, rig = run_rig(rva, pool, frames, views)
    got = rig.solve()[0]
    rig.close()
    assert got.tags_per_cam == [3, 0, 3, 0, 4, 0, 0, 0] and got.n_cams_used == 3 and got.n_tags == 10
    assert got.ids[0] == [0, 1, 3] and got.ids[2] == [2, 3, 4] and got.ids[4] == [0, 5, 6, 7] and got.ids[1] == []
    assert got.cov_valid
    assert same(got, twin(rva, dets, views))


def test_throughput_batch_of_four_instants(rva, pool, frames):
    """Two throughput-mode detectors, four instants: both cameras, no tag in any camera, tags in
    one camera only, and a view the mount does not belong to (a poor fit: rejected steps)."""
    views = ["front", "right"]
    a, b = pool("thr_a", rc.CAM_A, 8), pool("thr_b", rc.CAM_B, 8)
    a.detect_batch([frames[n] for n in ("front", "blank", "front", "wall_a")], rva.AT_FMT_GRAY8)
    b.detect_batch([frames[n] for n in ("right", "blank", "blank", "right")], rva.AT_FMT_GRAY8)
    rig = rva.RigSolver([a, b], [rc.view_mount(v) for v in views], LAYOUT)
    got = rig.solve()
    stats = rig.stats()
    rig.close()
    assert len(got) == 4
    assert [g.n_tags for g in got] == [6, 0, 3, 6] and [g.n_cams_used for g in got] == [2, 0, 1, 2]
    assert not got[1].R.any() and not got[1].cov.any() and not got[1].cov_valid and got[1].steps_taken == 0
    for f in range(4):
        assert same(got[f], twin(rva, [a, b], views, f)), f
    assert stats["instants_solved"] == 3 and stats["tags_used"] == 15 and stats["dropped"] == 0
    assert stats["rejected_steps"] == sum(g.rejected for g in got) and stats["kernel_ns"] == 0


# ---- the members are left alone -------------------------------------------------------------------
def _snapshot(d):
    return ([(x.id, x.hamming, x.decision_margin, np.array(x.H), np.array(x.c), np.array(x.p))
             for x in d.detections(0)],
            [(p.id, np.array(p.R), np.array(p.t), p.err) for p in d.poses(0)],
            [(f.n_tags, f.ids, f.R, f.t, f.rms_px, f.steps_taken) for f in d.field_poses()])


def _equal(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def test_solve_while_pending_leaves_the_members_alone(rva, pool, frames):
    views = ["front", "right"]
    dets = [pool("pend%d" % i, view_cam(v)) for i, v in enumerate(views)]
    for d in dets:
        d.set_field_layout(LAYOUT)
    first, second = ["front", "right"], ["wall_a", "right"]
    plain = []
    for batch in (first, second):                      # without a rig
        for d, v in zip(dets, batch):
            d.detect(frames[v], rva.AT_FMT_GRAY8)
        plain.append([_snapshot(d) for d in dets])
    rig = rva.RigSolver(dets, [rc.view_mount(v) for v in views], LAYOUT)
    for k, batch in enumerate((first, second)):        # the rig solves before the members are collected
        keep = [np.ascontiguousarray(frames[v]) for v in batch]
        for d, fr in zip(dets, keep):
            d.enqueue_host([fr.ctypes.data], rva.AT_FMT_GRAY8)
        got = rig.solve()[0]
        for d in dets:
            d.collect()
        assert _equal([_snapshot(d) for d in dets], plain[k]), k
        assert same(got, twin(rva, dets, views)), k
        assert same(rig.solve()[0], got)                 # ... and again after they were
    rig.close()
    for d in dets:
        d.set_field_layout(None)


# ---- accuracy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [("front", "right"), ("right", "left"), ("front", "right", "left")],
                         ids=lambda v: "+".join(v))
def test_rig_is_no_worse_than_its_worst_member(rva, pool, frames, views):
    """Robot position against the scene's truth: the rig's error is at most the largest of the
    members' own field-pose errors carried through robot_in_field (solve_rig_ref on the CPU
    oracle's detections of these views: 3.9 / 0.7 / 0.9 mm against 6.3 mm)."""
    views = list(views)
    dets = [pool("acc%d" % i, view_cam(v)) for i, v in enumerate(views)]
    for d, v in zip(dets, views):
        d.set_field_layout(LAYOUT)
        d.detect(frames[v], rva.AT_FMT_GRAY8)
    rig = rva.RigSolver(dets, [rc.view_mount(v) for v in views], LAYOUT)
    got = rig.solve()[0]
    rig.close()
    truth = rc.RENDER_ROBOT[1]
    member = []
    for d, v in zip(dets, views):
        _R, t = rva.robot_in_field(d.field_poses()[0], *rc.view_mount(v))
        member.append(float(np.linalg.norm(t - truth)))
        d.set_field_layout(None)
    err = float(np.linalg.norm(got.t - truth))
    print("%s: rig %.2f mm, members %s mm, sigma_t %s mm" % ("+".join(views), err * 1e3,
                                                             ["%.2f" % (m * 1e3) for m in member],
                                                             np.round(np.sqrt(np.diag(got.cov)[3:]) * 1e3, 2)))
    assert err <= max(member)


# ---- refused calls ----------------------------------------------------------------------------------
def test_invalid_calls(rva, pool, frames):
    a, b = pool("inv0", rc.CAM_A), pool("inv1", rc.CAM_B)
    eye = (np.eye(3), np.zeros(3))

    def refused(dets, extr=None, layout=LAYOUT, **kw):
        with pytest.raises(rva.FieldPoseError) as e:
            rva.RigSolver(dets, extr if extr is not None else [eye] * len(dets), layout, **kw)
        return e.value.code == -1

    assert refused([])                                                    # n_cams outside 1..8
    many = [pool("inv%d" % i, rc.CAM_A) for i in range(9)]
    assert refused(many)
    assert refused([a, None])                                             # a NULL member
    assert refused([a, b, a])                                             # the same detector twice
    off = rva.GpuDetector(W, H, max_batch=1, tag_size=0.0)
    other = rva.GpuDetector(W, H, max_batch=1, tag_size=0.2)
    assert refused([off]) and refused([a, off])                           # tag_size 0
    assert refused([a, other])                                            # ... or differing
    off.close()
    other.close()
    assert refused([a, b], layout=[])                                     # a bad layout
    assert refused([a, b], layout=LAYOUT + [fc.wall_a(1024, 0, 0)])
    assert refused([a, b], layout=LAYOUT + [fc.wall_a(3, 1.0, 1.0)])
    assert refused([a, b], layout=LAYOUT + [(9, 1.00001 * np.eye(3), np.zeros(3))])
    assert refused([a, b], max_hamming=-1)
    assert refused([a, b], extr=[eye, (np.diag([1.0, 1.0, -1.0]), np.zeros(3))])   # extrinsics: a rotation
    import torch
    if torch.cuda.device_count() > 1:                                     # members on different devices
        far = rva.GpuDetector(W, H, max_batch=1, device=1)
        assert refused([a, far])
        far.close()
    # members that have run no batch, then batches of different frame counts
    fresh = [rva.GpuDetector(W, H, max_batch=8), rva.GpuDetector(W, H, max_batch=8)]
    rig = rva.RigSolver(fresh, [eye, eye], LAYOUT)
    with pytest.raises(rva.FieldPoseError):
        rig.solve()
    fresh[0].detect_batch([frames["front"]] * 3, rva.AT_FMT_GRAY8)
    with pytest.raises(rva.FieldPoseError):
        rig.solve()
    fresh[1].detect_batch([frames["right"]] * 3, rva.AT_FMT_GRAY8)
    full = rig.solve()
    assert len(full) == 3 and rig.instants == 3
    # cap below the number of instants: cap records written, the count returned
    part = rig.solve(cap=2)
    assert rig.instants == 3 and len(part) == 2 and all(same(x, y) for x, y in zip(part, full))
    # a member given a batch of another size afterwards
    fresh[0].detect_batch([frames["front"]] * 2, rva.AT_FMT_GRAY8)
    with pytest.raises(rva.FieldPoseError) as e:
        rig.solve()
    assert e.value.code == -1
    rig.close()
    for d in fresh:
        d.close()


# ---- the node ---------------------------------------------------------------------------------------
def test_rig_pose_fuser_publishes_the_solver_record(rva, frames, tmp_path):
    import json

    from ros_vision_amd import node
    views = ["front", "right"]
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
    fuser = node.RigPoseFuser(nodes, LAYOUT, publishers={"camera/pose/rig": sent.append})
    assert fuser.rig_pose_topic == "camera/pose/rig"
    for n, v in zip(nodes, views):
        n.image_callback(frames[v], 0.0, encoding="mono8")
    pose = fuser.publish()
    want = twin(rva, [n.detector for n in nodes], views)
    assert same(pose, want) and pose.n_tags == 6
    assert len(sent) == 1 and np.array_equal(sent[0][0], want.R) and np.array_equal(sent[0][1], want.t)
    assert np.array_equal(sent[0][2], want.cov)
    for n in nodes:                                            # an instant without a tag: nothing is sent
        n.image_callback(frames["blank"], 0.0, encoding="mono8")
    assert fuser.publish().n_tags == 0 and len(sent) == 1
    fuser.close()
    for n in nodes:
        n.close()


# ---- stats ------------------------------------------------------------------------------------------
def test_stats_report_the_kernel_time_while_profiling(rva, pool, frames):
    views = ["front", "right"]
    dets, rig = run_rig(rva, pool, frames, views, tag="prof")
    rig.solve()
    assert rig.stats()["kernel_ns"] == 0
    dets[1].set_profiling(True)
    for d, v in zip(dets, views):
        d.detect(frames[v], rva.AT_FMT_GRAY8)
    got = rig.solve()[0]
    stats = rig.stats()
    dets[1].set_profiling(False)
    rig.close()
    print("k_rig, two cameras: %.1f us" % (stats["kernel_ns"] / 1e3))
    assert stats["kernel_ns"] > 0 and stats["instants_solved"] == 1 and stats["tags_used"] == 6
    assert stats["rejected_steps"] == got.rejected == rc.ITERS - got.steps_taken
