"""The field map on the GPU: at_fieldmap_solve (the k_fm_* kernels: one wave per view, one lane per
corner; the sparse assembly of the reduced system block pair by block pair; its Cholesky solve in
one workgroup) against its CPU twin at_fieldmap_solve_host over the same stored views, bit for bit
on every record; that a solve leaves no state behind and leaves a detector's pending batch alone;
and rendered frames through a real detector end to end.  The cases are tests/field_map_cases.py's,
the ones the twin is held to the numpy restatement on in tests/test_field_map_host.py.  Each is the
smallest shape at which its part can go wrong."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import field_map_cases as fm
import field_pose_cases as fc
import tag_scenes as ts

pytestmark = pytest.mark.gpu

W, H = 640, 480
NO_DIST = SimpleNamespace(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def check_equal(m):
    got = m.solve()
    got_s = fm.snapshot(m)
    want = m.solve_host()
    assert got == want, (got, want)
    assert got_s == fm.snapshot(m)
    return got


# ---- device against the CPU twin ------------------------------------------------------------------
def test_three_tags_three_views_equal_the_twin(rva):
    rng = np.random.default_rng(900)
    truth = fm.field(3)
    m, kept = fm.mapper(rva, fm.map_tags(truth, rng), fm.make_views(truth, 3, rng, noise_px=0.3))
    got = check_equal(m)
    assert got.views_used == 3 and got.corners == 36 and got.accepted > 0 and got.rms_after < got.rms_before


@pytest.mark.parametrize("n", [33, 65])
def test_chunks_and_disjoint_subsets_equal_the_twin(rva, n):
    """33 views: a partial second chunk; 65: a third.  Views see disjoint subsets of the six tags
    (0, 3, 6 or 9, 12, 15), some see a bridge, some all: most block pairs are held by some views of
    a chunk only, and two cameras are mixed."""
    rng = np.random.default_rng(900 + n)
    truth = fm.field(6)
    views = fm.make_views(truth, n, rng, noise_px=0.3, cams=(fc.CAM, fm.CAM2),
                          subsets=[(0, 1, 2), (3, 4, 5), (0, 3, 4), (1, 2, 5), (0, 1, 2, 3, 4, 5)])
    m, kept = fm.mapper(rva, fm.map_tags(truth, rng), views)
    got = check_equal(m)
    assert len(m) == n and got.views_used == n and got.accepted > 0 and got.cov_valid
    assert got.rms_after < 0.5 < got.rms_before


def test_thirty_two_tags_and_the_seventeenth_tag_of_a_view(rva):
    """M = 192, the solve's cap: 32 tags in 9 views of 16; view 4 is offered 17 and drops one."""
    truth, tags, views = fm.windows_case(np.random.default_rng(932))
    m, kept = fm.mapper(rva, tags, views)
    got = check_equal(m)
    assert got.n_tags == got.n_placed == 32 and got.views_used == 9 and got.corners == 9 * 64
    assert m.stats()["dropped"] == 1 and all(v.n_tags == 16 for v in m.views())
    assert got.accepted > 0 and got.cov_valid and all(q.views > 0 for q in m.tags())


def test_a_view_that_takes_no_part_in_the_middle_of_a_chunk(rva):
    rng = np.random.default_rng(933)
    truth = fm.field(6)
    views = fm.make_views(truth, 12, rng, noise_px=0.3)
    views[5] = fm.behind(views[5])
    m, kept = fm.mapper(rva, fm.map_tags(truth, rng), views)
    got = check_equal(m)
    recs = m.views()
    assert got.views_used == 11 and got.views_skipped == 1 and not recs[5].used and recs[4].used and recs[6].used
    assert not recs[5].R.any() and recs[5].rms_px == 0 and got.accepted > 0


def test_chain_placement_and_an_unplaced_tag_equal_the_twin(rva):
    truth, tags, views = fm.chain_case(np.random.default_rng(934), noise_px=0.3)
    m, kept = fm.mapper(rva, tags, views)
    got = check_equal(m)
    recs = m.tags()
    assert [q.placed for q in recs] == [True, True, True, False, False] and got.n_placed == 3
    assert got.views_used == 6 and got.views_skipped == 3
    for q in recs[3:]:
        assert not q.R.any() and not q.t.any() and not q.cov.any() and q.views == 3


def test_rotation_only_and_translation_only_tags(rva):
    """Tag 6 is free_rot only, tag 9 free_trans only: the halves held fixed come back bit for bit."""
    rng = np.random.default_rng(935)
    truth = fm.field(6)
    tags = fm.map_tags(truth, rng, free={2: (True, False), 3: (False, True)})
    m, kept = fm.mapper(rva, tags, fm.make_views(truth, 7, rng, noise_px=0.3))
    got = check_equal(m)
    recs = m.tags()
    assert np.array_equal(recs[2].t, np.asarray(tags[2][2])) and not np.array_equal(recs[2].R, np.asarray(tags[2][1]))
    assert np.array_equal(recs[3].R, np.asarray(tags[3][1])) and not np.array_equal(recs[3].t, np.asarray(tags[3][2]))
    assert np.array_equal(recs[0].R, truth[0][1]) and np.array_equal(recs[0].t, truth[0][2])
    assert got.cov_valid and not recs[2].cov[3:, :].any() and not recs[3].cov[:3, :].any() and recs[2].cov[0, 0] > 0


def test_accepted_and_rejected_steps_equal_the_twin(rva):
    """Noisy views: the solve converges in a few accepted steps, after which the cost no longer
    falls and the remaining iterations are rejected."""
    rng = np.random.default_rng(936)
    truth = fm.field(6)
    m, kept = fm.mapper(rva, fm.map_tags(truth, rng), fm.make_views(truth, 6, rng, noise_px=0.3))
    got = check_equal(m)
    assert got.accepted > 0 and got.rejected > 0 and got.accepted + got.rejected == fm.ITERS


def test_a_component_without_a_fixed_tag_equals_the_twin(rva):
    """at_fieldmap.h: the component floats; both routes return equal records.  They hold what the twin
    gives in tests/test_field_map_host.py on this case: 14 accepted steps, the cost down to the noise,
    no factor of the undamped matrix and so no covariance."""
    truth, tags, views = fm.floating_case(np.random.default_rng(769))
    m, kept = fm.mapper(rva, tags, views)
    got = check_equal(m)
    assert got.n_placed == 5 and got.views_used == 8 and got.accepted == 14 and got.rms_after < 0.5 < got.rms_before
    assert not got.cov_valid and not any(q.cov.any() for q in m.tags())


# ---- no state left over ---------------------------------------------------------------------------
def test_two_solves_in_a_row_and_a_solve_after_clear(rva):
    rng = np.random.default_rng(938)
    truth = fm.field(6)
    views = fm.make_views(truth, 7, rng, noise_px=0.3)
    m, kept = fm.mapper(rva, fm.map_tags(truth, rng), views)
    m.solve()
    first = fm.snapshot(m)
    m.solve()
    assert fm.snapshot(m) == first
    m.clear()
    with pytest.raises(rva.FieldPoseError):
        m.solve()
    cam = rva.CameraMatrix(fx=fc.CAM.fx, cx=fc.CAM.cx, fy=fc.CAM.fy, cy=fc.CAM.cy)
    for v in views[:4]:                                    # fewer, other views in the same buffers
        assert m.add(v[0], v[1], cam)
    four = check_equal(m)
    assert four.views_used == 4 and fm.snapshot(m) != first
    for v in views[4:]:
        assert m.add(v[0], v[1], cam)
    m.solve()
    assert fm.snapshot(m) == first


def test_solve_while_a_detector_has_a_batch_pending(rva):
    """The mapper's stream is its own: a detector's batch enqueued before the solve and collected
    after it gives what it gives without a solve in between."""
    codes = ts.codes()
    frame = np.ascontiguousarray(fc.render_scene("five", ts.draw_tag, codes, ts.blank)[0])
    g = fc.GPU_CAM
    det = rva.GpuDetector(W, H, rva.CameraMatrix(fx=g.fx, cx=g.cx, fy=g.fy, cy=g.cy), NO_DIST, max_batch=1)

    def snapshot():
        return [(x.id, x.hamming, x.decision_margin, np.array(x.H).tobytes(), np.array(x.p).tobytes())
                for x in det.detections(0)]

    det.detect(frame, rva.AT_FMT_GRAY8)
    plain = snapshot()
    rng = np.random.default_rng(939)
    truth = fm.field(4)
    m, kept = fm.mapper(rva, fm.map_tags(truth, rng), fm.make_views(truth, 5, rng, noise_px=0.3))
    m.solve_host()
    want = fm.snapshot(m)
    det.enqueue_host([frame.ctypes.data], rva.AT_FMT_GRAY8)
    m.solve()
    det.collect()
    assert len(plain) == 5 and snapshot() == plain
    assert fm.snapshot(m) == want
    det.close()


def test_stats_report_the_kernel_time_while_profiling(rva):
    rng = np.random.default_rng(940)
    truth = fm.field(4)
    m, kept = fm.mapper(rva, fm.map_tags(truth, rng), fm.make_views(truth, 4, rng, noise_px=0.3))
    got = m.solve()
    assert m.stats()["kernel_ns"] == 0
    m.set_profiling(True)
    again = m.solve()
    stats = m.stats()
    print("field-map kernels, 4 views x 4 tags: %.1f us" % (stats["kernel_ns"] / 1e3))
    assert stats["kernel_ns"] > 0 and got == again
    assert stats["views_used"] == 4 and stats["views_skipped"] == 0 and stats["dropped"] == 0
    assert stats["accepted_steps"] == got.accepted and stats["rejected_steps"] == got.rejected


# ---- end to end -------------------------------------------------------------------------------------
E2E_SCENES = ("two_coplanar", "three_coplanar", "three_two_walls", "five")


def test_rendered_frames_end_to_end(rva):
    """Four rendered 640 x 480 frames of field_pose_cases' field through a detector into the mapper:
    tag 0 is the anchor, tags 1 .. 4 start 3 degrees and 30 mm off.  The refined positions are nearer
    the truth than the start's, for every free tag."""
    codes = ts.codes()
    g = fc.GPU_CAM
    cam = rva.CameraMatrix(fx=g.fx, cx=g.cx, fy=g.fy, cy=g.cy)
    det = rva.GpuDetector(W, H, cam, NO_DIST, max_batch=1)
    truth = sorted(fc.GPU_LAYOUT, key=lambda t: t[0])
    m = rva.FieldMapper(fm.map_tags(truth, np.random.default_rng(941)))
    for name in E2E_SCENES:
        img, _pose, ids = fc.render_scene(name, ts.draw_tag, codes, ts.blank)
        det.detect(np.ascontiguousarray(img), rva.AT_FMT_GRAY8)
        dets = det.detections(0)
        assert sorted(d.id for d in dets) == sorted(ids)
        assert m.add(dets, det.poses(0), cam)
    det.close()
    got = check_equal(m)
    errs = fm.position_errors(truth, m.tags())[1:]
    start_mm, final_mm = (1e3 * float(np.mean([e[k] for e in errs])) for k in (0, 1))
    line = ("field map from %d rendered views (%d corners): mean position error of 4 free tags %.2f mm at the "
            "start, %.2f mm refined (worst %.2f mm); rms %.4f -> %.4f px; %d accepted, %d rejected"
            % (got.views_used, got.corners, start_mm, final_mm, 1e3 * max(e[1] for e in errs), got.rms_before,
               got.rms_after, got.accepted, got.rejected))
    print(line)
    out = os.environ.get("AT_FIELDMAP_E2E_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"views": got.views_used, "corners": got.corners, "start_mm": start_mm, "refined_mm": final_mm,
                       "worst_refined_mm": 1e3 * max(e[1] for e in errs), "rms_before_px": got.rms_before,
                       "rms_after_px": got.rms_after}, f)
    assert got.views_used == len(E2E_SCENES) and got.n_placed == 5
    assert all(e[1] < e[0] for e in errs) and final_mm < start_mm
