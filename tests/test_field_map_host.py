"""The field map on the CPU (no GPU): at_fieldmap_solve_host against the numpy restatement in
tests/field_map_cases.py bit for bit, the Jacobian against central differences, exact corners
against the true tag poses, the final cost against scipy's least squares, the covariance against the
scatter of 400 noisy solves, the placing of tags without a start, refusals and save_field_layout.
at_fieldmap_solve_host shares its arithmetic with the k_fm_* kernels (csrc/at_fieldmap.h), so what
holds here is what the device path is then held to in tests/test_field_map_gpu.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import field_map_cases as fm
import field_pose_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = 1e-9      # tests/test_rig_calib_host.py's bound for exact data


@pytest.fixture(scope="module")
def rva():
    import ros_vision_amd
    return ros_vision_amd


def tag_error(truth, recs):
    """The largest entry of R - R_true and of t - t_true over the placed tags."""
    return max(max(float(np.abs(q.R - g[1]).max()), float(np.abs(q.t - g[2]).max())) for g, q in zip(truth, recs) if q.placed)


# ---- the Jacobian ---------------------------------------------------------------------------------
def test_jacobian_against_central_differences():
    """d(u, v)/d(w, dt) of a view (R' = dR(w) R, t' = t + dt) and d(u, v)/d(w_j, d_j) of a tag
    (R_j' = R_j dR(w_j), t_j' = t_j + d_j) of the restatement's own rows against central differences
    at step 1e-6, each column held to 1e-6 of its largest entry: test_rig_calib_host.py's argument
    (rounding about 1e-7 px per unit, truncation of order h^2, columns of 300 px per unit and
    more) holds for these columns as it does there.  The link to the library is indirect, as in the
    rig calibration's test: these are the rows of the restatement, which the twin equals bit for bit
    in the tests below; this test alone passes without the library."""
    rng = np.random.default_rng(3)
    h, hs = 1e-6, fc.TAG_SIZE / 2.0
    worst = 0.0
    for tid, Rt, tt in fm.field(6):
        R, t = fc.random_camera(rng)
        for c, (sx, sy) in enumerate(fc.CORNER_SIGNS):
            jpu, jpv, jtu, jtv, _ru, _rv = fm._slot_rows(fc.CAM, (Rt.tolist(), tt.tolist()), sx * hs, sy * hs, (0.0, 0.0),
                                                         R.tolist(), t.tolist(), True, True)

            def uv(dv, dt_):
                Rv, tv = fm.rodrigues(dv[:3]) @ R, t + dv[3:]
                Rj, tj = Rt @ fm.rodrigues(dt_[:3]), tt + dt_[3:]
                return fc.project(fc.CAM, Rv, tv, fc.tag_corners_field(Rj, tj)[c:c + 1])[0][0]
            for p in range(6):
                d = np.zeros(6)
                d[p] = h
                nv = (uv(d, np.zeros(6)) - uv(-d, np.zeros(6))) / (2 * h)
                nt = (uv(np.zeros(6), d) - uv(np.zeros(6), -d)) / (2 * h)
                worst = max(worst, max(abs(nv[0] - jpu[p]), abs(nv[1] - jpv[p])) / max(abs(jpu[p]), abs(jpv[p])),
                            max(abs(nt[0] - jtu[p]), abs(nt[1] - jtv[p])) / max(abs(jtu[p]), abs(jtv[p])))
    print("field-map Jacobian: worst relative difference %.3g" % worst)
    assert worst <= 1e-6


# ---- the twin against the restatement ----------------------------------------------------------------
def check_against_restatement(rva, tags, views, **kw):
    """Every record of the twin equals the restatement's, which takes the start poses R0, t0 (the
    placing's outcome) from the twin."""
    m, kept = fm.mapper(rva, tags, views, **kw)
    got = m.solve_host()
    recs, vrecs = m.tags(), m.views()
    ref, rtags, rviews = fm.solve_ref(tags, kept, [(q.R0, q.t0) for q in recs], [q.placed for q in recs])
    for k in ("rms_before", "rms_after", "views_used", "views_skipped", "corners", "accepted", "rejected", "cov_valid"):
        assert getattr(got, k) == getattr(ref, k), (k, got, ref)
    for a, b in zip(recs, rtags):
        assert a.id == b.id and a.placed == b.placed and a.views == b.views
        assert np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t) and np.array_equal(a.cov, b.cov), a.id
    for a, b in zip(vrecs, rviews):
        assert a.used == b.used and a.n_tags == b.n_tags and a.rms_px == b.rms_px
        assert np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t)
    return m, got


def test_host_equals_the_restatement_3_tags_3_views(rva):
    rng = np.random.default_rng(766)
    truth = fm.field(3)
    _m, got = check_against_restatement(rva, fm.map_tags(truth, rng), fm.make_views(truth, 3, rng, noise_px=0.3))
    assert got.accepted > 0 and got.cov_valid


def test_host_equals_the_restatement_6_tags_33_views_of_subsets(rva):
    """Two chunks, two cameras, views of disjoint subsets, a rotation-only and a translation-only
    tag, and a view that takes no part."""
    rng = np.random.default_rng(767)
    truth = fm.field(6)
    views = fm.make_views(truth, 33, rng, noise_px=0.3, cams=(fc.CAM, fm.CAM2),
                          subsets=[(0, 1, 2), (3, 4, 5), (0, 3, 4), (1, 2, 5), (0, 1, 2, 3, 4, 5)])
    views[7] = fm.behind(views[7])
    tags = fm.map_tags(truth, rng, free={2: (True, False), 3: (False, True)})
    m, got = check_against_restatement(rva, tags, views)
    recs = m.tags()
    assert got.views_used == 32 and got.views_skipped == 1 and got.cov_valid and not m.views()[7].used
    assert np.array_equal(recs[2].t, tags[2][2]) and np.array_equal(recs[3].R, tags[3][1])
    assert np.array_equal(recs[0].R, truth[0][1]) and np.array_equal(recs[0].t, truth[0][2])


def test_host_equals_the_restatement_on_the_chain_and_the_floating_component(rva):
    truth, tags, views = fm.chain_case(np.random.default_rng(768), noise_px=0.3)
    check_against_restatement(rva, tags, views)
    truth, tags, views = fm.floating_case(np.random.default_rng(769))
    m, got = check_against_restatement(rva, tags, views)
    # at_fieldmap.h: the component floats.  What the twin gives here: the damped steps are taken (14
    # accepted) and the cost falls to the noise as in an anchored map; the undamped final matrix is
    # singular and has no Cholesky factor, so cov_valid is 0 and every covariance is zero.
    recs = m.tags()
    print("floating component: accepted %d, cov_valid %d" % (got.accepted, got.cov_valid))
    assert got.accepted == 14 and got.rms_after < 0.5 < got.rms_before and got.views_used == 8
    assert not got.cov_valid and not any(q.cov.any() for q in recs) and all(q.placed for q in recs)


# ---- exact corners -----------------------------------------------------------------------------------
def test_exact_corners_give_the_tag_poses(rva):
    """6 tags, 12 views, the free tags started 3 degrees / 30 mm off, the anchor fixed."""
    rng = np.random.default_rng(5)
    truth = fm.field(6)
    m, _kept = fm.mapper(rva, fm.map_tags(truth, rng), fm.make_views(truth, 12, rng))
    got = m.solve_host()
    recs = m.tags()
    print("exact corners: rms %.3g -> %.3g px, worst entry %.3g, %d accepted" % (got.rms_before, got.rms_after,
                                                                                  tag_error(truth, recs), got.accepted))
    assert got.views_used == 12 and got.cov_valid and got.rms_before > 1.0
    assert tag_error(truth, recs) <= EXACT and got.rms_after <= EXACT
    assert np.array_equal(recs[0].R, truth[0][1]) and np.array_equal(recs[0].t, truth[0][2])


# ---- noise ---------------------------------------------------------------------------------------------
def test_noisy_final_cost_against_scipy_least_squares(rva):
    """0.3 px noise on 6 tags x 12 views.  scipy.optimize.least_squares on the same residuals from
    the same start (the tags as given, the views' field-pose starts), parameters (w, dt) per view and
    (w_j, d_j) per free tag.  Both are minima of one function, so only rounding and the iteration cap
    separate them.  Measured: twin 44.3524962207 px^2, scipy 44.3524962249 px^2, relative excess
    -9.5e-11 (the twin's cost is the lower one); ten times an excess that is not positive is below
    the floor, so the bound is the floor: 1e-9."""
    from scipy import optimize as scipy_optimize
    rng = np.random.default_rng(11)
    truth = fm.field(6)
    tags = fm.map_tags(truth, rng)
    m, kept = fm.mapper(rva, tags, fm.make_views(truth, 12, rng, noise_px=0.3))
    got = m.solve_host()
    twin_cost = got.rms_after ** 2 * got.corners
    idx = {int(g[0]): J for J, g in enumerate(tags)}
    start_tags = [(np.asarray(g[1]), np.asarray(g[2])) for g in tags]
    layout = [(g[0], g[1], g[2]) for g in tags]
    start_cams = []
    for dets, poses, cam in kept:
        r = fc.solve_ref(dets, poses, layout, cam=cam)
        start_cams.append((np.asarray(r.R), np.asarray(r.t)))
    n, free = len(kept), [J for J, g in enumerate(tags) if g[3] or g[4]]

    def fun(x):
        cams = [(fm.rodrigues(x[6 * i:6 * i + 3]) @ start_cams[i][0], start_cams[i][1] + x[6 * i + 3:6 * i + 6]) for i in range(n)]
        tg = list(start_tags)
        for k, J in enumerate(free):
            p = x[6 * n + 6 * k:6 * n + 6 * k + 6]
            tg[J] = (start_tags[J][0] @ fm.rodrigues(p[:3]), start_tags[J][1] + p[3:])
        return fm.residuals(kept, idx, tg, cams)

    sol = scipy_optimize.least_squares(fun, np.zeros(6 * n + 6 * len(free)), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    scipy_cost = 2.0 * sol.cost
    excess = (twin_cost - scipy_cost) / scipy_cost
    print("twin %.10f px^2, scipy %.10f px^2, relative excess %.3g" % (twin_cost, scipy_cost, excess))
    assert got.rms_after < got.rms_before and excess <= 1e-9


def test_noise_rms_falls_and_covariance_matches_the_scatter(rva):
    """400 draws of 0.3 px corner noise on 6 tags x 12 views, fixed seed
    (test_rig_calib_host.py's test of the same name: its repeats and its margin): for each of the six
    parameters of each of the five free tags the empirical variance of the error (w_j from
    R_true^T R, tag frame; d_j in the field frame) over the mean reported variance lies in
    [0.7, 1.4]; in every draw the after-RMS is below the before-RMS."""
    rng = np.random.default_rng(2026)
    truth = fm.field(6)
    tags = fm.map_tags(truth, rng)
    cams = [fc.random_camera(rng) for _ in range(12)]
    m = rva.FieldMapper(tags)
    cm = rva.CameraMatrix(fx=fc.CAM.fx, cx=fc.CAM.cx, fy=fc.CAM.fy, cy=fc.CAM.cy)
    err, var = [], []
    for _ in range(400):
        m.clear()
        for dets, poses, _c in fm.views_from(truth, cams, rng, noise_px=0.3):
            assert m.add(dets, poses, cm)
        got = m.solve_host()
        assert got.cov_valid and got.rms_after < got.rms_before
        e, v = [], []
        for g, q in list(zip(truth, m.tags()))[1:]:
            dR = g[1].T @ q.R
            w = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
            e.append(np.concatenate([w, q.t - g[2]]))
            v.append(np.diag(q.cov))
        err.append(np.concatenate(e))
        var.append(np.concatenate(v))
    ratio = (np.array(err) ** 2).mean(0) / np.array(var).mean(0)
    print("variance ratios (w_j, d_j) per free tag:\n", np.round(ratio.reshape(5, 6), 3))
    assert (ratio >= 0.7).all() and (ratio <= 1.4).all()


# ---- placing ---------------------------------------------------------------------------------------------
def test_chain_placement_and_a_tag_nothing_reaches(rva):
    """C is seen only with B, B only with the anchor A: all three are placed and the refined poses
    meet the truth on exact corners.  Tags 9 and 12 are seen only with each other: placed = 0,
    zeros, and their views take no part."""
    truth, tags, views = fm.chain_case(np.random.default_rng(21))
    m, kept = fm.mapper(rva, tags, views)
    got = m.solve_host()
    recs = m.tags()
    assert [q.placed for q in recs] == [True, True, True, False, False] and got.n_placed == 3 and got.n_tags == 5
    assert got.views_used == 6 and got.views_skipped == 3 and got.corners == 6 * 8
    assert [v.used for v in m.views()] == [True, True, False] * 3
    print("chain: start %.3g m off, refined worst entry %.3g" % (max(e[0] for e in fm.position_errors(truth, recs)),
                                                                  tag_error(truth, recs)))
    assert tag_error(truth, recs) <= EXACT and got.rms_after <= EXACT
    for q in recs[3:]:
        assert not q.R.any() and not q.t.any() and not q.R0.any() and not q.cov.any() and q.views == 3


# ---- stored views -------------------------------------------------------------------------------------------
def test_views_that_are_not_stored_and_the_seventeenth_tag(rva):
    rng = np.random.default_rng(32)
    truth = fm.field(20)
    tags = fm.map_tags(truth, rng)
    m = rva.FieldMapper(tags)
    cm = rva.CameraMatrix(fx=fc.CAM.fx, cx=fc.CAM.cx, fy=fc.CAM.fy, cy=fc.CAM.cy)
    R, t = fc.random_camera(rng)
    one = fc.make_frame(truth[:1], R, t, rng)
    foreign = fc.make_frame([truth[0], fc.wall_a(500, 0.3, 0.3)], R, t, rng)      # id 500 is not in the map
    assert m.add(*one, cm) is False and m.add(*foreign, cm) is False and m.add([], [], cm) is False and len(m) == 0
    assert m.add(*fc.make_frame(truth[:17], R, t, rng), cm) is True and len(m) == 1
    assert m.add(*fc.make_frame(truth[2:6], R, t, rng), cm) is True and len(m) == 2
    got = m.solve_host()
    assert [v.n_tags for v in m.views()] == [16, 4] and got.corners == 80 and m.stats()["dropped"] == 1
    assert [q.views for q in m.tags()] == [1, 1, 2, 2, 2, 2] + [1] * 10 + [0] * 4
    with pytest.raises(ValueError):
        m.add(one[0], [], cm)


# ---- records and refusals ---------------------------------------------------------------------------------
def test_record_layouts(rva):
    from ros_vision_amd import detector as d
    assert C.sizeof(d.AtFieldmapTag) == 120 and d.AtFieldmapTag.known.offset == 104
    assert C.sizeof(d.AtFieldmapTagResult) == 8 + 8 * (12 + 12 + 36) + 8 and d.AtFieldmapTagResult.cov.offset == 200
    assert C.sizeof(d.AtFieldmapResult) == 48 and d.AtFieldmapResult.n_placed.offset == 44
    assert C.sizeof(d.AtFieldmapView) == 112 and d.AtFieldmapView.rms_px.offset == 96
    assert rva.AT_FIELDMAP_MAX_TAGS == fm.MAX_TAGS == 32 and rva.load_library().at_abi_version() == 8


def test_refused_arguments(rva):
    rng = np.random.default_rng(5)
    truth = fm.field(4)
    good = fm.map_tags(truth, rng)

    def refused(tags, **kw):
        with pytest.raises(rva.FieldPoseError) as e:
            rva.FieldMapper(tags, **kw)
        return e.value.code == -1

    free_anchor = [(good[0][0], good[0][1], good[0][2], True, False)] + good[1:]
    assert refused([]) and refused(fm.map_tags(fm.field(33), rng))                    # 0 and 33 tags
    assert refused(free_anchor)                                                        # no tag held fully fixed
    assert refused([(good[0][0], None, None, False, False)] + good[1:])                # the only fixed tag has no start
    assert refused(good, tag_size=0.0) and refused(good, tag_size=-1.0) and refused(good, max_hamming=-1)
    assert refused(good + [(1024, np.eye(3), np.zeros(3), True, True)])                # an id outside [0, 1024)
    assert refused(good + [(-1, None, None, True, True)])
    assert refused(good + [(good[1][0], None, None, True, True)])                      # an id twice
    assert refused(good + [(77, np.diag([1.0, 1.0, -1.0]), np.zeros(3), True, True)])  # a known R that is no rotation
    assert refused(good + [(77, 1.001 * np.eye(3), np.zeros(3), True, True)])
    rva.FieldMapper(good + [(77, None, None, True, True)]).close()                     # without a start: R is not read
    rva.FieldMapper(fm.map_tags(fm.field(32), rng)).close()                            # 32 tags: fine
    m = rva.FieldMapper(good)
    with pytest.raises(rva.FieldPoseError) as e:                                       # nothing stored
        m.solve_host()
    assert e.value.code == -1


def test_the_4097th_view_is_refused(rva):
    from ros_vision_amd import detector as d
    rng = np.random.default_rng(6)
    truth = fm.field(3)
    m = rva.FieldMapper(fm.map_tags(truth, rng))
    dets, poses, cam = fm.make_views(truth, 1, rng)[0]
    darr, n = d._detection_records(dets)
    parr = d._pose_records(poses, n)
    c = d.AtCamera(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
    L = rva.load_library()
    assert rva.AT_FIELDMAP_MAX_VIEWS == fm.MAX_VIEWS == 4096
    for _ in range(4096):
        assert L.at_fieldmap_add(m._h, darr, parr, n, C.byref(c)) == 1
    assert len(m) == 4096 and L.at_fieldmap_add(m._h, darr, parr, n, C.byref(c)) == -3    # AT_E_CAPACITY
    with pytest.raises(rva.FieldPoseError) as e:
        m.add(dets, poses, rva.CameraMatrix(fx=cam.fx, cx=cam.cx, fy=cam.fy, cy=cam.cy))
    assert e.value.code == -3 and len(m) == 4096
    m.clear()
    assert len(m) == 0 and m.add(dets, poses, rva.CameraMatrix(fx=cam.fx, cx=cam.cx, fy=cam.fy, cy=cam.cy)) is True


# ---- files -------------------------------------------------------------------------------------------
def test_save_field_layout_round_trip(tmp_path):
    from ros_vision_amd import node
    rng = np.random.default_rng(8)
    tags = [(7, fc.rot_xyz(3.0, -20.0, 1.0), np.array([0.25, -0.125, 0.0625])),
            (2, fc.rot_xyz(170.0, 5.0, -100.0), np.array([8.1, 0.3, 1.45])),
            (5, fc.rot_y(180.0), rng.normal(size=3)), (9, np.eye(3), np.zeros(3))]
    path = node.save_field_layout(str(tmp_path / "field.json"), tags, field_length=16.54, field_width=8.21)
    data = json.loads(open(path).read())
    assert [g["ID"] for g in data["tags"]] == [2, 5, 7, 9] and data["field"] == {"length": 16.54, "width": 8.21}
    back = node.load_field_layout(path)
    want = {g[0]: g for g in tags}
    for tid, R, t in back:
        assert np.array_equal(t, want[tid][2])                                    # the printed digits read back
        assert np.abs(R - want[tid][1]).max() <= 8 * np.finfo(float).eps
        q = data["tags"][[g["ID"] for g in data["tags"]].index(tid)]["pose"]["rotation"]["quaternion"]
        assert q["W"] >= 0 and abs(q["W"] ** 2 + q["X"] ** 2 + q["Y"] ** 2 + q["Z"] ** 2 - 1) <= 4 * np.finfo(float).eps
    again = node.save_field_layout(str(tmp_path / "again.json"), back)            # a second trip moves nothing more
    for (tid, R, t), (tid2, R2, t2) in zip(back, node.load_field_layout(again)):
        assert tid == tid2 and np.array_equal(t, t2) and np.abs(R - R2).max() <= 8 * np.finfo(float).eps
    assert "field" not in json.loads(open(again).read())


# ---- the host side under sanitizers ----------------------------------------------------------------------
def test_sanitized_standalone_program(tmp_path):
    """tests/field_map_host_check.cpp + csrc/at_fieldmap.cpp, at_fieldpose.cpp built with the host
    compiler and -fsanitize=address,undefined (the runtimes linked statically), run as a child
    process: 20 tags (one placed by the chain, one that nothing reaches, one free_rot only), 35 views
    from exact-size heap buffers (one of 17 tags, one of one tag, one from NULL arrays), the host
    solve, the records, clear, the refused calls."""
    exe = tmp_path / "field_map_host_check"
    csrc = os.path.join(ROOT, "ros_vision_amd", "csrc")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                    "-o", str(exe), os.path.join(ROOT, "tests", "field_map_host_check.cpp"),
                    os.path.join(csrc, "at_fieldmap.cpp"), os.path.join(csrc, "at_fieldpose.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "33", "2", "7", "19"]
