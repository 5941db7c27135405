"""Decode, host-tail and parameter parity on the scenes of tests/tag_scenes.py.

The back half of the pipeline away from its default corner: decoded orientations
1..3 (rotate90 on the device, the rot field of k_decode's packed min-reduction,
H Rz(rot) and the fused pose's R0 Rz(rot)), hamming 1 and 2 and the rejection at 3,
inverted and mirrored tags, reconcile_detections in the host tail, every tunable
at_config field away from its default, and a non-default tag size.

CPU part (no marker): the oracle alone on every scene, pinning the outcomes that
make the GPU half meaningful.  GPU part: latency mode (max_batch=1) and throughput
mode (max_batch=8, the scene between two other scenes of one detect_batch) against
the oracle with the project's tolerances (parity_util: integer stages bit-exact,
floats within 1e-4 with equal integer parts).
"""
import numpy as np
import pytest

import tag_scenes as ts
from parity_util import compare_detections, compare_frame

W, H = ts.W, ts.H
GRAY8 = 2
FAMILIES = ("tag36h11", "tag25h9", "tag16h5")

# ---- scenes and their oracle runs, built once per module -----------------------

_SCENES = {}
_ORACLES = {}


def _overlap_variant(i):
    c = ts.codes()
    a, b, shift = [(c[7], c[7], 0), (c[7], c[7] ^ (1 << 20), 0), (c[7] ^ (1 << 20), c[7], 0), (c[7], c[8], 0),
                   (c[7], c[7], 24)][i]
    return ts.overlap(a, b, shift)


def scene(key):
    """(frame, truth, family) of "angles/<family>", "flipped/<family>", "quarter/<r>",
    "polarity/<i>", "overlap/<i>" or "param"."""
    if key not in _SCENES:
        kind, _, arg = key.partition("/")
        family = arg if kind in ("angles", "flipped") else "tag36h11"
        if kind == "angles":
            frame, truth = ts.angles(family)
        elif kind == "flipped":
            frame, truth = ts.angles_flipped(family)
        elif kind == "quarter":
            frame, truth = ts.quarter_turns(int(arg))
        elif kind == "polarity":
            frames, truth = ts.polarity()
            frame = frames[int(arg)]
        elif kind == "overlap":
            frame, truth = _overlap_variant(int(arg))
        else:
            frame, truth = ts.param_frame()
        frame = np.ascontiguousarray(frame)
        frame.setflags(write=False)
        _SCENES[key] = (frame, truth, family)
    return _SCENES[key]


def oracle(oracle_mod, key, **override):
    """The oracle after detecting scene `key` with the given parameter overrides."""
    k = (key, tuple(sorted(override.items())))
    if k not in _ORACLES:
        frame, _, family = scene(key)
        prm = oracle_mod.default_params(W, H, family)
        for name, v in override.items():
            setattr(prm, name, v)
        orc = oracle_mod.Oracle(W, H, prm)
        orc.detect(frame, GRAY8)
        _ORACLES[k] = orc
    return _ORACLES[k]


def id_hamming(orc):
    return [(d["id"], d["hamming"]) for d in orc.detections()]


def stage_counts(orc):
    return (orc.num_pairs(), int(orc.sorted_index_points().size), sum(1 for f in orc.fitquads() if f.valid),
            len(orc.quads()))


def quad_rotation(d, quads):
    """Index of the corner of the detection's fitted quad nearest its p[0]: which of the
    four rotations quick_decode matched (the quad's corner order is the fit's, p's is
    the tag's)."""
    cands = [c for c, b in quads if b == d["blob_index"]]
    c = min(cands, key=lambda c: float(np.abs(c.mean(0) - d["c"]).max()))
    return ts.nearest_corner(d["p"][0], c)


# ---- CPU part: what the oracle makes of the scenes ------------------------------

def test_scene_rotate90_matches_oracle(oracle_mod):
    L = oracle_mod.lib()
    rng = np.random.default_rng(8)
    for nbits in (36, 25, 16):
        for _ in range(20):
            code = int(rng.integers(0, 1 << nbits))
            for r in range(4):
                want = code
                for _k in range(r):
                    want = int(L.ao_rotate90_n(want, nbits))
                assert ts.rotate90_n(code, nbits, r) == want


def test_oracle_angles_and_quarter_turns_cover_every_orientation(oracle_mod):
    """angles: all 12 tags of each family, hamming 0.  Decoded orientation (index of the
    truth corner nearest p[0]): every value 0..3 at least twice over angles and the
    four quarter_turns boards; within angles the four rotations of quick_decode (p[0]
    against the fitted quad's corner order) occur three times each."""
    seen = []
    for fam in FAMILIES:
        orc = oracle(oracle_mod, "angles/" + fam)
        assert id_hamming(orc) == [(k, 0) for k in ts.ANGLE_IDS], fam
    orc = oracle(oracle_mod, "angles/tag36h11")
    truth = dict(scene("angles/tag36h11")[1])
    assert len(orc.quads()) == 14
    seen += [ts.nearest_corner(d["p"][0], truth[d["id"]]) for d in orc.detections()]
    rots = [quad_rotation(d, orc.quads()) for d in orc.detections()]
    assert sorted(rots) == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3, rots
    per_turn = []
    for r in range(4):
        orc = oracle(oracle_mod, "quarter/%d" % r)
        truth = dict(scene("quarter/%d" % r)[1])
        assert id_hamming(orc) == [(i, 0) for i in ts.QUARTER_IDS], r
        assert len(orc.quads()) == 15
        o = [ts.nearest_corner(d["p"][0], truth[d["id"]]) for d in orc.detections()]
        assert len(set(o)) == 1, (r, o)  # the whole board turns together
        per_turn.append(o[0])
        seen += o
        assert len({quad_rotation(d, orc.quads()) for d in orc.detections()}) == 1
    assert sorted(per_turn) == [0, 1, 2, 3], per_turn  # p[0] on another truth corner for each r
    assert all(seen.count(v) >= 2 for v in range(4)), seen


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_hamming_scene(oracle_mod, family):
    """k % 4 flipped bits: hamming 0, 1, 2 decode with that hamming, 3 bits do not (9
    detections).  For tag16h5 (codes 5 apart) a 3-bit error may land within 2 bits of
    another codeword; whatever the oracle returns there, the tag's own id is absent."""
    orc = oracle(oracle_mod, "flipped/" + family)
    got = id_hamming(orc)
    want = [(k, k % 4) for k in ts.ANGLE_IDS if k % 4 != 3]
    assert all(len(ts.flipped_bits(k, family)) == k % 4 for k in ts.ANGLE_IDS)
    if family == "tag16h5":
        assert [g for g in got if g[0] in dict(want)] == want
        assert not any(i % 4 == 3 and i in ts.ANGLE_IDS for i, _ in got)
    else:
        assert got == want
    assert len(orc.quads()) >= 12  # every tag still yields its quad: decode rejects the 3-bit ones


def test_oracle_polarity_scene(oracle_mod):
    """Plain: id 7 from 1 quad.  Inverted: 3 quads, none decodes (reversed_border == 0).
    Mirrored: 1 quad, no decode."""
    got = [(id_hamming(oracle(oracle_mod, "polarity/%d" % i)), len(oracle(oracle_mod, "polarity/%d" % i).quads()))
           for i in range(3)]
    assert got == [([(7, 0)], 1), ([], 3), ([], 1)]


def test_oracle_overlap_scene(oracle_mod):
    """reconcile_detections: two overlapping quads of one id leave the one with the
    smaller hamming, then the larger margin; other ids and disjoint quads both stay."""
    res = []
    for i in range(5):
        orc = oracle(oracle_mod, "overlap/%d" % i)
        assert len(orc.quads()) == 2, i
        res.append([(d["id"], d["hamming"], [int(round(v)) for v in d["c"]]) for d in orc.detections()])
    assert res[0] == [(7, 0, [200, 200])]  # equal hamming: A's margin is larger
    assert res[1] == [(7, 0, [200, 200])]  # B has hamming 1
    assert res[2] == [(7, 0, [356, 356])]  # A has hamming 1: hamming goes before margin
    assert res[3] == [(7, 0, [200, 200]), (8, 0, [356, 356])]
    assert res[4] == [(7, 0, [200, 200]), (7, 0, [380, 380])]
    a = oracle(oracle_mod, "overlap/0").detections()[0]
    assert abs(a["c"][0] - 200.5) < 0.1 and abs(a["c"][1] - 200.1) < 0.1


def test_oracle_param_scene_moves_with_every_override(oracle_mod):
    """Every non-default parameter value changes a stage count, a margin or a corner of
    the parameter frame, so a kernel ignoring the field cannot match the oracle."""
    base = oracle(oracle_mod, "param")
    assert [d["id"] for d in base.detections()] == [3, 100, 200]
    assert stage_counts(base) == (146, 18564, 88, 53)

    def floats(orc):
        return [(d["decision_margin"], d["p"].tolist()) for d in orc.detections()]

    want = {"min_cluster_pixels=100": (146, 14934, 38, 10), "max_line_fit_mse=0.3": (146, 18564, 44, 42),
            "max_line_fit_mse=40.0": (146, 18564, 96, 54), "cos_critical_rad=0.5": (146, 18564, 85, 47),
            "cos_critical_rad=0.999": (146, 18564, 88, 55), "min_white_black_diff=40": (93, 12443, 63, 49),
            "min_white_black_diff=120": (104, 7507, 53, 40)}
    for ov in ts.OVERRIDES + [ts.ALL_OVERRIDES]:
        orc = oracle(oracle_mod, "param", **ov)
        assert stage_counts(orc) != stage_counts(base) or floats(orc) != floats(base), ov
        assert len(orc.detections()) > 0, ov
        name = ",".join("%s=%s" % kv for kv in ov.items())
        if name in want:
            assert stage_counts(orc) == want[name], ov
    for ov in (dict(refine_edges=0), dict(decode_sharpening=0.0), dict(decode_sharpening=1.0)):
        orc = oracle(oracle_mod, "param", **ov)
        assert stage_counts(orc) == stage_counts(base)
        m = [abs(a["decision_margin"] - b["decision_margin"]) for a, b in zip(orc.detections(), base.detections())]
        assert min(m) > 1e-3, (ov, m)  # far beyond the 1e-4 the GPU comparison allows
    assert stage_counts(oracle(oracle_mod, "param", **ts.ALL_OVERRIDES)) == (93, 9259, 10, 6)


# ---- GPU part -------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True  # the IndexPoint tap (copy_blob_points) for every detector here
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


_FILLERS = ("param", "quarter/2", "polarity/0")


def run_case(gpu, oracle_mod, key, batch, **override):
    """Scene `key` through a detector of max_batch `batch` (1: latency mode, alone; 8:
    throughput mode, as frame 1 of 3): every stage and the detections against the
    oracle.  Returns (detector, detections, oracle)."""
    frame, _, family = scene(key)
    orc = oracle(oracle_mod, key, **override)
    det = gpu.GpuDetector(W, H, max_batch=batch, family=family, **override)
    if batch == 1:
        dets, idx = det.detect(frame, gpu.AT_FMT_GRAY8), 0
    else:
        others = [scene(k)[0] for k in _FILLERS if k != key][:2]
        dets, idx = det.detect_batch([others[0], frame, others[1]], gpu.AT_FMT_GRAY8)[1], 1
    assert compare_frame(det, orc, frame_idx=idx) == [], (key, batch, override)
    assert compare_detections(dets, orc.detections()) == [], (key, batch, override)
    return det, dets, orc


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", ["angles", "flipped"])
def test_gpu_angles_and_bit_errors(gpu, oracle_mod, kind, family, batch):
    """Tags at 17, 47, .. 347 degrees (all four decoded rotations; tag25h9: the odd-nbits
    centre bit of rotate90) and with 0..3 flipped bits (hamming 1, 2 kept, 3 dropped)."""
    _, dets, _ = run_case(gpu, oracle_mod, "%s/%s" % (kind, family), batch)
    assert len(dets) >= (12 if kind == "angles" else 9)
    if kind == "flipped":
        assert {d.hamming for d in dets} == {0, 1, 2}


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_gpu_quarter_turns(gpu, oracle_mod, r, batch):
    """Codewords turned r quarter turns inside unchanged outlines: H Rz(rot), c and the
    corner order p follow the decoded rotation."""
    _, dets, _ = run_case(gpu, oracle_mod, "quarter/%d" % r, batch)
    assert [d.id for d in dets] == list(ts.QUARTER_IDS)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_gpu_polarity(gpu, oracle_mod, i, batch):
    """The plain tag decodes; its negative (white border: three quads) and its mirror
    image (one quad) give quads but no detection."""
    det, dets, orc = run_case(gpu, oracle_mod, "polarity/%d" % i, batch)
    assert [d.id for d in dets] == ([7] if i == 0 else [])
    idx = 0 if batch == 1 else 1
    assert sum(q["accepted"] for q in det.copy_quads(idx)) == (3 if i == 1 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("i", [0, 1, 2, 3, 4])
def test_gpu_overlap_reconcile(gpu, oracle_mod, i, batch):
    """The host tail's reconcile_detections: both tags decode on the device (two
    candidates), the host keeps what the oracle keeps."""
    det, dets, orc = run_case(gpu, oracle_mod, "overlap/%d" % i, batch)
    assert len(dets) == (1 if i < 3 else 2)
    # the candidates of this frame alone (batch_stats sums over the batch's frames)
    alone = det.detect_batch([scene("overlap/%d" % i)[0]], gpu.AT_FMT_GRAY8)[0]
    assert compare_detections(alone, orc.detections()) == []
    assert det.batch_stats()["candidates"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("override", ts.OVERRIDES + [ts.ALL_OVERRIDES],
                         ids=lambda ov: ",".join("%s=%s" % kv for kv in ov.items()) if len(ov) == 1 else "all")
def test_gpu_parameters(gpu, oracle_mod, override, batch):
    """Every tunable at_config field at a non-default value (one at a time, then all
    at once) on a frame where the value changes the oracle's result."""
    _, dets, orc = run_case(gpu, oracle_mod, "param", batch, **override)
    assert len(orc.detections()) > 0 and len(dets) > 0


# ---- pose under rotation ---------------------------------------------------------

def _pose_close(a_R, a_t, b_R, b_t, tol):
    return np.abs(np.asarray(a_R) - np.asarray(b_R)).max() <= tol and np.abs(np.asarray(a_t) - np.asarray(b_t)).max() <= tol


def _pose_diff(a, b):
    return max(float(np.abs(a.R - b.R).max()), float(np.abs(a.t - b.t).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["quarter/0", "quarter/1", "quarter/2", "quarter/3", "angles/tag36h11"])
def test_gpu_pose_under_rotation(gpu, oracle_mod, key):
    """The three pose paths at every decoded rotation (the boards r = 0 and r = 2 decode
    with the two odd rotations of k_decode, r = 1 with the half turn, r = 3 with none;
    angles has three tags of each): the latency mode's fused pose (k_decode<true>: pose
    of the unrotated quad, then R0 Rz(rot)), k_pose<true> (latency mode while
    profiling) and k_pose<false> (throughput mode), both on the rotated H and
    corners.  (a) fused against the oracle's pose of the oracle's detection, 1e-4;
    (b) against the oracle's pose of the GPU's own H and p, 1e-9; (c) the three paths
    agree to 1e-9 on R, t and err."""
    cam = gpu.TEST_CAMERA
    frame = scene(key)[0]
    orc = oracle(oracle_mod, key)
    odets = {d["id"]: d for d in orc.detections()}
    det = gpu.GpuDetector(W, H, max_batch=1)
    dets = det.detect(frame, gpu.AT_FMT_GRAY8)
    fused = det.poses()
    assert [d.id for d in dets] == [d["id"] for d in orc.detections()] and len(fused) == len(dets) > 0
    for d, p in zip(dets, fused):  # (a)
        assert p.id == d.id
        od = odets[d.id]
        R, t, err, (e1, e2), _ = oracle_mod.estimate_tag_pose(od["H"], od["p"], cam.fx, cam.fy, cam.cx, cam.cy)
        if abs(e1 - e2) <= 1e-9 * max(e1, e2, 1e-30):
            continue  # two minima with equal error: either is the reference's answer
        assert _pose_close(p.R, p.t, R, t, 1e-4), (d.id, p.R, R, p.t, t)
        assert abs(p.err - err) <= 1e-4 * max(1.0, abs(err))
    worst_b = 0.0
    for d, p in zip(dets, fused):  # (b)
        R, t, _, _, _ = oracle_mod.estimate_tag_pose(d.H, d.p, cam.fx, cam.fy, cam.cx, cam.cy)
        worst_b = max(worst_b, float(np.abs(p.R - R).max()), float(np.abs(p.t - t).max()))
    det.set_profiling(True)  # direct launches: the pose comes from k_pose<true>
    again = det.detect(frame, gpu.AT_FMT_GRAY8)
    wave = det.poses()
    det.set_profiling(False)
    assert [d.id for d in again] == [d.id for d in dets]
    det8 = gpu.GpuDetector(W, H, max_batch=8)
    assert [d.id for d in det8.detect_batch([frame], gpu.AT_FMT_GRAY8)[0]] == [d.id for d in dets]
    quad = det8.poses(0)
    assert len(wave) == len(quad) == len(fused)
    worst_c = max(max(_pose_diff(f, w), _pose_diff(f, q), _pose_diff(w, q)) for f, w, q in zip(fused, wave, quad))
    print("%s: fused vs oracle on the GPU's H, p %.3g; between the pose paths %.3g" % (key, worst_b, worst_c))
    assert worst_b <= 1e-9
    for f, w, q in zip(fused, wave, quad):  # (c)
        assert f.id == w.id == q.id
        assert _pose_close(f.R, f.t, w.R, w.t, 1e-9), (f.id, f.R, w.R, f.t, w.t)
        assert _pose_close(f.R, f.t, q.R, q.t, 1e-9), (f.id, f.R, q.R, f.t, q.t)
        assert _pose_close(w.R, w.t, q.R, q.t, 1e-9), (f.id, w.R, q.R, w.t, q.t)
        assert f.err == pytest.approx(w.err, rel=1e-9, abs=1e-15)
        assert f.err == pytest.approx(q.err, rel=1e-9, abs=1e-15)


@pytest.mark.gpu
def test_gpu_tag_size(gpu, oracle_mod):
    """tag_size 0.2 m: the pose against estimate_tag_pose(tagsize=0.2) at 1e-4, and t
    scales by 0.2 / 0.1651 against the default run."""
    cam = gpu.TEST_CAMERA
    frame = scene("quarter/1")[0]
    orc = oracle(oracle_mod, "quarter/1")
    odets = {d["id"]: d for d in orc.detections()}
    big = gpu.GpuDetector(W, H, tag_size=0.2)
    dets = big.detect(frame, gpu.AT_FMT_GRAY8)
    poses = big.poses()
    std = gpu.GpuDetector(W, H)
    std.detect(frame, gpu.AT_FMT_GRAY8)
    ref = std.poses()
    assert [p.id for p in poses] == [p.id for p in ref] == list(ts.QUARTER_IDS)
    assert compare_detections(dets, orc.detections()) == []
    for p, q in zip(poses, ref):
        od = odets[p.id]
        R, t, err, (e1, e2), _ = oracle_mod.estimate_tag_pose(od["H"], od["p"], cam.fx, cam.fy, cam.cx, cam.cy,
                                                              tagsize=0.2)
        if not abs(e1 - e2) <= 1e-9 * max(e1, e2, 1e-30):
            assert _pose_close(p.R, p.t, R, t, 1e-4), (p.id, p.R, R, p.t, t)
        assert np.allclose(p.t, q.t * (0.2 / 0.1651), rtol=1e-6, atol=0), (p.id, p.t, q.t)
