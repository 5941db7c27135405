"""Throughput mode's k_decode packs four quads into a wave, one per row of 16 lanes.

What can go wrong only there: a quad whose refine samples overflow its row's LDS
area next to quads that fit, a last group with fewer than four quads, groups of
consecutive queue entries that straddle frames (one of them empty), rows that give up
inside the decode while their neighbours go on, and a wave with a single active row.

CPU part (no marker): the oracle alone pins the quad counts, detections and refine
sample counts that make the GPU half meaningful.  GPU part: max_batch=8 detectors
against the oracle at the project's tolerances (parity_util: integer stages exact,
floats within 1e-4 with equal integer parts), and every frame alone against the same
frame inside the batch, record for record.

Which launches take the packed kernel: a max_batch >= 8 detector packs unless the
launch is pose-fused, i.e. unless it has fewer than 8 frames and tag_size > 0 (then the
pose wave's one-quad kernel runs, as in latency mode).  So every case runs twice:
"no_pose", a detector with tag_size = 0 given the batches of 1 and 4 frames as they
are, and "padded", a detector with the default tag_size given the same frames followed
by blank ones up to 8 (blank frames add no quads, so the queue is the same), where
k_pose follows the packed kernel and the poses are compared too.
"""
import numpy as np
import pytest

import tag_scenes as ts
from parity_util import compare_detections, compare_frame

W, H = ts.W, ts.H
GRAY8 = 2
ROW_REFINE = 64  # refine samples a row keeps in LDS (at_common.h kRowRefine)
SMALL = [(470, 80), (560, 80), (470, 200), (560, 200), (470, 330)]


def mixed():
    """Tag 3 on a 330-px square (border sides of 264 px) and tags 20..24 on 64-px squares."""
    img = ts.blank()
    book = ts.codes()
    ts.draw_tag(img, book[3], ts.square(200, 240, 330, 7.0))
    for k, (x, y) in enumerate(SMALL):
        ts.draw_tag(img, book[20 + k], ts.square(x, y, 64, 10 * k))
    return img


_FRAMES = {}
_ORACLES = {}


def frame(key):
    if key not in _FRAMES:
        f = {"mixed": mixed, "blank": ts.blank, "inverted": lambda: ts.polarity()[0][1],
             "plain": lambda: ts.polarity()[0][0], "angles": lambda: ts.angles("tag36h11")[0]}[key]()
        f = np.ascontiguousarray(f)
        f.setflags(write=False)
        _FRAMES[key] = f
    return _FRAMES[key]


def oracle(oracle_mod, key):
    if key not in _ORACLES:
        orc = oracle_mod.Oracle(W, H, oracle_mod.default_params(W, H, "tag36h11"))
        orc.detect(frame(key), GRAY8)
        _ORACLES[key] = orc
    return _ORACLES[key]


BATCH = ("mixed", "blank", "inverted", "angles")


def refine_samples(corners):
    """Samples per edge of a quad as the refine step counts them (float32: max(16, |edge| / 8))."""
    c = np.asarray(corners, np.float32)
    out = []
    for a in range(4):
        b = (a + 1) & 3
        nx, ny = c[b][1] - c[a][1], -c[b][0] + c[a][0]
        mag = np.sqrt(np.float32(nx * nx + ny * ny), dtype=np.float32)
        out.append(max(16, int(mag / np.float32(8))))
    return out


# ---- CPU part ---------------------------------------------------------------------

def test_oracle_mixed_scene(oracle_mod):
    orc = oracle(oracle_mod, "mixed")
    assert sorted((d["id"], d["hamming"]) for d in orc.detections()) == [(3, 0)] + [(20 + k, 0) for k in range(5)]
    quads = orc.quads()
    assert len(quads) == 6 and len(quads) % 4 != 0
    per_quad = sorted((refine_samples(c) for c, _ in quads), key=sum)
    assert all(q == [16] * 4 for q in per_quad[:5])  # exactly a row's LDS area
    assert sum(per_quad[0]) == ROW_REFINE
    big = per_quad[5]
    assert all(32 <= n <= 33 for n in big) and 129 <= sum(big) <= 132 and sum(big) > ROW_REFINE
    sides = [np.linalg.norm(np.roll(c, -1, 0) - c, axis=1) for c, _ in quads]
    assert max(s.max() for s in sides) > 260 and sorted(s.max() for s in sides)[4] < 136


def test_oracle_batch_scenes(oracle_mod):
    nq = [len(oracle(oracle_mod, k).quads()) for k in BATCH]
    nd = [len(oracle(oracle_mod, k).detections()) for k in BATCH]
    assert nq == [6, 0, 3, 14] and sum(nq) % 4 == 3
    assert nd == [6, 0, 0, 12]
    orc = oracle(oracle_mod, "plain")
    assert len(orc.quads()) == 1 and [(d["id"], d["hamming"]) for d in orc.detections()] == [(7, 0)]


# ---- GPU part ---------------------------------------------------------------------

MODES = ("no_pose", "padded")


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


@pytest.fixture(scope="module")
def dets_by_mode(gpu):
    return {"no_pose": gpu.GpuDetector(W, H, max_batch=8, family="tag36h11", tag_size=0.0),
            "padded": gpu.GpuDetector(W, H, max_batch=8, family="tag36h11")}


def run(gpu, det, mode, frames):
    """The frames through `det` as one batch (mode "padded": followed by blank frames up
    to 8, so that the launch is not pose-fused).  Returns the detections per frame."""
    batch = list(frames)
    if mode == "padded":
        batch += [frame("blank")] * (8 - len(batch))
    assert mode == "no_pose" or len(batch) >= 8  # (else the launch would be pose-fused: one quad per wave)
    return det.detect_batch(batch, gpu.AT_FMT_GRAY8)[:len(frames)]


def records(det, mode, idx):
    """Everything frame idx of the last batch returned: the at_detection records as
    bytes (every field), and the poses (R, t, err) where the detector computes them."""
    out = [det.frame_record_bytes(idx)]
    if mode == "padded":
        out += [(p.id, p.R.tobytes(), p.t.tobytes(), p.err) for p in det.poses(idx)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_mixed_scene(gpu, dets_by_mode, oracle_mod, mode):
    """A quad of 129-132 refine samples (past the row's 64) in one wave with quads of
    exactly 64; six quads: a last group of two."""
    det = dets_by_mode[mode]
    dets = run(gpu, det, mode, [frame("mixed")])[0]
    orc = oracle(oracle_mod, "mixed")
    assert compare_frame(det, orc, frame_idx=0) == []
    assert compare_detections(dets, orc.detections()) == []
    assert len(dets) == 6 and all(d.hamming == 0 for d in dets)
    if mode == "padded":
        assert [p.id for p in det.poses(0)] == [d.id for d in dets]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_batch_straddles_frames(gpu, dets_by_mode, oracle_mod, mode):
    """23 quads over frames of 6, 0, 3 and 14: groups straddle frames, one frame is
    empty, the inverted tag's three quads fail inside the decode beside rows that
    succeed.  Every frame against its own oracle run, and alone against in the batch."""
    det = dets_by_mode[mode]
    frames = [frame(k) for k in BATCH]
    got = run(gpu, det, mode, frames)
    in_batch = [records(det, mode, i) for i in range(4)]
    assert [len(d) for d in got] == [6, 0, 0, 12]
    for idx, key in enumerate(BATCH):
        orc = oracle(oracle_mod, key)
        assert compare_frame(det, orc, frame_idx=idx) == [], key
        assert compare_detections(got[idx], orc.detections()) == [], key
    assert [sum(q["accepted"] for q in det.copy_quads(i)) for i in range(4)] == [6, 0, 3, 14]
    for idx, key in enumerate(BATCH):
        alone = run(gpu, det, mode, [frames[idx]])[0]
        assert len(alone) == len(got[idx]), key
        assert records(det, mode, 0) == in_batch[idx], key


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_single_quad(gpu, dets_by_mode, oracle_mod, mode):
    """One quad in the whole batch: a wave with a single active row."""
    det = dets_by_mode[mode]
    dets = run(gpu, det, mode, [frame("plain")])[0]
    orc = oracle(oracle_mod, "plain")
    assert compare_frame(det, orc, frame_idx=0) == []
    assert compare_detections(dets, orc.detections()) == []
    assert [d.id for d in dets] == [7]
    assert sum(q["accepted"] for q in det.copy_quads(0)) == 1
