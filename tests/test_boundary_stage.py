"""k_boundary's LDS stage: 4-byte slot words, kBndStage = 2048 per 64 x 16 tile.

A tile with at most kBndStage points and a pair table that did not fill is narrow
(4-byte words carrying the pair-entry index); any other tile is crowded (8-byte keys,
a second pass over its rows).  Small frames whose tiles sit at, below and above the
stage size, alone (k_boundary<false>) and mixed in one batch (k_boundary<true>),
against the live oracle; and the stream property the stage size rests on.
"""
import numpy as np
import pytest

from parity_util import compare_detections, compare_frame

K_BND_STAGE = 2048  # at_common.h
W, H = 272, 144     # decimated 136 x 72: 3 x 5 boundary tiles, partial on both edges

PATTERNS = ["vstripes_2", "v_2_4", "diag_4", "vstripes_4", "h_2_4", "noise8"]


def _frame(kind):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "flat":
        return np.full((H, W), 128, np.uint8)
    if kind == "noise8":
        small = np.random.default_rng(5).integers(0, 256, size=(H // 8 + 1, W // 8 + 1), dtype=np.uint8)
        return np.ascontiguousarray(np.kron(small, np.ones((8, 8), np.uint8))[:H, :W])
    light = {"vstripes_2": (xx // 2) & 1, "v_2_4": xx % 6 < 2, "diag_4": ((xx + yy) // 4) & 1,
             "vstripes_4": (xx // 4) & 1, "h_2_4": yy % 6 < 2, "checker_10": ((yy // 10) + (xx // 10)) & 1}[kind]
    return np.where(light, 230, 25).astype(np.uint8)


def tile_counts(points):
    """Points per k_boundary tile (64 x 16 interior pixels from (1, 1)) of the oracle's
    point keys: x = bits 14-23, y = bits 4-13."""
    p = np.asarray(points, np.uint64)
    x = ((p >> np.uint64(14)) & np.uint64(0x3ff)).astype(np.int64)
    y = ((p >> np.uint64(4)) & np.uint64(0x3ff)).astype(np.int64)
    _, n = np.unique(((y - 1) // 16) * 1024 + (x - 1) // 64, return_counts=True)
    return n


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True  # the IndexPoint tap compare_frame reads
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


@pytest.fixture(scope="module")
def refs(oracle_mod):
    """kind -> (frame, oracle after detect): computed once, read by every test."""
    out = {}
    for kind in PATTERNS + ["flat", "checker_10"]:
        frame = _frame(kind)
        orc = oracle_mod.Oracle(W, H)
        assert orc.detect(frame, 2) >= 0
        out[kind] = (frame, orc)
    return out


@pytest.mark.gpu
def test_tile_counts_reach_both_paths(refs):
    """The frames hold a tile of exactly kBndStage points (narrow at capacity), one
    above it (crowded) and one between the former 1024-point stage and the new one."""
    n = np.concatenate([tile_counts(refs[k][1].sorted_points()) for k in PATTERNS])
    print("tile counts:", {k: sorted(set(tile_counts(refs[k][1].sorted_points()).tolist())) for k in PATTERNS})
    assert (n == K_BND_STAGE).any()
    assert (n > K_BND_STAGE).any()
    assert ((n >= 1025) & (n <= K_BND_STAGE - 1)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PATTERNS)
def test_single_frame(gpu, refs, kind):
    """max_batch = 1: k_boundary<false>."""
    frame, orc = refs[kind]
    det = gpu.GpuDetector(W, H, max_batch=1)
    dets = det.detect(frame, gpu.AT_FMT_GRAY8)
    assert det.frame_status(0) == orc.status()
    assert compare_frame(det, orc) == []
    assert compare_detections(dets, orc.detections()) == []


@pytest.mark.gpu
def test_mixed_batch(gpu, refs):
    """max_batch = 8: k_boundary<true>, narrow and crowded tiles side by side."""
    kinds = PATTERNS + ["flat", "checker_10"]
    det = gpu.GpuDetector(W, H, max_batch=8)
    batch = det.detect_batch([refs[k][0] for k in kinds], gpu.AT_FMT_GRAY8)
    for c, k in enumerate(kinds):
        orc = refs[k][1]
        assert det.frame_status(c) == orc.status(), k
        assert compare_frame(det, orc, frame_idx=c) == [], k
        assert compare_detections(batch[c], orc.detections()) == [], k


def test_stream_tiles_fit_the_stage(oracle_mod):
    """The workload property the stage size rests on: no tile of the 720p stream holds
    more than kBndStage points (so none is crowded), and some hold more than 1024."""
    from ros_vision_amd import synth
    n = []
    for f in range(4):
        orc = oracle_mod.Oracle(1280, 720)
        orc.detect(synth.stream_frame(1280, 720, f)[0], 0)
        n.append(tile_counts(orc.sorted_points()))
    n = np.concatenate(n)
    print("stream tiles: max %d, over 1024: %.1f %%" % (n.max(), 100.0 * (n > 1024).mean()))
    assert n.max() <= K_BND_STAGE
    assert (n > 1024).any()
