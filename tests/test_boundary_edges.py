"""k_boundary's halo staging at tile and image edges.

The kernel stages a 17 x 66 halo tile (64 x 16 interior pixels from (1, 1)) by rows:
a wave per halo row, a lane per halo column, the two columns past the 64th and the
last row in a pass of their own, every address clamped into the image.  What that can
get wrong is geometry, so small GRAY8 frames at the sizes where the decimated image
ends at a different place in the last tile:

  width  128 -> 64 decimated: one full tile column, halo columns 64 / 65 outside
         136 -> 68: a last tile column 2 px wide
         248 -> 124: a last tile column 58 px wide, its halo inside the image
  height  40 -> 20: a second tile row of 2 interior rows, its halo row the last image row
          64 -> 32: the second tile row's halo row outside the image
          72 -> 36: a third tile row of 2 rows

each alone (max_batch = 1: k_boundary<false>) and all frames of a size in one batch
(max_batch = 8: k_boundary<true>), against the live oracle.  The half-flat frame puts
threshold-127 pixels (labels that take no part) beside patterned ones.
"""
import numpy as np
import pytest

from parity_util import compare_detections, compare_frame

WIDTHS = [128, 136, 248]
HEIGHTS = [40, 64, 72]
SIZES = [(w, h) for w in WIDTHS for h in HEIGHTS]
PATTERNS = ["diag_4", "noise8", "vstripes_2", "half_flat"]


def _frame(kind, W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise8":
        small = np.random.default_rng(5).integers(0, 256, size=(H // 8 + 1, W // 8 + 1), dtype=np.uint8)
        return np.ascontiguousarray(np.kron(small, np.ones((8, 8), np.uint8))[:H, :W])
    if kind == "half_flat":  # left half flat (threshold 127), right half diagonal stripes
        # (not the 2-px columns: 20 rows high they are blobs under 25 pixels, without points)
        return np.where(xx < W // 2, 128, np.where(((xx + yy) // 4) & 1, 230, 25)).astype(np.uint8)
    light = {"vstripes_2": (xx // 2) & 1, "diag_4": ((xx + yy) // 4) & 1}[kind]
    return np.where(light, 230, 25).astype(np.uint8)


def _point_xy(points):
    """Columns and rows of the oracle's point keys: x = bits 14-23, y = bits 4-13."""
    p = np.asarray(points, np.uint64)
    return (((p >> np.uint64(14)) & np.uint64(0x3ff)).astype(np.int64),
            ((p >> np.uint64(4)) & np.uint64(0x3ff)).astype(np.int64))


@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True  # the IndexPoint tap compare_frame reads
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


@pytest.fixture(scope="module")
def refs(oracle_mod):
    """(W, H, kind) -> (frame, oracle after detect): computed once, read by every test."""
    out = {}
    for W, H in SIZES:
        for kind in PATTERNS:
            frame = _frame(kind, W, H)
            orc = oracle_mod.Oracle(W, H)
            assert orc.detect(frame, 2) >= 0
            out[(W, H, kind)] = (frame, orc)
    return out


@pytest.mark.parametrize("W,H", SIZES)
def test_frames_reach_the_edges(refs, W, H):
    """Precondition, on the oracle alone: at every size one pattern has points in the
    first and the last interior row and column, and the half-flat frame has both
    threshold-127 pixels and points."""
    Wd, Hd = W // 2, H // 2
    reach = []
    for kind in PATTERNS:
        x, y = _point_xy(refs[(W, H, kind)][1].sorted_points())
        reach.append(bool((x == 1).any() and (x == Wd - 2).any() and (y == 1).any() and (y == Hd - 2).any()))
    print(W, H, dict(zip(PATTERNS, reach)))
    assert any(reach)
    orc = refs[(W, H, "half_flat")][1]
    assert (orc.thresholded() == 127).any() and orc.sorted_points().size > 0


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_single_frames(gpu, refs, W, H):
    """max_batch = 1: k_boundary<false>."""
    det = gpu.GpuDetector(W, H, max_batch=1)
    for kind in PATTERNS:
        frame, orc = refs[(W, H, kind)]
        dets = det.detect(frame, gpu.AT_FMT_GRAY8)
        assert det.frame_status(0) == orc.status(), kind
        assert compare_frame(det, orc) == [], kind
        assert compare_detections(dets, orc.detections()) == [], kind


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_batch(gpu, refs, W, H):
    """max_batch = 8 (throughput mode): k_boundary<true>, the frames of a size together."""
    det = gpu.GpuDetector(W, H, max_batch=8)
    batch = det.detect_batch([refs[(W, H, k)][0] for k in PATTERNS], gpu.AT_FMT_GRAY8)
    for c, k in enumerate(PATTERNS):
        orc = refs[(W, H, k)][1]
        assert det.frame_status(c) == orc.status(), k
        assert compare_frame(det, orc, frame_idx=c) == [], k
        assert compare_detections(batch[c], orc.detections()) == [], k
