"""The blob kernels at every cut of their routing, with blobs of an exact point count.

A pair of components is routed by its exact number of boundary points n:

  size_class()      cuts at 64, 128, 256, 512 (kSmallBlob), 1024 and 2048
  latency mode      n <= 512 a wave, n > 512 a 512-thread team: k_blob_lat (geometries with
                    max_cluster = 2 (W + H) <= 4096), k_blob<512, 4096, true> +
                    k_blob_small<true> when the kernels are timed apart, k_extents +
                    k_blob<512, kSortCap> + k_blob_small<true> + k_fit_quads above 4096
  throughput mode   a call of 8 frames or more (kWideBlobMaxBatch; the launches go by the
                    call's frame count, not by max_batch): k_extents, then n <= 512
                    k_blob_small<false>, 513-1024 k_blob_small<false, 1024, 3, 9>, 1025-4096
                    k_blob<256, 4096>, above 4096 k_blob<AT_BIG_NT, kSortCap> with nlo = 4096,
                    then k_fit_quads; a call of fewer frames: k_extents, n <= 512
                    k_blob_small<false>, n > 512 k_blob<512, 4096> or (max_cluster > 4096)
                    k_blob<512, kSortCap>, then k_fit_quads
  blob_item         n >= 64 takes the register theta sorts (32 buckets up to 64 points, the
                    power of two nb with n/2 <= nb < n above: 4096 points are the last with
                    2048 buckets, where team_reg_bucket_sort_kv's nb / 2 > KEYS / 4 is just
                    false for the 256-thread teams), a bucket of more than 512 keys the
                    bitonic sort; n == CAP fills the sort's array (512, 1024, 4096 and, as the
                    largest geometry admits 2 (W + H) = 8176, 8176 of kSortCap = 8192)
  max_cluster       a pair of 2 (W + H) points is kept, one of a point more dropped

blob_size_cases.py builds frames whose pairs have exactly the asked count: N - 1 (where the
cut is also a sort's capacity), N and N + 1 for every cut, at the smallest geometry that
admits them, plus thin bars (theta crowds into few buckets), two mosaics of 14 blobs (both
sides of every cut up to 1025, ascending and descending) and a crowd of 40 blobs of 64 and
40 of 65 points beside 16 dropped ones.

CPU half (no marker): the oracle alone pins that every count is hit exactly, what is kept and
dropped, each bar's fullest theta bucket, the mosaics' and the crowd's blobs.  GPU half: every
frame through latency mode (plain, with the kernel timer on k_blob, with stage profiling) and
through a max_batch = 8 detector (in a call of its own, with seven blank frames, and all
frames of a geometry in calls of 8), every stage bit-equal to the oracle's, and the points the
small-blob and large-blob kernels report (at_batch_stats [3] and [4]) equal to the kept
blobs' on their side of the cut between the one-wave kernels and the teams: 1024 in a call
of 8 frames, 512 in every other.

Not reached:
  * a bucket of more than 512 keys in a blob of up to 1,024 points (wave_bucket_sort_kv's
    fallback): such a blob has 513 or more points, so 512 buckets, and more than half of its
    points would have to lie within 0.7 degrees as seen from the centre of its extents, while
    a closed outline has points on both sides of it; bars of under 1,024 points stay under
    200.  The team sorts' fallback is reached (bars of 3,764 and 4,004 points with 703 and 763
    keys in one bucket).
  * dropped blobs of an odd count in the crowd: the only blobs SelectBlobs drops at 64 points
    are those of the reversed border direction (a sliver's extents are never under
    min_tag_width at 64 points), white holes in a dark slab; white is 8-connected, so the
    lone corner pixel that takes a point from a dark shape joins a white one.  The dropped
    ones have 64 and 68 points, one count in each of the two classes.
"""
import numpy as np
import pytest

import blob_size_cases as bc
from parity_util import compare_detections, compare_frame

GRAY8 = 2
CUTS = (64, 128, 256, 512, 1024, 2048)  # size_class()
CAPS = (512, 1024, 4096)                # sort capacities a blob can fill exactly
WIDE_BLOB_MAX_BATCH = 8                 # kWideBlobMaxBatch: frames of a call from which the throughput launches run

# (W, H) -> exact counts; a count above 2 (W + H) is a dropped pair
COUNTS = {
    (640, 480): [63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 258, 511, 512, 513, 514,
                 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2240, 2241],
    (1280, 768): [4095, 4096, 4097],      # max_cluster == 4096: the cap4k / lat_fused side
    (1288, 768): [4096, 4097, 4112, 4113],  # the first geometry on the kSortCap side
    (1920, 1080): [4096, 4097, 5999, 6000, 6001],
    (2048, 2040): [8176, 8177],           # the largest geometry accepted
}
# (W, H) -> bars (length, thickness) in decimated pixels, with (n, nb, fullest bucket)
BARS = {
    (1920, 1080): {(940, 1): (3764, 2048, 703), (940, 2): (3768, 2048, 460), (900, 3): (3612, 2048, 380)},
    (2048, 2040): {(1000, 1): (4004, 2048, 763)},
}
MOSAIC_UP = [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1025]
CROWD = [64, 65] * 40
CROWD_HOLES = [64, 68] * 8
EXTRA = {(640, 480): ["mosaic_up", "mosaic_down", "crowd"]}
GEOMETRIES = list(COUNTS)
GEOM_IDS = ["%dx%d" % g for g in GEOMETRIES]


def max_cluster(geom):
    return 2 * (geom[0] + geom[1])


def keys_of(geom):
    return ([("n", n) for n in COUNTS[geom]] + [("bar",) + b for b in BARS.get(geom, {})]
            + [(k,) for k in EXTRA.get(geom, [])])


def build(geom, key):
    W, H = geom
    if key[0] == "n":
        return bc.blob(W, H, key[1])
    if key[0] == "bar":
        return bc.bar(W, H, key[1], key[2])
    if key[0] == "crowd":
        return bc.crowd(W, H, CROWD, CROWD_HOLES)
    if key[0] == "blank":
        return bc.white(W, H)
    return bc.mosaic(W, H, MOSAIC_UP if key[0] == "mosaic_up" else MOSAIC_UP[::-1])


class Ref:
    """A frame and what the oracle made of it (read only)."""

    def __init__(self, oracle_mod, geom, key):
        self.frame = np.ascontiguousarray(build(geom, key))
        self.frame.setflags(write=False)
        self.orc = oracle_mod.Oracle(geom[0], geom[1])
        assert self.orc.detect(self.frame, GRAY8) >= 0
        self.index_points = self.orc.sorted_index_points()
        self.kept = list(bc.blob_counts(self.index_points).values())  # kept blobs' counts, in blob order
        self.detections = self.orc.detections()


_REFS = {}


def ref(oracle_mod, geom, key):
    if (geom, key) not in _REFS:
        _REFS[(geom, key)] = Ref(oracle_mod, geom, key)
    return _REFS[(geom, key)]


def pair_counts(orc):
    """Points of every pair, kept or not, ascending."""
    return sorted(np.unique(orc.sorted_points() >> np.uint64(24), return_counts=True)[1].tolist())


# ---- CPU half -----------------------------------------------------------------------

def test_case_list_holds_every_cut_and_capacity():
    counts = {n for g in GEOMETRIES for n in COUNTS[g] if n <= max_cluster(g)}
    for cut in CUTS:
        assert {cut, cut + 1} <= counts
    assert 63 in counts  # blob_item's n >= 64
    for cap in CAPS:
        assert {cap - 1, cap, cap + 1} <= counts
    assert {4096, 4097} <= set(COUNTS[(1288, 768)]) and 4096 < max_cluster((1288, 768))  # nlo = 4096
    for g in GEOMETRIES:
        assert {max_cluster(g), max_cluster(g) + 1} <= set(COUNTS[g])
    assert max_cluster(GEOMETRIES[-1]) == 8176  # of kSortCap = 8192 (2048 x 2048 has too many pixels)


@pytest.mark.parametrize("geom,n", [(g, n) for g in GEOMETRIES for n in COUNTS[g]],
                         ids=["%dx%d-%d" % (g + (n,)) for g in GEOMETRIES for n in COUNTS[g]])
def test_oracle_counts_are_exact(oracle_mod, geom, n):
    """One pair of exactly n points; kept whole up to max_cluster, dropped above."""
    r = ref(oracle_mod, geom, ("n", n))
    assert r.orc.status() == 0 and r.orc.num_pairs() == 1
    assert pair_counts(r.orc) == [n]
    assert r.kept == ([n] if n <= max_cluster(geom) else [])
    if n > max_cluster(geom):
        assert r.index_points.size == 0 and r.orc.fitquads() == []
    if n % 4 == 0 and n <= max_cluster(geom):
        assert len(r.orc.quads()) == 1  # an untouched rectangle (or one with dents) is a quad


def test_oracle_bucket_counts_at_4096(oracle_mod):
    """4096 points are the last with 2048 theta buckets, 4097 the first with 4096."""
    fills = {n: bc.bucket_fill(ref(oracle_mod, (1288, 768), ("n", n)).index_points) for n in (4096, 4097)}
    assert [f[0][:2] for f in fills.values()] == [(4096, 2048), (4097, 4096)]
    n, nb, mx = bc.bucket_fill(ref(oracle_mod, (2048, 2040), ("n", 8176)).index_points)[0]
    assert (n, nb) == (8176, 4096) and mx <= bc.REG_SORT_MAX_BUCKET
    for n, nb in ((63, 32), (64, 32), (65, 64), (512, 256), (513, 512), (1024, 512), (1025, 1024)):
        assert bc.bucket_fill(ref(oracle_mod, (640, 480), ("n", n)).index_points)[0][:2] == (n, nb)


@pytest.mark.parametrize("geom,bar", [(g, b) for g in BARS for b in BARS[g]],
                         ids=["%dx%d-%dx%d" % (g + b) for g in BARS for b in BARS[g]])
def test_oracle_bars(oracle_mod, geom, bar):
    """Each bar's fullest theta bucket: the one-pixel bars are over kRegSortMaxBucket (the
    bitonic fallback of the team sorts), the thicker ones under it."""
    r = ref(oracle_mod, geom, ("bar",) + bar)
    assert r.orc.status() == 0 and r.orc.num_pairs() == 1
    fill = bc.bucket_fill(r.index_points)
    print(geom, bar, fill)
    assert fill == [BARS[geom][bar]]
    assert (fill[0][2] > bc.REG_SORT_MAX_BUCKET) == (bar[1] == 1)
    assert 1024 < fill[0][0] <= 4096  # the 256-thread teams in throughput mode


def test_oracle_mosaics(oracle_mod):
    for key, want in (("mosaic_up", MOSAIC_UP), ("mosaic_down", MOSAIC_UP[::-1])):
        r = ref(oracle_mod, (640, 480), (key,))
        assert r.orc.status() == 0 and r.orc.num_pairs() == 14
        assert r.kept == want  # blob order is placement order
    for cut in CUTS[:-1]:
        assert {cut, cut + 1} <= set(MOSAIC_UP)


def test_oracle_crowd(oracle_mod):
    """40 kept blobs of 64 points and 40 of 65, eight dropped ones of 64 and eight of 68 (the
    reversed border direction), and the slab that holds those."""
    r = ref(oracle_mod, (640, 480), ("crowd",))
    assert r.orc.status() == 0 and r.orc.num_pairs() == 97
    pairs = pair_counts(r.orc)
    assert pairs[:96] == [64] * 48 + [65] * 40 + [68] * 8 and pairs[96] > 1024
    assert sorted(r.kept) == [64] * 40 + [65] * 40 + pairs[96:]


# ---- GPU half -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    import ros_vision_amd as rva
    rva.GpuDetector.DEBUG_TAPS = True  # the IndexPoint tap compare_frame reads
    yield rva
    rva.GpuDetector.DEBUG_TAPS = False


def snapshot(det, idx, dets):
    """Everything the blob stage and the decode left for frame idx, as comparable values."""
    quads = [(q["blob_index"], q["valid"], q["accepted"], tuple(q["indices"]), q["corners"].tobytes())
             for q in det.copy_quads(idx)]
    return (quads, det.copy_blob_points(idx).tobytes(),
            [(d.id, d.hamming, d.decision_margin, d.H.tobytes(), d.p.tobytes()) for d in dets])


def run(gpu, det, refs, what, check=None):
    """One call with the frames of refs: the frames in check (default:
    all) against their oracles, the call's small-blob and large-blob point totals against the
    kept blobs' of all frames by the call's cut.  Returns the checked frames' snapshots."""
    if det.max_batch == 1:
        res = [det.detect(refs[0].frame, gpu.AT_FMT_GRAY8)]
    else:
        res = det.detect_batch([r.frame for r in refs], gpu.AT_FMT_GRAY8)
    out = []
    for c in range(len(refs)) if check is None else check:
        r = refs[c]
        assert det.frame_status(c) == r.orc.status(), (what, c)
        assert compare_frame(det, r.orc, frame_idx=c) == [], (what, c)
        assert compare_detections(res[c], r.detections) == [], (what, c)
        out.append(snapshot(det, c, res[c]))
    kept = [n for r in refs for n in r.kept]
    cut = 1024 if len(refs) >= WIDE_BLOB_MAX_BATCH else 512  # the one-wave kernels' share
    st = det.batch_stats()
    assert (st["small_blob_points"], st["large_blob_points"]) == (
        sum(n for n in kept if n <= cut), sum(n for n in kept if n > cut)), (what, kept)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMETRIES, ids=GEOM_IDS)
def test_latency_mode(gpu, oracle_mod, geom):
    """max_batch = 1: k_blob_lat (max_cluster <= 4096) or k_extents + k_blob<512, kSortCap> +
    k_blob_small<true>; then the kernels timed apart, by the kernel timer and by stage
    profiling (k_blob<512, 4096, true> + k_blob_small<true> up to 4096): the same results."""
    det = gpu.GpuDetector(geom[0], geom[1], max_batch=1)
    try:
        plain = {}
        for key in keys_of(geom):
            plain[key] = run(gpu, det, [ref(oracle_mod, geom, key)], key)
        det.set_kernel_timer("k_blob")
        for key in keys_of(geom):
            assert run(gpu, det, [ref(oracle_mod, geom, key)], ("timer",) + key) == plain[key], key
        det.set_kernel_timer(None)
        det.set_profiling(True)
        for key in keys_of(geom):
            assert run(gpu, det, [ref(oracle_mod, geom, key)], ("profiling",) + key) == plain[key], key
        det.set_profiling(False)
    finally:
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMETRIES, ids=GEOM_IDS)
def test_throughput_mode(gpu, oracle_mod, geom):
    """max_batch = 8.  A call of eight frames: k_extents, k_blob<256, 4096>,
    k_blob_small<false, 1024, 3, 9>, k_blob<AT_BIG_NT, kSortCap> (max_cluster > 4096),
    k_blob_small<false>, k_fit_quads; every frame with seven blank ones (its blobs alone in the
    work lists), then the geometry's frames together, eight to a call (the last call filled
    up with blank frames).  A call of one frame: k_extents, k_blob<512, 4096> or
    k_blob<512, kSortCap> for every blob over 512 points, k_blob_small<false>, k_fit_quads."""
    det = gpu.GpuDetector(geom[0], geom[1], max_batch=8)
    try:
        keys = keys_of(geom)
        blank = ref(oracle_mod, geom, ("blank",))
        assert blank.kept == [] and blank.orc.num_pairs() == 0
        fill = [blank] * (WIDE_BLOB_MAX_BATCH - 1)
        one = {key: run(gpu, det, [ref(oracle_mod, geom, key)], ("one",) + key)[0] for key in keys}
        for key in keys:  # (the first and the last frame of the call compared)
            got = run(gpu, det, [ref(oracle_mod, geom, key)] + fill, ("alone",) + key, check=(0, 7))
            assert got[0] == one[key], key
        for k0 in range(0, len(keys), 8):
            part = keys[k0:k0 + 8]
            refs = [ref(oracle_mod, geom, key) for key in part]
            got = run(gpu, det, refs + fill[:8 - len(refs)], ("together", k0))
            assert got[:len(part)] == [one[key] for key in part], k0
    finally:
        det.close()
