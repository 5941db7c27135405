"""bench.py's command line on the CPU: the headline defaults the GPU parity test of the
headline configuration imports (tests/test_stream_parity.py), and the helpers the
roofline and multi-GPU legs use."""
import bench


def test_headline_defaults():
    a = bench.parse([])
    assert (a.width, a.height, a.tags, a.pool) == (1280, 720, 15, 64)
    assert a.batch >= 1 and a.instances >= 1
    # at least 4 copies and two batches' worth of frames resident in HBM
    c = bench.pool_copies(a)
    assert c >= 4 and a.pool * c >= 2 * a.batch
    assert bench.pool_copies(bench.parse(["--hbm-copies", "2"])) == 2
    assert bench.DOMINANT in ("k_thr_ccl", "k_boundary", "k_blob_small", "k_blob", "k_extents", "k_decode")


def test_plain_run_is_the_headline_only():
    """Without --full every leg beside the headline is off, whatever its own option says;
    the headline's own options (steps, warm-up, batch, instances, kernel timer) stay."""
    a = bench.parse(["--steps", "7", "--warmup", "2", "--latency-frames", "500"])
    assert not a.full and a.dump_outputs is None
    bench.headline_only(a)
    assert a.no_stage_profile and a.no_cpu_baseline
    assert (a.latency_frames, a.c3_latency_iters, a.host_ingest_steps, a.node_path_calls, a.isolated_batches,
            a.scatter_leg_steps) == (0, 0, 0, 0, 0, 0)
    assert (a.steps, a.warmup, a.batch, a.instances, a.no_kernel_timer) == (7, 2, 192, 4, False)
    f = bench.parse(["--full", "--dump-outputs", "out"])
    assert f.full and f.dump_outputs == "out" and f.latency_frames == 1000 and not f.no_cpu_baseline


def test_last_step_outputs_layout(tmp_path):
    """--dump-outputs: counts / detections / poses of the batch in a detector's output
    buffer, as float64 rows led by the frame index; written as DIR/<name>.npy."""
    import numpy as np

    from ros_vision_amd.detector import Detection, Pose

    class Det:
        def __init__(self):
            self.res = [[Detection(7, 0, 55.5, np.arange(9.).reshape(3, 3), np.array([1.5, 2.5]),
                                   np.arange(8.).reshape(4, 2) + 100)], [],
                        [Detection(3, 1, 9.25, np.eye(3), np.zeros(2), np.ones((4, 2))),
                         Detection(9, 2, 1.0, 2 * np.eye(3), np.ones(2), np.zeros((4, 2)))]]

        def results(self):
            return self.res

        def poses(self, f):
            return [Pose(d.id, np.eye(3) * (f + 1), np.array([0.1, 0.2, 0.3]), 1e-6) for d in self.res[f]]

    out = bench.last_step_outputs(Det(), 3)
    assert all(a.dtype == np.float64 for a in out.values())
    assert out["counts"].tolist() == [1, 0, 2]
    assert out["detections"].shape == (3, 23) and out["poses"].shape == (3, 15)
    assert out["detections"][:, :3].tolist() == [[0, 7, 0], [2, 3, 1], [2, 9, 2]]
    assert out["detections"][0, 3:].tolist() == [55.5] + list(range(9)) + [1.5, 2.5] + list(range(100, 108))
    assert out["poses"][:, :2].tolist() == [[0, 7], [2, 3], [2, 9]]
    assert out["poses"][1, 2:].tolist() == (3 * np.eye(3)).ravel().tolist() + [0.1, 0.2, 0.3, 1e-6]
    # a batch with no detection keeps the column counts
    empty = bench.last_step_outputs(type("E", (), {"results": lambda s: [[]], "poses": lambda s, f: []})(), 1)
    assert empty["detections"].shape == (0, 23) and empty["poses"].shape == (0, 15)
    bench.dump_outputs(str(tmp_path / "d"), out)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["counts.npy", "detections.npy", "poses.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "detections.npy"), out["detections"])
    bench.dump_outputs(str(tmp_path / "d2"), out, rank=1, world=2)
    assert (tmp_path / "d2" / "poses_rank1.npy").exists()


def test_isolated_table_orders_by_span():
    st = {"frames": 2, "boundary_points": 1000, "ccl_listed_roots": 10, "small_blob_points": 500,
          "large_blob_points": 100}
    iso = {"k_thr_ccl": (0.2, 0.25, 10, st), "k_boundary": (0.3, 0.31, 10, st), "k_pairs": (0.01, 0.02, 10, st)}
    rows = bench.isolated_table(iso, 1280, 720)
    assert [r["kernel"] for r in rows] == ["k_boundary", "k_thr_ccl", "k_pairs"]
    kb = bench.kernel_algorithmic_bytes("k_boundary", st, 1280, 720)
    assert rows[0]["algorithmic_bytes_per_launch"] == kb
    assert abs(rows[0]["achieved"] - kb / 0.3e-3 / 1e9) < 1e-3
    assert rows[2]["frac"] is None  # (no algorithmic byte model for k_pairs)


def test_dominant_matches_committed_ablation():
    """DOMINANT is the top stage of the stage-cut ablation committed
    at bench.ABLATION (marginal ms per step of each stage at the bench configuration)."""
    marg, top = bench.ablation_marginals()
    assert top == bench.DOMINANT, marg
    assert set(marg) >= {"k_pre", "k_thr_ccl", "k_boundary", "k_blob_small", "k_blob", "k_decode"}
    assert all(v > -0.05 for v in marg.values()), marg


def test_ablation_marginals_parse(tmp_path):
    p = tmp_path / "abl.txt"
    p.write_text("pipe_stop=0 100 2.0 15\npipe_stop=1 9 0.1 0\npipe_stop=2 8 0.5 0\npipe_stop=3 7 0.6 0\n"
                 "pipe_stop=5 6 1.2 0\n")
    marg, top = bench.ablation_marginals(str(p))
    assert marg == {"k_pre": 0.1, "k_thr_ccl": 0.4, "k_ccl_merge": 0.1, "k_boundary": 0.6}
    assert top == "k_boundary"
