"""Full-size runs of the BASELINE.json configurations: parity against the oracle where it finishes in seconds
(config 2: 1080p, 4096 keypoints) and size-independent properties where it does not (config 5: 12 MP, 16384
keypoints, SuperGlue + Sinkhorn): determinism, mutual consistency of the match tables, Sinkhorn marginals."""
import numpy as np
import pytest
import torch

from icepy4d_amd import synthetic

pytestmark = pytest.mark.gpu

SP_SD = synthetic.superpoint_state_dict(0)


def mutual_consistency(m0, m1):
    i = np.where(m0 > -1)[0]
    assert (m0[i] < len(m1)).all() and np.array_equal(m1[m0[i]], i)
    j = np.where(m1 > -1)[0]
    assert np.array_equal(m0[m1[j]], j)


def test_config2_full_size_determinism_and_geometry():
    """1080 x 1920, 4096 keypoints, SuperPoint + LightGlue: two runs bit-identical, match tables mutually consistent, matches
    follow the true translation. (Parity against the oracle at this size: test_gpu_parity.py, exact or margin-explained.)"""
    from icepy4d_amd.engine import Engine
    lg_sd = synthetic.lightglue_state_dict(0, "passthrough")
    img0, img1 = synthetic.translated_pair(0, 1080, 1920, 40, 8)
    e = Engine(0)
    e.load_state_dict("superpoint", SP_SD)
    e.load_state_dict("lightglue", lg_sd)
    e.reserve(1080, 1920, 2, 4096)
    pair = torch.from_numpy(np.stack([img0, img1])).cuda()
    outs = []
    for _ in range(2):
        e.superpoint(pair, 4, 0.0005, 4, 4096)
        e.lightglue((1920, 1080), (1920, 1080))
        torch.cuda.synchronize()
        k0, d0, s0 = e.features_to_host(0)
        k1, d1, s1 = e.features_to_host(1)
        outs.append((k0, d0, s0, k1, d1, s1, e.matches_to_host(len(k0), len(k1))))
    a, b = outs
    for x, y in zip(a[:6], b[:6]):
        assert np.array_equal(x, y)                      # bit-identical across runs
    assert np.array_equal(a[6]["matches0"], b[6]["matches0"]) and np.array_equal(a[6]["matching_scores0"], b[6]["matching_scores0"])
    k0, d0, s0, k1, d1, s1, out = a
    assert k0.shape == (4096, 2)
    mutual_consistency(out["matches0"], out["matches1"])
    v = out["matches0"] > -1
    assert v.sum() > 500
    d = k1[out["matches0"][v]] - k0[v]
    assert np.mean(np.all(np.abs(d - np.array([40, 8])) < 1.5, 1)) > 0.7   # matches follow the true translation
    e.close()


def test_config5_12mp_superglue_properties():
    """12 MP pair, up to 16384 keypoints, SuperGlue with 20 Sinkhorn iterations (1 GB score matrix)."""
    from icepy4d_amd.engine import Engine
    from icepy4d_amd._lib import ptr, stream_ptr
    H, W, K = 3000, 4000, 16384
    img0, img1 = synthetic.translated_pair(5, H, W, 48, 16)
    e = Engine(0)
    e.load_state_dict("superpoint", SP_SD)
    e.load_state_dict("superglue", synthetic.superglue_state_dict(0, "passthrough"))
    e.reserve(H, W, 2, K)
    pair = torch.from_numpy(np.stack([img0, img1])).cuda()
    res = []
    for _ in range(2):
        e.superpoint(pair, 3, 0.001, 4, K, flavour=1)
        e.superglue((H, W), (H, W), sinkhorn_iterations=20, match_threshold=0.3)
        torch.cuda.synchronize()
        n0, n1 = int(e.n[0]), int(e.n[1])
        res.append((n0, n1, e.kpts[0, :n0].cpu().numpy(), e.scores[0, :n0].cpu().numpy(), e.matches_to_host(n0, n1)))
    (n0, n1, kp, sc, out), (_, _, kp2, sc2, out2) = res
    assert n0 == K and n1 == K
    assert np.array_equal(kp, kp2) and np.array_equal(out["matches0"], out2["matches0"])        # deterministic
    assert (np.diff(sc) <= 0).all()                                                              # top-k sorted descending
    assert kp[:, 0].min() >= 4 and kp[:, 0].max() < W - 4 and kp[:, 1].min() >= 4 and kp[:, 1].max() < H - 4
    assert len({tuple(p) for p in kp}) == K                                                     # no duplicate keypoints
    mutual_consistency(out["matches0"], out["matches1"])
    v = out["matches0"] > -1
    assert v.sum() > 1000 and (out["matching_scores0"][v] > 0.3).all() and (out["matching_scores0"] <= 1.0 + 1e-5).all()
    k1 = e.kpts[1, :n1].cpu().numpy()
    d = k1[out["matches0"][v]] - kp[v]
    assert np.mean(np.all(np.abs(d - np.array([48, 16])) < 1.5, 1)) > 0.7
    # Sinkhorn marginals on a 4096 x 3000 random score block: after the last v-update every column of
    # exp(Z) sums to exp(log_nu - norm), i.e. logsumexp_i Z[i][j] = log_nu[j] - norm = 0 (and log m for the dustbin)
    m, n = 4096, 3000
    g = torch.Generator(device="cuda").manual_seed(1)
    zin = torch.randn(m, n, device="cuda", generator=g) * 2
    zout = torch.empty(m + 1, n + 1, device="cuda")
    e.ctx.call("im_log_optimal_transport", ptr(zin), m, n, n, 1.0, 20, ptr(zout), stream_ptr())
    torch.cuda.synchronize()
    col = torch.logsumexp(zout.double(), 0).cpu().numpy()
    assert np.abs(col[:n]).max() < 1e-4 and abs(col[n] - np.log(m)) < 1e-4
    e.close()


def test_config3_timed_launch_mode_equals_direct_launches_and_the_oracle():
    """BASELINE configs[2] in EXACTLY the launch mode `bench.py` times - `PairPipeline(pairs_per_launch=bench.DEFAULT_PAIRS_PER_LAUNCH,
    n_streams=2, use_graph=True)`: ten pairs share every launch, two launch groups in flight on separate streams, HIP-graph replay -
    at full size (1080 x 1920, 4096 keypoints), over 20 distinct epochs (18 of the sequence's homography-warped pairs, two translated
    pairs with ~1000 matches): the match table is bit-identical to one pair per direct launch on one stream, and two of its
    records decode to the oracle's matches (reference loop: `main_dev.py:60`, matcher call `main_dev.py:115-132`)."""
    import bench
    from icepy4d_amd.engine import Engine
    from icepy4d_amd import sequence as sq
    from margins import assert_same_matches
    from oracle import ref_cpu as o
    lg_sd = synthetic.lightglue_state_dict(0, "passthrough")
    H, W, K = 1080, 1920, 4096
    P = bench.DEFAULT_PAIRS_PER_LAUNCH
    n_st = 2 * P - 2
    pairs_np = [synthetic.stereo_pair(e, H, W) for e in range(n_st)] + [synthetic.translated_pair(s, H, W, 40, 8) for s in (6, 7)]
    pairs = [torch.from_numpy(np.stack(p)).cuda() for p in pairs_np]
    epochs = list(range(100, 100 + len(pairs)))
    checked = (2, len(pairs) - 1)                          # a homography-warped pair and a translated one

    def make_engine():
        e = Engine(0)
        e.load_state_dict("superpoint", SP_SD)
        e.load_state_dict("lightglue", lg_sd)
        return e

    pipe = sq.PairPipeline(make_engine, H, W, K, n_streams=2, use_graph=True, pairs_per_launch=P)
    timed = sq.new_table(len(pairs), K, pipe.device)
    for _ in range(2):                                      # the second pass replays graphs whose buffers hold the first pass
        for row, (p, ep) in enumerate(zip(pairs, epochs)):
            pipe.match_pair(p, ep, timed, row)
        pipe.flush()
        pipe.synchronize()
    timed = timed.cpu()
    pipe.close()

    e = make_engine()
    direct = sq.SequenceMatcher(e, H, W, K, use_graph=False, pairs_per_launch=1)
    ref_tab = sq.new_table(len(pairs), K, e.device)
    kp_dev = {}
    for row, (p, ep) in enumerate(zip(pairs, epochs)):
        direct.match_pair(p, ep, ref_tab, row)
        if row in checked:
            torch.cuda.synchronize()
            kp_dev[row] = (e.features_to_host(0)[0], e.features_to_host(1)[0])
    torch.cuda.synchronize()
    assert torch.equal(timed, ref_tab.cpu())
    assert timed[:, 0].tolist() == epochs and (timed[:, 1] == K).all() and (timed[:, 2] == K).all() and (timed[:, 4] == 9).all()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    for row in checked:
        rec = sq.decode_record(timed[row].numpy(), K)
        F0, F1, m0, mconf, ref = o.match_images_lightglue(*pairs_np[row], SP_SD, lg_sd, max_keypoints=K)
        k0, k1 = kp_dev[row]
        if {tuple(q) for q in k0} == {tuple(q) for q in F0[0]} and {tuple(q) for q in k1} == {tuple(q) for q in F1[0]}:
            assert_same_matches(k0, k1, rec["matches0"], F0[0], F1[0], m0, F0[2], F1[2])
            assert rec["n_matches"] == int((m0 > -1).sum())
        else:    # a keypoint pair flipped at the top-k cut (about one image in 25, margin-explained in test_gpu_parity.py)
            import margins
            ours, theirs = margins.match_pairs(k0, k1, rec["matches0"]), margins.match_pairs(F0[0], F1[0], m0)
            assert len(ours & theirs) >= len(theirs) - 8 and len(ours) <= len(theirs) + 8
        assert rec["n_matches"] > (500 if row == checked[1] else 0)
    e.close()


def run_bench(flags, dump):
    """`python bench.py --gpus 1 *flags --dump-outputs dump` in a fresh process: exit 0 and ONE JSON line on stdout, returned parsed."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", *flags, "--dump-outputs", str(dump)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("flags", [["--steps", "5", "--warmup", "3"], ["--steps", "2", "--warmup", "0"],
                                   ["--steps", "4", "--warmup", "2", "--config", "4", "--pool", "2"],
                                   ["--steps", "10", "--warmup", "2", "SIDE"]])
def test_bench_line_with_odd_step_counts(flags, tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W --full`, with counts that do not fill the launch
    groups (ten pairs each by default): one JSON line with the contract fields, every step recorded, a throughput in the range of the device
    (an odd warm-up once left a parked pair behind and shifted every timed group: 93 instead of 102 pairs/s at K = 20, W = 5).
    `--dump-outputs`: the record of the last timed step (epoch W + K - 1) as float .npy files, consistent in itself."""
    side = "SIDE" in flags                  # the default line's side measurements (configs[2] / configs[4] / one match() call) ride along
    flags = [f for f in flags if f != "SIDE"]
    dump = tmp_path / "outputs"
    d = run_bench([*flags, "--full", "--no-cpu-baseline", *([] if side else ["--no-side-measurements"])], dump)
    assert d["n_gpus"] == 1 and d["steps"] == int(flags[1]) and d["warmup"] == int(flags[3]) and d["unit"] == "pairs/s"
    assert d["config"]["mean_keypoints"] == 4096 and d["roofline"]["bound"] == "mfma" and 0.2 < d["roofline"]["frac"] < 1.0
    assert d["value"] > 5.0, d["value"]      # a sanity bound, not a performance threshold (a cold or shared device is slower)
    assert "all_gather_ms" in d and "traffic_source" in d["roofline"] and "pair_executed_mfma_utilisation" in d
    if side:
        sm = d["side_measurements"]
        c3, c5, mc = sm["config3_distinct_epochs"], sm["config5"], sm["match_call_ms"]
        assert c3["pairs"] >= 60 and c3["epochs_distinct_and_in_order"] and c3["pairs_per_s"] > 5.0
        assert c5["pairs"] == 3 and c5["mean_keypoints"] == 16384 and c5["pairs_per_s"] > 0.5
        assert 0.2 < c5["attention"]["frac_of_peak"] < 1.0 and 1.0 < c5["sinkhorn"]["solve_ms"] < 50.0
        assert 1.0 < mc["median"] < 500.0 and mc["keypoints"] == 4096
        assert sm["other_launch_mode"]["pairs_per_s"] > 5.0 and sm["host_inputs_pairs_per_s"]["pairs_per_s"] > 5.0
    if "--config" in flags:                 # configs[3] on one rank: 98 KB records (keypoints of both images ride along)
        assert "98 KB records" in d["config"]["workload"] and "configs[3]" in d["config"]["workload"]
    out = {p.stem: np.load(p) for p in dump.glob("*.npy")}
    fields = {"epoch", "n_keypoints", "n_matches", "stop_layer", "matches0", "matching_scores0"}
    assert set(out) == (fields | {"keypoints"} if "--config" in flags else fields)
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert out["epoch"].tolist() == [d["warmup"] + d["steps"] - 1] and out["n_keypoints"].tolist() == [[4096, 4096]]
    m0, s0 = out["matches0"][0], out["matching_scores0"][0]
    assert m0.shape == (4096,) and out["n_matches"][0] == (m0 > -1).sum() and ((m0 >= -1) & (m0 < 4096)).all()
    assert np.isfinite(s0).all() and (s0 >= 0).all() and (s0 <= 1 + 1e-5).all() and (s0[m0 > -1] > 0).all()
    if "--config" in flags:
        kp = out["keypoints"]
        assert kp.shape == (1, 2, 4096, 2) and (kp >= 0).all() and (kp[..., 0] < 1920).all() and (kp[..., 1] < 1080).all()


def test_bench_plain_line_is_lean_and_dumps_what_full_dumps(tmp_path):
    """Without --full a run does only what its headline needs: the contract fields, the same timed steps, and none of the runs of
    their own that --full adds (roofline pass, side measurements, CPU baseline). The records of its last timed step equal, bit for
    bit, those of the same run with --full, and so does everything the two lines derive from the timed records."""
    flags = ["--steps", "5", "--warmup", "3"]
    plain = run_bench(flags, tmp_path / "plain")
    full = run_bench([*flags, "--full", "--no-cpu-baseline", "--no-side-measurements"], tmp_path / "full")
    assert plain["full"] is False and full["full"] is True
    for k in ("metric", "unit", "higher_is_better", "dtype", "dtype_note", "n_gpus", "steps", "warmup", "config", "failed_epochs"):
        assert plain[k] == full[k], k
    assert plain["steps"] == 5 and plain["warmup"] == 3 and plain["unit"] == "pairs/s" and plain["dtype"] == "f32"
    assert plain["value"] > 5.0 and abs(plain["value"] - 1e3 / plain["ms_per_step"]) < 1e-6 * plain["value"]
    extras = {"roofline", "roofline_attention", "roofline_convolutions", "kernel_ms_per_pair", "pair_matrix_pipe_time_at_peak_frac",
              "side_measurements", "cpu_baseline"}
    assert not extras & set(plain), extras & set(plain)
    assert full["roofline"]["bound"] == "mfma" and "kernel_ms_per_pair" in full
    a = {p.stem: np.load(p) for p in (tmp_path / "plain").glob("*.npy")}
    b = {p.stem: np.load(p) for p in (tmp_path / "full").glob("*.npy")}
    assert set(a) == set(b) == {"epoch", "n_keypoints", "n_matches", "stop_layer", "matches0", "matching_scores0"}
    for name in a:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name
