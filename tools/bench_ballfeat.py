"""Times the ball features of csrc/ballfeat.hip on the device (device events, one warm-up, median of the repeats) on the synthetic
glacier front of tools/bench_pointcloud.py (`--points`, default 2 M, plus 0.5 % outliers), with the two calls of the reference's
`scripts/pcd_postprocessing/top_border.py`:
  - Linearity over balls of 2.0 m and Verticality over balls of 0.15 m: the whole call (`ball_features` on a device tensor: bounds,
    binning, torch's stable sort, cell ranges, gather, kernel) and the kernel with its gather alone (`im_ball_features` on a cloud binned
    beforehand);
  - both through `detect_border_by_geometry` end to end (host array in, border cloud out; wall clock);
  - the mean and the largest number of neighbours per ball, the mean steps per query and the number of whole-cloud scans.
Before timing, the sums and the feature of `--check` random points are compared with the restatement over the whole cloud
(tests/ball_oracle.py: Python integers, bits).
For scale only, `scipy.spatial.cKDTree.query_ball_point(workers=16)` plus numpy's covariance and eigvalsh on the host for `--host-sample`
queries of the same cloud, extrapolated to all points: a ratio that is reported, not asserted.

    python tools/bench_ballfeat.py [--points 2000000] [--repeats 5] [--no-kdtree] [--out profiles/r14_ballfeat_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_pointcloud import glacier, timed  # noqa: E402

CALLS = (("Linearity", 2.0), ("Verticality", 0.15))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check", type=int, default=16)
    ap.add_argument("--host-sample", type=int, default=20000)
    ap.add_argument("--no-kdtree", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_ballfeat_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.points >= 1000
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ballfeat.py needs a HIP device: there is nothing to time without one")
    import ball_oracle as B
    from icepy4d_amd import top_border as T
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.utils import point_cloud_filters as F
    eng = Engine(0)
    dev, st = eng.device, eng.stream_ptr()
    n = a.points
    host = glacier(n)
    pts = torch.from_numpy(host).to(dev)
    lo, hi = host.min(0), host.max(0)
    res = {"device": torch.cuda.get_device_name(0), "points": n, "repeats": a.repeats, "cloud": "glacier (tools/bench_pointcloud.py)",
           "clock": "device events around the calls, one warm-up, median of the repeats; detect_border_by_geometry and the host by wall clock",
           "calls": {}}
    ok = True
    for feature, r in CALLS:
        kind = np.array([F.BALL_KINDS[feature]], np.int32)
        s, dims, grid, perm, start = F._binned(eng, pts, lo, hi, r / 2.0)
        feat = torch.empty((n, 1), dtype=torch.float64, device=dev)
        count, steps = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        sums = torch.empty((n, 10), dtype=torch.int64, device=dev)

        def kernel(with_stats=False):
            eng.ctx.call("im_ball_features", ptr(pts), ptr(perm), ptr(start), n, grid.ctypes.data, dims[0], dims[1], dims[2], r, kind.ctypes.data, 1,
                         ptr(count) if with_stats else None, ptr(sums) if with_stats else None, None, None, ptr(feat),
                         ptr(steps) if with_stats else None, st)

        def whole():
            return F.ball_features(pts, r, features=(feature,), engine=eng)

        kernel(True)
        out = {"radius": r, "cell_size": s, "dims": dims}
        out["kernel_ms"], out["kernel_ms_all"] = timed(torch, kernel, a.repeats)
        out["whole_ms"], out["whole_ms_all"] = timed(torch, whole, a.repeats)
        out["points_per_s"] = round(n / (out["whole_ms"] * 1e-3))
        out["mean_neighbours"] = round(float(count.double().mean()), 2)
        out["max_neighbours"] = int(count.max())
        out["balls_without_a_feature"] = int(torch.isnan(feat).sum())
        out["mean_steps"] = round(float(steps.abs().double().mean()), 2)
        out["whole_cloud_scans"] = int((steps < 0).sum())
        out["candidates_per_s"] = round(float(count.double().sum()) / (out["kernel_ms"] * 1e-3))
        # the restatement over the whole cloud for a few points: the production size reaches what the small shapes of the suite do not
        sel = np.random.default_rng(int(r * 100)).integers(0, n, a.check)
        d_sel = torch.from_numpy(sel).to(dev)
        hs, hf = sums[d_sel].cpu().numpy(), feat[d_sel, 0].cpu().numpy()
        equal = True
        for j, q in enumerate(sel):
            S = np.array([B.python_int_sums(host, int(q), r)], np.int64)
            eig, e3 = B.finish(S, r)
            want = B.features(eig, e3, S[:, 0])[feature]
            equal = equal and np.array_equal(S[0], hs[j]) and want.view(np.uint64)[0] == hf[j:j + 1].view(np.uint64)[0]
        out["checked_points"], out["equal_to_the_restatement"] = int(a.check), bool(equal)
        ok = ok and equal
        if not a.no_kdtree:
            from scipy.spatial import cKDTree
            t0 = time.perf_counter()
            tree = cKDTree(host)
            t1 = time.perf_counter()
            m = min(a.host_sample, n)
            qs = np.random.default_rng(1).integers(0, n, m)
            balls = tree.query_ball_point(host[qs], r, workers=16)
            t2 = time.perf_counter()
            for q, nb in zip(qs, balls):
                if len(nb) >= 3:
                    np.linalg.eigvalsh(np.cov((host[nb] - host[q]).T, bias=True))
            t3 = time.perf_counter()
            out["host_ckdtree_build_s"] = round(t1 - t0, 3)
            out["host_sample_queries"] = int(m)
            out["host_query_ball_point_s_16_workers_sample"] = round(t2 - t1, 3)
            out["host_numpy_cov_eigvalsh_s_sample"] = round(t3 - t2, 3)
            out["host_extrapolated_s_all_points"] = round((t1 - t0) + (t3 - t1) * n / m, 1)
            out["host_over_device_extrapolated"] = round(out["host_extrapolated_s_all_points"] / (out["whole_ms"] * 1e-3), 1)
        res["calls"][f"{feature}_r{r}"] = out
        print(f"{feature} r = {r}: whole {out['whole_ms']:.2f} ms ({out['points_per_s'] / 1e6:.2f} M points/s), kernel {out['kernel_ms']:.2f} ms, "
              f"s = {s:.4g}, neighbours mean {out['mean_neighbours']} max {out['max_neighbours']}, scans {out['whole_cloud_scans']}, equal {equal}",
              flush=True)
    T.detect_border_by_geometry(host, engine=eng)
    torch.cuda.synchronize()
    secs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        border = T.detect_border_by_geometry(host, engine=eng)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    res["detect_border_by_geometry"] = {"end_to_end_ms": round(float(np.median(secs)) * 1e3, 2), "border_points": int(len(border)),
                                        "note": "host array in, border cloud out: two uploads, two feature calls, downloads, host percentiles"}
    print(f"detect_border_by_geometry: {np.median(secs) * 1e3:.1f} ms end to end, {len(border)} border points", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not ok:
        sys.exit("the device output differs from the restatement at the production size")


if __name__ == "__main__":
    main()
