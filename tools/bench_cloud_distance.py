"""Times the cross-cloud distances of csrc/cloud_distance.hip on the device (device events, one warm-up, median of the repeats) between two
synthetic glacier fronts of `--points` points each (default 2 M): the front of tests/ball_cases.py scaled up to 200 m x 400 m in a world
frame, the second epoch sampled anew and displaced by 0.3 m across the front:
  - the cloud-to-cloud distance (`cloud_to_cloud_distance`, device tensors in and out: binning, sort, ranges, gather, kernel, sqrt, split);
  - the cross searches with k = 1 and k = 8: the whole call (`knn_cross`) and the gather + kernel alone on a target binned beforehand;
  - M3C2 with 100 k core points and with all points as core points, normal_scale 2 m, search_scale 1 m, search_depth 5 m and 20 m: the
    whole call on clouds binned beforehand (normals, two cylinder passes, finish), and the cylinder pass over the second epoch alone;
  - the distribution of d_steps of that cylinder pass (mean, median, 99th percentile, maximum, whole-cloud scans) and of d_rings of the
    searches, and the mean number of points per cylinder.
Before timing, the sums of `--check` cylinders and the neighbours of `--check` queries are compared with the restatement over the whole
cloud (tests/cloud_distance_oracle.py: Python integers, bits).
What bounds the cylinder kernel (row lookups, rejected candidates of a long oblique box, or memory) is NOT measured here: that takes a
counter run of its own.

    python tools/bench_cloud_distance.py [--points 2000000] [--repeats 5] [--out profiles/r17_cloud_distance_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_pointcloud import timed  # noqa: E402

SIZE = (200.0, 400.0)
ORIGIN = (416000.0, 5091000.0, 1800.0)
SHIFT = (0.3, 0.0, 0.0)
NORMAL_SCALE, SEARCH_SCALE, DEPTHS, CORE = 2.0, 1.0, (5.0, 20.0), 100_000


def distribution(t):
    a = t.abs().double()
    q = np.quantile(a.cpu().numpy(), [0.5, 0.99])
    return {"mean": round(float(a.mean()), 2), "median": float(q[0]), "p99": float(q[1]), "max": int(a.max()), "negative": int((t < 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_cloud_distance_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.points >= 1000
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_cloud_distance.py needs a HIP device: there is nothing to time without one")
    import ball_cases as BC
    import cloud_distance_oracle as O
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.post_processing import cloud_to_cloud_distance, m3c2
    from icepy4d_amd.utils import point_cloud_filters as F
    eng = Engine(0)
    dev, st = eng.device, eng.stream_ptr()
    n = a.points
    host1 = BC.front(n, seed=51, size=SIZE, origin=ORIGIN)
    host2 = BC.front(n, seed=52, size=SIZE, origin=ORIGIN) + np.asarray(SHIFT)
    c1, c2 = torch.from_numpy(host1).to(dev), torch.from_numpy(host2).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "points": n, "repeats": a.repeats,
           "clouds": f"tests/ball_cases.py front, size {SIZE}, seeds 51 / 52, the second displaced by {SHIFT}",
           "clock": "device events around the calls, one warm-up, median of the repeats",
           "unmeasured": "what bounds im_cyl_stats (row lookups, rejected candidates of a long oblique box, memory): no counter run was made"}
    ok = True

    # ---- cloud-to-cloud and the cross searches
    out = {}
    out["c2c_whole_ms"], out["c2c_whole_ms_all"] = timed(torch, lambda: cloud_to_cloud_distance(c1, c2, engine=eng), a.repeats)
    d = cloud_to_cloud_distance(c1, c2, engine=eng).distance
    out["c2c_mean_distance"], out["c2c_points_per_s"] = round(float(d.mean()), 4), round(n / (out["c2c_whole_ms"] * 1e-3))
    for k in (1, 8):
        whole_ms, whole_all = timed(torch, lambda: F.knn_cross(c1, c2, k, engine=eng), a.repeats)
        s = F.choose_cell_size(eng, c2, *F._bounds(c2), k)
        b = F.bin_cloud(c2, s, engine=eng)
        order = F.query_order(eng, c1, b)
        idx, d2 = torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.float64, device=dev)
        rings = torch.empty(n, dtype=torch.int32, device=dev)

        def kernel(with_rings=False):
            eng.ctx.call("im_knn_cross", *F._target_args(b), ptr(c1), ptr(order), n, k, float("inf"), None, ptr(idx), ptr(d2),
                         ptr(rings) if with_rings else None, st)

        kernel(True)
        kernel_ms, kernel_all = timed(torch, kernel, a.repeats)
        sel = np.random.default_rng(k).integers(0, n, a.check)
        oidx, od2, _ = O.knn_cross(host1[sel], host2, k)
        d_sel = torch.from_numpy(sel).to(dev)
        equal = bool(np.array_equal(idx[d_sel].cpu().numpy(), oidx) and np.array_equal(d2[d_sel].cpu().numpy().view(np.uint64), od2.view(np.uint64)))
        ok = ok and equal
        out[f"knn_cross_k{k}"] = {"whole_ms": whole_ms, "whole_ms_all": whole_all, "kernel_ms": kernel_ms, "kernel_ms_all": kernel_all,
                                  "cell_size": b.cell_size, "dims": b.dims, "rings": distribution(rings), "checked_queries": int(a.check),
                                  "equal_to_the_restatement": equal}
        print(f"knn_cross k = {k}: whole {whole_ms:.2f} ms, gather + kernel {kernel_ms:.2f} ms, s = {b.cell_size:.4g}, equal {equal}", flush=True)
    res["searches"] = out
    print(f"C2C: whole {out['c2c_whole_ms']:.2f} ms, mean distance {out['c2c_mean_distance']} m", flush=True)

    # ---- M3C2
    b1, b2 = F.bin_cloud(c1, SEARCH_SCALE / 2.0, engine=eng), F.bin_cloud(c2, SEARCH_SCALE / 2.0, engine=eng)
    res["m3c2"] = {"normal_scale": NORMAL_SCALE, "search_scale": SEARCH_SCALE, "cell_size": b1.cell_size, "dims": b1.dims, "runs": {}}
    cores = {f"{CORE // 1000}k": c1[torch.from_numpy(np.random.default_rng(3).choice(n, min(CORE, n), replace=False)).to(dev)].contiguous(), "all": c1}
    for tag, core in cores.items():
        m = core.shape[0]
        for depth in DEPTHS:
            kw = dict(core_points=core, normal_scale=NORMAL_SCALE, search_scale=SEARCH_SCALE, search_depth=depth, registration_error=0.02, engine=eng)
            r = m3c2(b1, b2, **kw)
            nrm = r.normals.contiguous()
            order = F.query_order(eng, core, b2)
            count, steps = torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev)
            sums = torch.empty((m, 2), dtype=torch.int64, device=dev)

            def cyl(with_steps=False):
                eng.ctx.call("im_cyl_stats", *F._target_args(b2), ptr(core), ptr(nrm), ptr(order), m, SEARCH_SCALE / 2.0, depth, ptr(count), ptr(sums),
                             None, None, ptr(steps) if with_steps else None, st)

            cyl(True)
            run = {"core_points": m, "search_depth": depth}
            run["whole_ms"], run["whole_ms_all"] = timed(torch, lambda: m3c2(b1, b2, **kw), a.repeats)
            run["cylinder_pass_ms"], run["cylinder_pass_ms_all"] = timed(torch, cyl, a.repeats)
            run["core_points_per_s"] = round(m / (run["whole_ms"] * 1e-3))
            run["steps"] = distribution(steps)
            run["mean_points_per_cylinder"] = round(float(count.double().mean()), 2)
            run["with_a_distance"], run["significant"] = int((~torch.isnan(r.distance)).sum()), int(r.significant.sum())
            sig = r.distance[r.significant]
            run["mean_significant_distance"] = round(float(sig.mean()), 4) if len(sig) else None
            sel = np.random.default_rng(int(depth)).integers(0, m, a.check)
            hq, hn = core[torch.from_numpy(sel).to(dev)].cpu().numpy(), nrm[torch.from_numpy(sel).to(dev)].cpu().numpy()
            hc, hs = count.cpu().numpy()[sel], sums.cpu().numpy()[sel]
            equal = all(O.cyl_sums(host2, hq[j], hn[j], SEARCH_SCALE / 2.0, depth) == (int(hc[j]), int(hs[j, 0]), int(hs[j, 1])) for j in range(len(sel)))
            run["checked_cylinders"], run["equal_to_the_restatement"] = int(a.check), bool(equal)
            ok = ok and equal
            res["m3c2"]["runs"][f"core_{tag}_depth_{depth:g}"] = run
            print(f"M3C2 {tag} core points, depth {depth:g} m: whole {run['whole_ms']:.2f} ms, cylinder pass {run['cylinder_pass_ms']:.2f} ms, "
                  f"steps mean {run['steps']['mean']} p99 {run['steps']['p99']} max {run['steps']['max']} scans {run['steps']['negative']}, "
                  f"{run['mean_points_per_cylinder']} points per cylinder, equal {equal}", flush=True)
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
