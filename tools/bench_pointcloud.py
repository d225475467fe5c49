"""Times the point-cloud neighbourhood kernels of csrc/knn.hip on the device (device events, one warm-up, median of the repeats) on
  - `glacier`: a synthetic glacier-front surface, a noisy height field sampled at `--points` points (default 2 M) plus 0.5 % outliers
    well off the surface, the shape of the dense clouds the reference cleans with SOR and gives normals to;
  - `cube`: the same number of points uniform in a cube, the easy case.
Per cloud and k = 10, 30, 50: the whole search (binning, torch's stable sort, cell ranges, `im_knn_self`) and its parts, points per
second, the share of the time spent in the sort, the chosen cell size and grid, the mean number of rings visited and the number of
searches that ended by a scan of the whole cloud; SOR end to end
(10 / 3.0 and 50 / 1.5, the reference's two call sites, host part included, wall clock) and the normals (radius 1, 30 neighbours).
`--occupancy` sweeps the cell-size heuristic (points per occupied cell as a fraction of k) for k = 30.
Before timing, the neighbours of `--check` random points are compared with a brute force over the whole cloud (bits of d2, indices).
For scale only, `scipy.spatial.cKDTree.query(k, workers=16)` on the same cloud on the host: a ratio that is reported, not asserted.

    python tools/bench_pointcloud.py [--points 2000000] [--repeats 7] [--no-kdtree] [--out profiles/r12_pointcloud_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def glacier(n, seed=12):
    rng = np.random.default_rng(seed)
    n_out = n // 200
    xy = rng.uniform(0.0, 400.0, (n - n_out, 2))
    z = 30.0 * np.sin(xy[:, 0] / 60.0) + 20.0 * np.cos(xy[:, 1] / 45.0) + 8.0 * np.sin(xy[:, 0] / 7.0) * np.cos(xy[:, 1] / 9.0) + rng.normal(0, 0.05, n - n_out)
    out = np.column_stack([rng.uniform(0.0, 400.0, (n_out, 2)), rng.uniform(-150.0, 250.0, n_out)])
    pts = np.concatenate([np.column_stack([xy, z]), out])
    return pts[rng.permutation(n)]


def cube(n, seed=13):
    return np.random.default_rng(seed).uniform(0.0, 100.0, (n, 3))


def timed(torch, fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(m, 3) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--occupancy", type=float, nargs="*", default=[0.125, 0.25, 0.5, 1.0])
    ap.add_argument("--no-kdtree", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_pointcloud_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.points >= 1000
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pointcloud.py needs a HIP device: there is nothing to time without one")
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.utils import point_cloud_filters as F
    eng = Engine(0)
    dev, st = eng.device, eng.stream_ptr()
    n = a.points
    res = {"device": torch.cuda.get_device_name(0), "points": n, "repeats": a.repeats,
           "clock": "device events around the launches, one warm-up, median of the repeats; SOR end to end and cKDTree by wall clock",
           "clouds": {}}
    ok = True
    for cname, host in (("glacier", glacier(n)), ("cube", cube(n))):
        pts = torch.from_numpy(host).to(dev)
        lo, hi = host.min(0), host.max(0)
        entry = {"searches": {}, "occupancy_sweep_k30": {}}
        res["clouds"][cname] = entry

        def parts(k, occupancy=None, radius2=float("inf"), normal=False):
            s = F.fit_cell_size(lo, hi, F.choose_cell_size(eng, pts, lo, hi, k, occupancy), F.max_cells())
            dims = F.grid_dims(lo, hi, s)
            cells = dims[0] * dims[1] * dims[2]
            grid = np.array([lo[0], lo[1], lo[2], s], np.float64)
            key = torch.empty(n, dtype=torch.int64, device=dev)
            start = torch.empty(cells + 1, dtype=torch.int32, device=dev)
            idx = torch.empty((n, k), dtype=torch.int32, device=dev)
            d2 = torch.empty((n, k), dtype=torch.float64, device=dev)
            count, rings = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
            mean = torch.empty(n, dtype=torch.float64, device=dev)
            nrm = torch.empty((n, 3), dtype=torch.float64, device=dev) if normal else None
            state = {}

            def binning():
                eng.ctx.call("im_knn_cells", ptr(pts), n, grid.ctypes.data, dims[0], dims[1], dims[2], ptr(key), st)

            def sort():
                state["skey"], state["perm"] = torch.sort(key, stable=True)

            def ranges():
                eng.ctx.call("im_knn_cell_ranges", ptr(state["skey"]), n, cells, ptr(start), st)

            def search():
                eng.ctx.call("im_knn_self", ptr(pts), ptr(state["perm"]), ptr(start), n, grid.ctypes.data, dims[0], dims[1], dims[2], k, radius2,
                             ptr(count), ptr(idx), ptr(d2), ptr(mean), ptr(nrm), ptr(rings), st)

            def whole():
                binning(), sort(), ranges(), search()

            out = {"cell_size": s, "dims": dims, "cells": cells}
            whole()
            for name, fn in (("binning", binning), ("sort", sort), ("ranges", ranges), ("search", search), ("whole", whole)):
                out[name + "_ms"], out[name + "_ms_all"] = timed(torch, fn, a.repeats)
            out["sort_share"] = round(out["sort_ms"] / out["whole_ms"], 4)
            out["points_per_s"] = round(n / (out["whole_ms"] * 1e-3))
            out["mean_rings"] = round(float(rings.abs().float().mean()), 3)
            out["max_rings"] = int(rings.abs().max())
            out["whole_cloud_scans"] = int((rings < 0).sum())          # searches that spent their step budget on the rings
            out["occupied_cells"] = int(torch.unique(state["skey"]).numel())
            return out, idx, d2

        for k in (10, 30, 50):
            out, idx, d2 = parts(k)
            # a brute force over the whole cloud for a few points: the production size reaches what the small shapes of the suite do not
            sel = np.random.default_rng(k).integers(0, n, a.check)
            hidx, hd2 = idx[torch.from_numpy(sel).to(dev)].cpu().numpy(), d2[torch.from_numpy(sel).to(dev)].cpu().numpy()
            index = np.arange(n)
            equal = True
            for j, i in enumerate(sel):
                d = host[i] - host
                bd2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
                order = np.lexsort((index, bd2))[:k]
                equal = equal and np.array_equal(order, hidx[j]) and np.array_equal(bd2[order].view(np.uint64), hd2[j].view(np.uint64))
            out["checked_points"], out["equal_to_brute_force"] = int(a.check), bool(equal)
            ok = ok and equal
            if not a.no_kdtree:
                from scipy.spatial import cKDTree
                t0 = time.perf_counter()
                tree = cKDTree(host)
                t1 = time.perf_counter()
                tree.query(host, k, workers=16)
                t2 = time.perf_counter()
                out["ckdtree_build_s"], out["ckdtree_query_s_16_workers"] = round(t1 - t0, 3), round(t2 - t1, 3)
                out["ckdtree_over_device"] = round((t2 - t0) / (out["whole_ms"] * 1e-3), 1)
            entry["searches"][f"k{k}"] = out
            print(f"{cname} k={k}: {out['whole_ms']:.2f} ms ({out['points_per_s'] / 1e6:.1f} M points/s), search {out['search_ms']:.2f}, sort share "
                  f"{out['sort_share']:.2f}, s = {out['cell_size']:.4g}, mean rings {out['mean_rings']}, equal {equal}", flush=True)
        for occ in a.occupancy:
            out, _, _ = parts(30, occupancy=occ)
            entry["occupancy_sweep_k30"][str(occ)] = {key: out[key] for key in ("cell_size", "cells", "occupied_cells", "whole_ms", "search_ms", "mean_rings", "whole_cloud_scans")}
            print(f"{cname} k=30 occupancy {occ}: {out['whole_ms']:.2f} ms, s = {out['cell_size']:.4g}, mean rings {out['mean_rings']}", flush=True)
        out, _, _ = parts(30, radius2=1.0, normal=True)
        entry["normals_radius1_nn30"] = {key: out[key] for key in ("cell_size", "whole_ms", "whole_ms_all", "search_ms", "points_per_s", "mean_rings")}
        print(f"{cname} normals: {out['whole_ms']:.2f} ms", flush=True)
        far = host.copy()                                            # one garbage point 1e6 away along y: the grid becomes long and thin
        far[0] = (far[0, 0], far[0, 1] + 1.0e6, far[0, 2])
        pts_all, pts = pts, torch.from_numpy(far).to(dev)
        lo, hi = far.min(0), far.max(0)
        out, _, _ = parts(30)
        entry["one_point_1e6_away_k30"] = {key: out[key] for key in ("cell_size", "dims", "whole_ms", "search_ms", "mean_rings", "max_rings", "whole_cloud_scans")}
        print(f"{cname} with one point 1e6 away, k=30: {out['whole_ms']:.2f} ms, dims {out['dims']}, scans {out['whole_cloud_scans']}", flush=True)
        pts, lo, hi = pts_all, host.min(0), host.max(0)
        for nb, ratio in ((10, 3.0), (50, 1.5)):
            F.remove_statistical_outlier(pts, nb, ratio, engine=eng)
            torch.cuda.synchronize()
            secs = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                kept, ind = F.remove_statistical_outlier(pts, nb, ratio, engine=eng)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
            entry[f"sor_{nb}_{ratio}"] = {"end_to_end_ms": round(float(np.median(secs)) * 1e3, 2), "kept": int(len(ind)),
                                          "note": "device tensor in and out: heuristic, search, download of the statistic, host sums, compaction"}
            print(f"{cname} SOR {nb} / {ratio}: {np.median(secs) * 1e3:.1f} ms end to end, {len(ind)} of {n} kept", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not ok:
        sys.exit("the device output differs from the brute force at the production size")


if __name__ == "__main__":
    main()
