#!/usr/bin/env python3
"""Velocity-field timings on one MI355X (`binned_statistics`, csrc/binned.hip). Writes profiles/r10_velocity_bench.json and prints it.
  epochs   158 point sets x 200 000 points, 4 value columns, median + mean + count on a 200 x 200 grid, in one call
  single   one set of 5000 points, the same columns, statistics and grid
Device times are events around each stage (cell assignment, torch's stable sort, the statistics call), the median of 7 after a warm-up,
with the inputs already on the device; the library's own per-launch profile splits the statistics call into its kernels. The public
call's wall time includes the uploads and the download of the statistics. Next to it `scipy.stats.binned_statistic_2d` on the same
inputs on the host: 3 x 4 calls per set; for `epochs` it is timed on the first --scipy-sets sets and scaled to 158 (each set is an
independent call of the same size). Traffic model of the statistics call, compulsory bytes only: the sorted keys and the permutation
read once (16 B per point), every value gathered once per statistic kernel that needs it (8 B per point and column, twice: basic +
median), the offsets (8 B per cell) and the outputs (8 B per cell, column and statistic), against the measured 6.3 TB/s HBM copy rate.

    python tools/bench_velocity.py [--reps 7] [--scipy-sets 3] [--case epochs|single|both]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_TBS = 6.3
STATS = ("median", "mean", "count")


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def bench_case(eng, n_sets, n_per_set, reps, scipy_sets):
    import torch
    from scipy.stats import binned_statistic_2d
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.utils import binned_stats as M
    rng = np.random.default_rng(10)
    N, V, G = n_sets * n_per_set, 4, 200
    nodes = np.arange(G) * 2.0
    edges = [np.asarray(e) for e in M.bins_from_nodes(nodes, nodes)]
    pts = rng.uniform(edges[0][0] - 2.0, edges[0][-1] + 2.0, (N, 2))
    vals = rng.normal(0.0, 1.0, (V, N)) * 10.0 ** rng.uniform(-2, 2, (V, N))
    offs = np.arange(n_sets + 1, dtype=np.int64) * n_per_set
    r = {"sets": n_sets, "points_per_set": n_per_set, "columns": V, "statistics": list(STATS), "grid": [G, G], "cells": n_sets * G * G}

    t0 = time.perf_counter()
    out = M.binned_statistics(pts, vals, STATS, edges, offs, engine=eng)
    r["public_call_wall_ms_1st"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    out = M.binned_statistics(pts, vals, STATS, edges, offs, engine=eng)
    r["public_call_wall_ms_2nd"] = (time.perf_counter() - t0) * 1e3

    # the stages, inputs resident
    dev, st = eng.device, eng.stream_ptr()
    dp, dv = torch.from_numpy(pts).to(dev), torch.from_numpy(vals).to(dev)
    de, do = torch.from_numpy(np.concatenate(edges)).to(dev), torch.from_numpy(offs).to(dev)
    key = torch.empty(N, dtype=torch.int64, device=dev)
    ne, sc, mo = np.array([G + 1, G + 1], np.int32), np.array([1e6, 1e6]), np.array([1, 1], np.int32)
    dmin = min(np.diff(e).min() for e in edges)
    sc[:] = 10.0 ** (int(-np.log10(dmin)) + 6)
    cells = lambda: eng.ctx.call("im_binned_cells", ptr(dp), N, 2, ptr(de), ne.ctypes.data, sc.ctypes.data, mo.ctypes.data, ptr(do), n_sets, ptr(key), st)  # noqa: E731
    r["cells_ms"] = timed(cells, reps)
    r["sort_ms"] = timed(lambda: torch.sort(key, stable=True), reps)
    skey, perm = torch.sort(key, stable=True)
    slots = np.full(7, -1, np.int32)
    slots[[6, 2, 0]] = [0, 1, 2]
    dout = torch.empty((3, n_sets, V, G, G), dtype=torch.float64, device=dev)
    stats = lambda: eng.ctx.call("im_binned_stats", ptr(skey), ptr(perm), N, n_sets, G * G, ptr(dv), V, slots.ctypes.data, ptr(dout), st)  # noqa: E731
    r["stats_ms"] = timed(stats, reps)
    r["device_total_ms"] = r["cells_ms"] + r["sort_ms"] + r["stats_ms"]
    eng.ctx.call("im_profile_begin")
    for _ in range(reps):
        stats()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    eng.ctx.call("im_profile_end", buf, len(buf))
    prof = json.loads(buf.value.decode())
    cal = prof.pop("_empty_event_pair", None)
    ov = cal["total_ms"] / cal["count"] if cal and cal["count"] else 0.0
    r["stats_kernels_ms"] = {k: (v["total_ms"] - v["count"] * ov) / reps for k, v in prof.items()}
    n_cells = n_sets * G * G
    traffic = 16.0 * N + 2 * 8.0 * N * V + 8.0 * n_cells + 8.0 * n_cells * V * len(STATS)
    r["stats_model_bytes"] = traffic
    r["stats_hbm_fraction"] = traffic / (r["stats_ms"] * 1e-3) / (HBM_COPY_TBS * 1e12)
    assert np.array_equal(dout.cpu().numpy()[0], out["median"], equal_nan=True)

    k = min(scipy_sets, n_sets)
    t0 = time.perf_counter()
    same = True
    for e in range(k):
        lo, hi = offs[e], offs[e + 1]
        for s in STATS:
            for c in range(V):
                ref = binned_statistic_2d(pts[lo:hi, 0], pts[lo:hi, 1], vals[c, lo:hi], s, bins=edges).statistic
                same = same and np.array_equal(ref, out[s][e, c], equal_nan=True)
    ms = (time.perf_counter() - t0) * 1e3
    r["scipy_sets_timed"], r["scipy_ms_per_set"], r["scipy_ms_all_sets_scaled"] = k, ms / k, ms / k * n_sets
    r["identical_to_scipy_on_timed_sets"] = bool(same)
    r["speedup_device_total_vs_scipy"] = r["scipy_ms_all_sets_scaled"] / r["device_total_ms"]
    r["speedup_public_call_vs_scipy"] = r["scipy_ms_all_sets_scaled"] / r["public_call_wall_ms_2nd"]

    def rnd(v):
        return round(v, 4) if isinstance(v, float) else ({a: rnd(b) for a, b in v.items()} if isinstance(v, dict) else v)
    return {a: rnd(b) for a, b in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scipy-sets", type=int, default=3)
    ap.add_argument("--case", choices=["epochs", "single", "both"], default="both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_velocity_bench.json"))
    a = ap.parse_args()
    from icepy4d_amd.engine import Engine
    eng = Engine(0)
    out = {"bench": "velocity_fields", "hbm_copy_tbs": HBM_COPY_TBS, "reps": a.reps}
    if a.case in ("single", "both"):
        out["single"] = bench_case(eng, 1, 5000, a.reps, 1)
    if a.case in ("epochs", "both"):
        out["epochs"] = bench_case(eng, 158, 200_000, a.reps, a.scipy_sets)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
