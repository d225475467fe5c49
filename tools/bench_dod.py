"""Times the volume-variation kernels of csrc/dod.hip on the device (device events, one warm-up, median of the repeats) on a synthetic
series of glacier fronts seen along x: `--clouds` epochs (default 8) of `--points` points each (default 2 M), a noisy height field over
150 m x 60 m that retreats from epoch to epoch, plus 0.5 % outliers off the surface; the pairs are `make_pairs(step=5)`'s, the step 0.3 m,
the direction "x" (the reference's `scripts/pcd_postprocessing/volume_variations.py`: TSTEP = 5, GRID_STEP = 0.3, DOD_DIR = "x").
Per step of the call (cloud bounds, keys, torch's stable sort, segment starts + cells + report): milliseconds for the series and per pair,
the sort's share, and the bytes each step must move per point and per cell (a model, stated in the output) against the 6.3 TB/s a copy
reaches on the device. `dod_series` end to end (upload and downloads included) by wall clock. The crop: 2 M points against a polygon of
64 vertices. Before timing, every report of the series and one raster are compared with tests/dod_oracle.py (bits); the oracle's CPU
seconds on this host are reported for scale, not asserted.

    python tools/bench_dod.py [--points 2000000] [--clouds 8] [--repeats 7] [--out profiles/r13_dod_bench.json]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
COPY_RATE = 6.3e12          # bytes per second of a device-to-device copy (read + write), profiles/README.md


def front(n, epoch, seed=13):
    rng = np.random.default_rng(seed + epoch)
    n_out = n // 200
    y, z = rng.uniform(0.0, 150.0, n - n_out), rng.uniform(0.0, 60.0, n - n_out)
    x = 500.0 + 12.0 * np.sin(y / 25.0) + 0.4 * z + 3.0 * np.sin(y / 4.0) * np.cos(z / 5.0) - 0.35 * epoch * (1.0 + 0.5 * np.cos(z / 11.0)) + rng.normal(0, 0.05, n - n_out)
    out = np.column_stack([rng.uniform(400.0, 600.0, n_out), rng.uniform(0.0, 150.0, n_out), rng.uniform(0.0, 60.0, n_out)])
    return np.concatenate([np.column_stack([x, y, z]), out])[rng.permutation(n)]


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
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_dod_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.points >= 1000 and a.clouds >= 6
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_dod.py needs a HIP device: there is nothing to time without one")
    import dod_oracle as O
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.post_processing.open3d_fun import crop_indices
    from icepy4d_amd.post_processing.utils import make_pairs
    from icepy4d_amd.volume_variations import FIELDS, dod_series
    eng = Engine(0)
    dev, st = eng.device, eng.stream_ptr()
    n, E, step, d = a.points, a.clouds, 0.3, 0
    host = [front(n, t) for t in range(E)]
    names = [Path(f"sampled_2022_05_{t + 1:02d}.ply") for t in range(E)]
    pair_dict, _ = make_pairs(names, 5)
    pairs = np.array([[names.index(Path(p0)), names.index(Path(p1))] for p0, p1 in pair_dict.values()], np.int32)
    P = len(pairs)
    res = {"device": torch.cuda.get_device_name(0), "points_per_cloud": n, "clouds": E, "pairs": pairs.tolist(), "step": step, "direction": "x",
           "repeats": a.repeats, "clock": "device events around the launches, one warm-up, median of the repeats; end to end and the oracle by wall clock"}

    offsets = (np.arange(E + 1) * n).astype(np.int64)
    pts = torch.from_numpy(np.concatenate(host)).to(dev)
    d_bounds = torch.empty((E, 4), dtype=torch.float64, device=dev)
    d_dropped = torch.empty(E, dtype=torch.int64, device=dev)
    items = int(2 * n * P)
    key = torch.empty(items, dtype=torch.int64, device=dev)
    grids = np.zeros((P, 4))
    state = {}

    def bounds():
        eng.ctx.call("im_dod_bounds", ptr(pts), offsets.ctypes.data, E, d, ptr(d_bounds), ptr(d_dropped), st)

    bounds()
    hb = np.ascontiguousarray(d_bounds.cpu().numpy())
    head = (ptr(pts), offsets.ctypes.data, E, pairs.ctypes.data, P, d, step, hb.ctypes.data)

    def keys():
        eng.ctx.call("im_dod_keys", *head, grids.ctypes.data, ptr(key), st)

    def sort():
        state["skey"], state["perm"] = torch.sort(key, stable=True)

    keys()
    cells = int((grids[:, 2] * grids[:, 3]).sum())
    d_H = torch.empty(cells, dtype=torch.float64, device=dev)
    d_report = torch.empty((P, len(FIELDS)), dtype=torch.float64, device=dev)

    def reduce():
        eng.ctx.call("im_dod_reduce", *head, ptr(state["skey"]), ptr(state["perm"]), ptr(d_H), ptr(d_report), st)

    def whole():
        bounds(), keys(), sort(), reduce()

    whole()
    # the production size against the restatement, before any timing
    t0 = time.perf_counter()
    want = [O.dod(host[g], host[c], d, step) for g, c in pairs]
    oracle_s = time.perf_counter() - t0
    report = d_report.cpu().numpy()
    equal = all(np.array_equal(report[k].view(np.uint64), want[k]["report_row"].view(np.uint64)) for k in range(P))
    H0 = d_H[:want[0]["H"].size].cpu().numpy()
    equal = equal and np.array_equal(H0.view(np.uint64), want[0]["H"].ravel().view(np.uint64))
    res["equal_to_oracle"], res["oracle_cpu_s"], res["oracle_cpu_s_per_pair"] = bool(equal), round(oracle_s, 3), round(oracle_s / P, 3)
    res["grids"] = [[int(g[2]), int(g[3])] for g in grids]
    res["cells"], res["items"] = cells, items
    res["points_per_filled_cell"] = round(2 * n / float(want[0]["report"]["cellCount"]), 2)
    res["reports"] = [{k: float(want[p]["report"][k]) for k in FIELDS[:10]} for p in range(P)]
    steps = {}
    for name, fn in (("bounds", bounds), ("keys", keys), ("sort", sort), ("reduce", reduce), ("whole", whole)):
        steps[name + "_ms"], steps[name + "_ms_all"] = timed(torch, fn, a.repeats)
    res["series"] = steps
    res["ms_per_pair"] = round(steps["whole_ms"] / P, 3)
    res["sort_share"] = round(steps["sort_ms"] / steps["whole_ms"], 4)
    # what each step must move: bounds reads every cloud once (24 B per point); keys reads 24 B and writes 8 B per item; reduce reads a
    # key (histogram) and a permutation entry (8 B each) and gathers one coordinate (8 B, of a 32 B sector at the least) per item, and per
    # cell writes and reads two counts (4 B), reads four starts (8 B), writes and reads H (8 B) and the state (1 B)
    model = {"bounds": 24 * n * E, "keys": 32 * items, "reduce": 24 * items + (2 * 2 * 4 + 4 * 8 + 2 * 8 + 2) * cells}
    res["bytes_model"] = {"per_point_bounds": 24, "per_item_keys": 32, "per_item_reduce": 24, "per_cell_reduce": 66}
    res["share_of_copy_rate"] = {k: round(model[k] / (steps[k + "_ms"] * 1e-3) / COPY_RATE, 4) for k in model}
    res["slowest_step"] = max(("bounds", "keys", "sort", "reduce"), key=lambda k: steps[k + "_ms"])
    print(f"series of {P} pairs: {steps['whole_ms']:.2f} ms ({res['ms_per_pair']:.2f} per pair): bounds {steps['bounds_ms']:.2f}, keys {steps['keys_ms']:.2f}, "
          f"sort {steps['sort_ms']:.2f} (share {res['sort_share']:.2f}), reduce {steps['reduce_ms']:.2f}; oracle {oracle_s:.2f} s on the host; equal {equal}", flush=True)

    secs = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dod_series(host, pairs, direction="x", grid_step=step, engine=eng)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    res["dod_series_end_to_end_ms"] = round(float(np.median(secs)) * 1e3, 2)
    res["dod_series_note"] = "numpy clouds in, reports out: concatenation and upload of every cloud once, the device pass, the downloads"
    print(f"dod_series end to end: {res['dod_series_end_to_end_ms']:.1f} ms", flush=True)

    # the crop: 2 M points x 64 vertices
    rng = np.random.default_rng(64)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 64))
    poly = np.ascontiguousarray(np.stack([75.0 + 60.0 * np.cos(ang), 30.0 + 25.0 * np.sin(ang)], 1) * rng.uniform(0.7, 1.0, (64, 1)))
    cloud = pts[:n]
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)

    def crop():
        eng.ctx.call("im_crop_polygon", ptr(cloud), n, 1, 2, poly.ctypes.data, 64, 1, ptr(mask), ptr(index), ptr(count), st)

    crop_ms, crop_all = timed(torch, crop, a.repeats)
    kept = int(count.item())
    want_mask = O.in_polygon(poly, host[0][:, 1], host[0][:, 2])
    crop_equal = bool(np.array_equal(mask.cpu().numpy().astype(bool), want_mask) and np.array_equal(index[:kept].cpu().numpy(), np.nonzero(want_mask)[0]))
    assert np.array_equal(crop_indices(cloud, poly, 1, 2, engine=eng), np.nonzero(want_mask)[0])
    res["crop"] = {"points": n, "vertices": 64, "ms": crop_ms, "ms_all": crop_all, "kept": kept, "equal_to_oracle": crop_equal,
                   "points_per_s": round(n / (crop_ms * 1e-3)), "edge_tests_per_s": round(64 * n / (crop_ms * 1e-3))}
    print(f"crop of {n} points by 64 vertices: {crop_ms:.3f} ms, {kept} kept, equal {crop_equal}", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not (equal and crop_equal):
        sys.exit("the device output differs from the restatement at the production size")


if __name__ == "__main__":
    main()
