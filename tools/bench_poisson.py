"""Times the Poisson surface reconstruction of csrc/poisson.hip on the device (device events, one warm-up, median of the repeats) on a
synthetic glacier front of `--points` points (default 2 M: the sloped, undulating front of tests/poisson_cases.py) at depth 7, 8 and 9:
  - per stage: the splat (memset, atomics, conversion), the divergence, the solve (8 V-cycles), the iso-value (two ordered sums), the
    crossing census, the extraction; and the whole `poisson_reconstruct` from device tensors to host arrays by wall clock;
  - per streaming kernel at the finest level: one Jacobi sweep, residual + restriction, prolongation, with the bytes each must move at
    least (every field read or written once: neighbours are taken as cached) and the rate that makes of the time.
Before timing, the depth-7 field of the first 20 000 points is compared with the restatement (tests/poisson_oracle.py, bits).
The rates are arithmetic on minimum traffic, not counters: what bounds each kernel (HBM, as a streaming stencil suggests, or the atomics
of the splat) is marked unmeasured until a counter run of its own exists.

    python tools/bench_poisson.py [--points 2000000] [--depths 7 8 9] [--repeats 5] [--out profiles/r18_poisson_bench.json]"""
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
from bench_pointcloud import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--depths", type=int, nargs="*", default=[7, 8, 9])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_poisson_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.points >= 20000
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_poisson.py needs a HIP device: there is nothing to time without one")
    import poisson_cases as PC
    import poisson_oracle as O
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.post_processing import poisson as P
    eng = Engine(0)
    dev, st, call = eng.device, eng.stream_ptr(), eng.ctx.call
    pts, nrm = PC.front(a.points, 5)
    small = P.poisson_field(pts[:20000], nrm[:20000], depth=7, engine=eng)
    want = O.field(pts[:20000], nrm[:20000], depth=7)
    equal = bool(np.array_equal(small.chi.cpu().numpy(), want["chi"]) and small.iso == want["iso"])
    del small, want
    d_pts, d_nrm = torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "points": a.points, "repeats": a.repeats, "cycles": P.CYCLES,
           "clock": "device events around each stage (its launches and torch's allocations), one warm-up, median of the repeats; `reconstruct_wall_ms` by wall clock with a "
                    "synchronise, device tensors in, host arrays out",
           "depth7_field_of_20000_points_equal_to_oracle": equal, "bound": "unmeasured: no counter run; the rates below are minimum traffic over time", "depths": {}}
    for depth in a.depths:
        origin, h, _ = P.grid_of(pts.min(0), pts.max(0), depth, 0, 1.1)
        M = 2 ** depth + 1
        N = M ** 3
        grid = np.array([*origin, h])
        fields = torch.empty((4, N), dtype=torch.float64, device=dev)
        rhs, coarse = torch.empty(N, dtype=torch.float64, device=dev), torch.empty((2 ** (depth - 1) + 1) ** 3, dtype=torch.float64, device=dev)
        ms, every = {}, {}

        def stage(name, fn):
            ms[name], every[name] = timed(torch, fn, a.repeats)

        stage("splat", lambda: call("im_poisson_splat", ptr(d_pts), ptr(d_nrm), a.points, grid.ctypes.data, depth, ptr(fields), st))
        stage("divergence", lambda: call("im_poisson_divergence", ptr(fields[1:]), depth, h, ptr(rhs), st))
        W, chi, tmp = fields[0], fields[1], fields[2]
        h2 = h * h
        stage("jacobi_sweep", lambda: call("im_poisson_jacobi", ptr(chi), ptr(rhs), depth, h2, ptr(tmp), st))
        stage("residual_restrict", lambda: call("im_poisson_restrict", ptr(chi), ptr(rhs), depth, h2, ptr(tmp), ptr(coarse), st))
        stage("prolong", lambda: call("im_poisson_prolong", ptr(coarse), depth, ptr(chi), st))

        def solve():
            chi.zero_()
            P._solve(eng, chi, rhs, tmp, h, depth, P.CYCLES)
        stage("solve", solve)
        iso = [0.0]

        def iso_value():
            iso[0] = P._ordered_sum(eng, W, chi) / P._ordered_sum(eng, W)
        stage("iso", iso_value)
        f = P.PoissonField(origin, h, depth, chi.view(M, M, M), iso[0], W.view(M, M, M))
        mask, base, counts = torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
        stage("census", lambda: call("im_poisson_census", ptr(chi), iso[0], depth, ptr(mask), ptr(base), ptr(counts), st))
        nv, nt = (int(c) for c in counts.cpu())
        vert, wgt, tri = torch.empty((nv, 3), dtype=torch.float64, device=dev), torch.empty(nv, dtype=torch.float64, device=dev), torch.empty((nt, 3), dtype=torch.int32, device=dev)
        stage("extract", lambda: call("im_poisson_extract", ptr(chi), ptr(W), iso[0], depth, grid.ctypes.data, ptr(mask), ptr(base), nv, nt, ptr(vert), ptr(wgt), ptr(tri), st))
        dens = P.density_of(wgt.cpu().numpy(), depth)
        del fields, rhs, coarse, mask, base, vert, wgt, tri, W, chi, tmp, f
        torch.cuda.empty_cache()
        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.poisson_reconstruct(d_pts, d_nrm, depth=depth, engine=eng)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.empty_cache()
        traffic = {"jacobi_sweep": 3 * 8 * N, "residual_restrict": 4 * 8 * N + 8 * N // 8, "prolong": 2 * 8 * N + 8 * N // 8, "divergence": 4 * 8 * N}
        out["depths"][str(depth)] = {
            "nodes_per_axis": M, "cell_size_m": h, "vertices": nv, "triangles": nt, "iso": iso[0],
            "density_min_median_max": [float(dens.min()), float(np.median(dens)), float(dens.max())],
            "device_ms": {k: round(v, 3) for k, v in ms.items()}, "device_ms_all": every,
            "pipeline_ms": round(sum(ms[k] for k in ("splat", "divergence", "solve", "iso", "census", "extract")), 3),
            "reconstruct_wall_ms": round(float(np.median(wall)), 1), "reconstruct_wall_ms_all": [round(w, 1) for w in wall],
            "minimum_bytes": traffic, "minimum_traffic_GB_per_s": {k: round(traffic[k] / (ms[k] * 1e-3) / 1e9, 1) for k in traffic},
            "field_GB": round(8 * N / 1e9, 3)}
        print(depth, json.dumps(out["depths"][str(depth)]["device_ms"]), "wall", out["depths"][str(depth)]["reconstruct_wall_ms"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({"out": a.out, "equal": equal}))


if __name__ == "__main__":
    main()
