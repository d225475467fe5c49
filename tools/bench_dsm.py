#!/usr/bin/env python3
"""DSM and orthophoto timings on one MI355X (`build_dsm` / `generate_ortophoto`, csrc/dsm.hip). Prints ONE JSON line with two cases:
  tie     a 30 k-point tie cloud on a 0.1 m grid of 5000 x 3000 = 15 M cells, and its orthophoto from a 6000 x 4000 RGB image
  dense   1 M points on a 0.2 m grid of 1250 x 1200 = 1.5 M cells
For each: device time per stage (binning: rounding + torch's sorts + group means; rasterisation + evaluation; orthophoto), the
host's qhull time (scipy Delaunay + its barycentric transforms), the transfers (the float64 grid to the host is the large one), the
wall time of the public calls including their numpy outputs, and the oracle's CPU time (tests/dsm_oracle.py: scipy + numpy, the
reference's own algorithm without pandas). The raster and orthophoto kernels are also put against the measured 6.3 TB/s HBM copy
rate with a minimal traffic model: raster + evaluation 16 B per cell (the per-cell triangle index written by the memset and read back,
the float64 z written); orthophoto 11 B per cell (z read, RGB written) plus one read of the image.

    python tools/bench_dsm.py [--reps 5] [--case tie|dense|both] [--no-oracle]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_COPY_TBS = 6.3


def surface(rng, x, y):
    return 50 + 8 * np.sin(x / 37) + 5 * np.cos(y / 23) + 0.02 * rng.normal(size=x.shape)


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


def stages(eng, pts, step, xlim, ylim, reps):
    """Each stage of build_dsm on its own (device stages by events, host stages by the wall clock)."""
    import torch
    from scipy.spatial import Delaunay
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.utils.dsm_orthophoto import _bin_on_device
    out = {}
    dev = eng.device
    t0 = time.perf_counter()
    dp = torch.from_numpy(pts).to(dev)
    torch.cuda.synchronize()
    out["upload_points_ms"] = (time.perf_counter() - t0) * 1e3
    out["bin_ms"] = timed(lambda: _bin_on_device(eng, pts, step), reps)   # includes the points' upload and the small download
    dev_b, host_b = _bin_on_device(eng, pts, step)
    out["groups"] = int(len(host_b[0]))
    t0 = time.perf_counter()
    tri = Delaunay(np.ascontiguousarray(np.stack(host_b[:2], 1), dtype=np.float64))
    out["qhull_delaunay_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    trans = np.ascontiguousarray(tri.transform)
    out["qhull_transform_ms"] = (time.perf_counter() - t0) * 1e3
    out["simplices"] = int(len(tri.simplices))
    xq, yq = np.arange(xlim[0], xlim[1], step), np.arange(ylim[0], ylim[1], step)
    cells = len(xq) * len(yq)
    out["cells"] = cells
    simp = np.ascontiguousarray(tri.simplices, dtype=np.int32)
    t0 = time.perf_counter()
    ds, dt = torch.from_numpy(simp).to(dev), torch.from_numpy(trans).to(dev)
    dxq, dyq = torch.from_numpy(xq).to(dev), torch.from_numpy(yq).to(dev)
    torch.cuda.synchronize()
    out["upload_triangles_ms"] = (time.perf_counter() - t0) * 1e3
    dz = torch.empty((len(yq), len(xq)), dtype=torch.float64, device=dev)
    bounds = np.ascontiguousarray(np.r_[tri.min_bound, tri.max_bound])
    args = (ptr(dev_b[0]), ptr(dev_b[1]), ptr(dev_b[2]), ptr(ds), ptr(dt), len(simp), bounds.ctypes.data, ptr(dxq), len(xq), ptr(dyq), len(yq),
            float(xq[0]), float(step), float(yq[0]), float(step), float("nan"), ptr(dz), eng.stream_ptr())
    ms = timed(lambda: eng.ctx.call("im_dsm_rasterize", *args), reps)
    out["raster_eval_ms"] = ms
    out["raster_eval_hbm_fraction"] = 16.0 * cells / (ms * 1e-3) / (HBM_COPY_TBS * 1e12)
    t0 = time.perf_counter()
    dz.cpu().numpy()
    out["z_to_host_ms"] = (time.perf_counter() - t0) * 1e3
    out["z_bytes"] = cells * 8
    return out, (dxq, dyq, dz)


def bench_case(eng, name, pts, step, xlim, ylim, image, cam, reps, oracle):
    import torch
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.sfm import _camera_params, _channel_map
    from icepy4d_amd.utils.dsm_orthophoto import build_dsm, generate_ortophoto
    r = {"points": len(pts), "step": step}
    st, (dxq, dyq, dz) = stages(eng, pts, step, xlim, ylim, reps)
    r.update(st)
    t0 = time.perf_counter()
    d = build_dsm(pts, dsm_step=step, xlim=xlim, ylim=ylim, engine=eng)
    r["build_dsm_wall_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    d = build_dsm(pts, dsm_step=step, xlim=xlim, ylim=ylim, engine=eng)
    r["build_dsm_wall_ms_2nd"] = (time.perf_counter() - t0) * 1e3
    r["qhull_share_of_wall"] = (r["qhull_delaunay_ms"] + r["qhull_transform_ms"]) / r["build_dsm_wall_ms_2nd"]
    if image is not None:
        rows, cols = d.z.shape
        dimg = torch.from_numpy(image).to(eng.device)
        out = torch.empty((rows, cols, 3), dtype=torch.uint8, device=eng.device)
        camp, chmap = _camera_params(cam), _channel_map(image, True)
        _, dxq, dyq, dz = d._device
        h, w, cin = image.shape
        args = (ptr(dxq), 0, 1, ptr(dyq), 1, 0, ptr(dz), cols, 1, rows, cols, 1, camp.ctypes.data, ptr(dimg), h, w, cin, chmap.ctypes.data, 3,
                None, None, ptr(out), eng.stream_ptr())
        ms = timed(lambda: eng.ctx.call("im_project_colors", *args), reps)
        r["ortho_kernel_ms"] = ms
        r["ortho_hbm_fraction"] = (11.0 * rows * cols + image.nbytes) / (ms * 1e-3) / (HBM_COPY_TBS * 1e12)
        t0 = time.perf_counter()
        o = generate_ortophoto(image, d, cam, engine=eng)
        r["generate_ortophoto_wall_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        o = generate_ortophoto(image, d, cam, engine=eng)
        r["generate_ortophoto_wall_ms_2nd"] = (time.perf_counter() - t0) * 1e3
        r["ortho_coloured_fraction"] = float((o.max(axis=2) > 0).mean())
    if oracle:
        import dsm_oracle as O
        t0 = time.perf_counter()
        ref = O.build_dsm(pts, step, xlim, ylim)
        r["oracle_build_dsm_cpu_ms"] = (time.perf_counter() - t0) * 1e3
        same = np.isnan(ref["z"]) == np.isnan(d.z)
        r["oracle_nan_mask_equal"] = bool(same.all())
        ok = ~np.isnan(ref["z"])
        r["oracle_z_bit_identical_fraction"] = float((ref["z"][ok] == d.z[ok]).mean())
        if image is not None:
            t0 = time.perf_counter()
            oo = O.orthophoto(*np.meshgrid(ref["xq"], ref["yq"]), d.z, image, cam.K, cam.dist, cam.R, cam.t)
            r["oracle_orthophoto_cpu_ms"] = (time.perf_counter() - t0) * 1e3
            r["oracle_orthophoto_identical"] = bool(np.array_equal(oo, o))
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=["tie", "dense", "both"], default="both")
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    from icepy4d_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(0)
    out = {"bench": "dsm_orthophoto", "hbm_copy_tbs": HBM_COPY_TBS}
    if a.case in ("tie", "both"):
        x, y = rng.uniform(0, 500, 30_000), rng.uniform(0, 300, 30_000)
        pts = np.c_[x, y, surface(rng, x, y)]
        from scipy import ndimage
        small = ndimage.gaussian_filter(rng.normal(0, 1, (1000 + 8, 1500 + 8, 3)), (2, 2, 0))
        img = np.kron(small, np.ones((4, 4, 1)))[:4000, :6000]
        img = np.clip((img - img.min()) / (img.max() - img.min()) * 255, 0, 255).astype(np.uint8)
        R = np.diag([1.0, -1.0, -1.0])
        C = np.array([250.0, 150.0, 450.0])
        cam = types.SimpleNamespace(K=np.array([[4400.0, 0, 3000], [0, 4400.0, 2000], [0, 0, 1]]),
                                    dist=np.array([-0.05, 0.01, 0.0005, -0.0003, 0.001]), R=R, t=-R @ C)
        out["tie"] = bench_case(eng, "tie", pts, 0.1, [0.0, 500.0], [0.0, 300.0], img, cam, a.reps, not a.no_oracle)
    if a.case in ("dense", "both"):
        x, y = rng.uniform(0, 250, 1_000_000), rng.uniform(0, 240, 1_000_000)
        pts = np.c_[x, y, surface(rng, x, y)]
        out["dense"] = bench_case(eng, "dense", pts, 0.2, [0.0, 250.0], [0.0, 240.0], None, None, a.reps, not a.no_oracle)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
