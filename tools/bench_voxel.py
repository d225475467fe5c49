"""Times the voxel kernels of csrc/voxel.hip on the device (device events, one warm-up, median of the repeats) on the synthetic series of
glacier fronts of tools/bench_dod.py, moved into the box of the reference's `scripts/pcd_postprocessing/voxelization.py`: `--clouds`
epochs (default 8) of `--points` coloured points each (default 2 M), voxel size 0.2 m, the box (-100, 130, 60) .. (30, 330, 120) of 195 M
voxels, all epochs in one call. Per step: keys, torch's stable sort, reduce (grid indices, counts, first indices, colour means), and for
the box mesh of the first epoch corners, the second sort and mesh: milliseconds, and the bytes each step must move (a model, stated in
the output) against the 6.3 TB/s a copy reaches on the device. `voxelize` end to end (upload, device pass, downloads, the text files) by
wall clock. Before timing, the first epoch's voxels and mesh are compared with tests/voxel_oracle.py (bits); the restatement's seconds on
this host are reported for scale, not asserted.

    python tools/bench_voxel.py [--points 2000000] [--clouds 8] [--repeats 7] [--out profiles/r15_voxel_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
COPY_RATE = 6.3e12          # bytes per second of a device-to-device copy (read + write), profiles/README.md
SHIFT = (-535.0, 155.0, 60.0)     # bench_dod's front (x about 500, y 0..150, z 0..60) into the script's box


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


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_voxel_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.points >= 1000 and a.clouds >= 1
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_voxel.py needs a HIP device: there is nothing to time without one")
    import voxel_oracle as O
    from bench_dod import front
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.post_processing import voxel_grid as VG
    from icepy4d_amd.voxelization import BB_MAX, BB_MIN, VOXEL_SIZE, voxelize
    eng = Engine(0)
    dev, st = eng.device, eng.stream_ptr()
    n, E, s = a.points, a.clouds, VOXEL_SIZE
    host = [front(n, t) + SHIFT for t in range(E)]
    rng = np.random.default_rng(15)
    colours = [np.round(rng.uniform(0, 1, (n, 3)) * 255) / 255 for _ in range(E)]
    grid = VG.make_grid(np.array(BB_MIN, np.float64), np.array(BB_MAX, np.float64), s)
    dims = VG.grid_dims(grid)
    res = {"device": torch.cuda.get_device_name(0), "points_per_cloud": n, "clouds": E, "voxel_size": s, "box": [list(BB_MIN), list(BB_MAX)], "grid": list(dims),
           "grid_voxels": int(np.prod(dims, dtype=object)), "repeats": a.repeats,
           "clock": "device events around the launches, one warm-up, median of the repeats; end to end and the restatement by wall clock"}
    N = n * E
    offsets = (np.arange(E + 1) * n).astype(np.int64)
    pts, col = torch.from_numpy(np.concatenate(host)).to(dev), torch.from_numpy(np.concatenate(colours)).to(dev)
    key, d_dropped, d_nvox = torch.empty(N, dtype=torch.int64, device=dev), torch.empty(E, dtype=torch.int64, device=dev), torch.empty(E + 1, dtype=torch.int64, device=dev)
    d_index = torch.empty((N, 3), dtype=torch.int32, device=dev)
    d_count, d_first = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    d_mean = torch.empty((N, 3), dtype=torch.float64, device=dev)
    head = (offsets.ctypes.data, E, grid.ctypes.data, 0)
    state = {}

    def keys():
        eng.ctx.call("im_voxel_keys", ptr(pts), *head, ptr(key), ptr(d_dropped), st)

    def sort():
        state["skey"], state["perm"] = torch.sort(key, stable=True)

    def reduce():
        eng.ctx.call("im_voxel_reduce", *head, ptr(state["skey"]), ptr(state["perm"]), None, ptr(col), None, ptr(d_nvox), ptr(d_index), ptr(d_count), ptr(d_first),
                     None, ptr(d_mean), None, st)

    keys(), sort(), reduce()
    nvox = d_nvox.cpu().numpy()
    V_all, V0 = int(nvox[E]), int(nvox[1])
    t0 = time.perf_counter()
    want = O.voxelize(host[0], grid, colours[0])
    oracle_s = time.perf_counter() - t0
    equal = (bits_equal(d_index[:V0].cpu().numpy(), want["grid_index"]) and bits_equal(d_count[:V0].cpu().numpy(), want["counts"])
             and bits_equal(d_first[:V0].cpu().numpy(), want["first"]) and bits_equal(d_mean[:V0].cpu().numpy(), want["colors"])
             and int(d_dropped[0]) == want["dropped"])
    res.update({"voxels": V_all, "voxels_first_cloud": V0, "points_per_voxel": round(N / max(V_all, 1), 2), "dropped": d_dropped.cpu().numpy().tolist(),
                "filled_share_of_grid": V0 / float(res["grid_voxels"]), "equal_to_oracle": bool(equal), "oracle_cpu_s_per_cloud": round(oracle_s, 3)})

    # the box mesh of the first epoch
    index0, col0 = d_index[:V0].contiguous(), d_mean[:V0].contiguous()
    ckey = torch.empty(8 * V0, dtype=torch.int64, device=dev)
    d_nv = torch.empty(1, dtype=torch.int64, device=dev)
    d_vert, d_vcol = torch.empty((8 * V0, 3), dtype=torch.float64, device=dev), torch.empty((8 * V0, 3), dtype=torch.float64, device=dev)
    d_tri = torch.empty((12 * V0, 3), dtype=torch.int32, device=dev)

    def corners():
        eng.ctx.call("im_voxel_mesh_corners", grid.ctypes.data, ptr(index0), V0, ptr(ckey), st)

    def sort2():
        state["ckey"], state["cperm"] = torch.sort(ckey, stable=True)

    def mesh():
        eng.ctx.call("im_voxel_mesh", grid.ctypes.data, V0, ptr(col0), ptr(state["ckey"]), ptr(state["cperm"]), ptr(d_nv), ptr(d_vert), ptr(d_vcol), ptr(d_tri), st)

    corners(), sort2(), mesh()
    U = int(d_nv.cpu()[0])
    t0 = time.perf_counter()
    wv, wc, wt = O.box_mesh(grid, want["grid_index"], want["colors"])
    mesh_oracle_s = time.perf_counter() - t0
    mesh_equal = bits_equal(d_vert[:U].cpu().numpy(), wv) and bits_equal(d_vcol[:U].cpu().numpy(), wc) and bits_equal(d_tri.cpu().numpy(), wt)
    res.update({"mesh_vertices": U, "mesh_triangles": 12 * V0, "mesh_equal_to_oracle": bool(mesh_equal), "mesh_oracle_cpu_s": round(mesh_oracle_s, 3)})

    def whole():
        keys(), sort(), reduce()

    steps = {}
    for name, fn in (("keys", keys), ("sort", sort), ("reduce", reduce), ("whole", whole), ("corners", corners), ("sort2", sort2), ("mesh", mesh)):
        steps[name + "_ms"], steps[name + "_ms_all"] = timed(torch, fn, a.repeats)
    res["steps"] = steps
    # What each step must move at the least. keys: 24 B read and 8 B written per point. reduce: the two scan passes read every key once
    # (16 B per point), the voxel pass reads a permutation entry (8 B) and gathers one colour row (24 B, of 32 B sectors) per point; per
    # voxel a start written and read twice (12 B), a key (8 B) and 44 B of results. corners: 12 B read and 64 B written per voxel. mesh: per
    # item the two scan passes (16 B), a permutation entry twice (16 B) and a vertex number written and read (8 B); per vertex a start
    # (12 B), 48 B written and 24 B of colour per sharing voxel (counted with the items); per voxel 144 B of triangles.
    items = 8 * V0
    model = {"keys": 32 * N, "reduce": 48 * N + 64 * V_all, "corners": 76 * V0, "mesh": (40 + 24) * items + 60 * U + 144 * V0}
    res["bytes_model"] = {"keys_per_point": 32, "reduce_per_point": 48, "reduce_per_voxel": 64, "corners_per_voxel": 76, "mesh_per_item": 64, "mesh_per_vertex": 60,
                          "mesh_per_voxel": 144}
    res["share_of_copy_rate"] = {k: round(model[k] / (steps[k + "_ms"] * 1e-3) / COPY_RATE, 4) for k in model}
    res["sort_share"] = round(steps["sort_ms"] / steps["whole_ms"], 4)
    res["not_determined"] = ("no counter run was made: what bounds im_voxel_reduce is not determined (the candidate is the one thread per voxel gathering its "
                             "points through the permutation)")
    print(f"{E} clouds of {n}: {V_all} voxels; keys {steps['keys_ms']:.2f} ms, sort {steps['sort_ms']:.2f}, reduce {steps['reduce_ms']:.2f}, whole "
          f"{steps['whole_ms']:.2f}; mesh of {V0} voxels: corners {steps['corners_ms']:.3f}, sort {steps['sort2_ms']:.3f}, mesh {steps['mesh_ms']:.3f}; "
          f"equal {equal} / {mesh_equal}; restatement {oracle_s:.2f} s per cloud, mesh {mesh_oracle_s:.2f} s", flush=True)

    secs = []
    with tempfile.TemporaryDirectory() as tmp:
        clouds = [(p, c) for p, c in zip(host, colours)]
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            voxelize(clouds, out_dir=tmp, engine=eng)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        from icepy4d_amd.voxelization import voxel_series
        voxel_series(clouds, engine=eng)
        torch.cuda.synchronize()
        series_s = time.perf_counter() - t0
    res["voxelize_end_to_end_s"] = round(float(np.median(secs)), 3)
    res["voxel_series_end_to_end_s"] = round(series_s, 3)
    res["end_to_end_note"] = ("numpy clouds in: concatenation and upload of every cloud once, the device pass, the downloads (voxel_series); voxelize adds the text "
                              "file of every epoch, written by Python; median of 3 / one run")
    print(f"voxel_series end to end {series_s:.2f} s, voxelize with its text files {res['voxelize_end_to_end_s']:.2f} s", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not (equal and mesh_equal):
        sys.exit("the device output differs from the restatement at the production size")


if __name__ == "__main__":
    main()
