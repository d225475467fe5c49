"""Times the mesh steps of `MeshingPoisson` on the device (csrc/mesh.hip) on a synthetic surface of the size the reference's
`scripts/pcd_postprocessing/point_cloud_meshing.py` produces at depth 9: a height field of `--side`^2 vertices (default 1225^2 = 1.50 M)
and 2 (side - 1)^2 triangles (3.00 M) with made-up densities, some duplicated vertices and triangles and a few degenerate triangles. The
steps, each on the output of the one before and each timed on its own (device events, one warm-up, median of the repeats; torch's sorts
and the read-back of the counts included): the density filter (`remove_vertices_by_mask`), `remove_degenerate_triangles`,
`remove_duplicated_triangles` (keys, two sorts, first of segment, select), `remove_duplicated_vertices` (keys, three sorts, first of
segment, select), the census of `remove_non_manifold_edges` (keys, sort, census), the hull filter (`point_in_hull` + `select_by_index`)
and `--samples` samples (default 4 M: table + sample kernel). Before timing, every step is compared with tests/mesh_oracle.py (bits); the
restatement's wall-clock seconds on this host are the baseline.

    python tools/bench_mesh.py [--side 1225] [--samples 4000000] [--repeats 7] [--out profiles/r16_mesh_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_voxel import bits_equal, timed  # noqa: E402


def surface(side, rng):
    x, y = np.meshgrid(np.arange(side, dtype=np.float64) * 0.25, np.arange(side, dtype=np.float64) * 0.25, indexing="ij")
    z = 8.0 * np.sin(x / 40.0) + 5.0 * np.cos(y / 25.0) + 0.05 * rng.normal(0, 1, x.shape)
    v = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    a = (np.arange(side - 1)[:, None] * side + np.arange(side - 1)[None]).ravel()
    t = np.concatenate([np.stack([a, a + side, a + 1], 1), np.stack([a + 1, a + side, a + side + 1], 1)]).astype(np.int32)
    density = 10.0 + 2.5 * np.sin(x / 30.0 + 1.0) * np.cos(y / 45.0) + rng.normal(0, 0.4, x.shape)
    d = density.ravel().copy()
    dup_v = rng.choice(len(v), 2000, replace=False)                    # 2000 vertices twice, 2000 triangles twice (rotated), 500 degenerate
    v, d = np.concatenate([v, v[dup_v]]), np.concatenate([d, d[dup_v]])
    dup_t = t[rng.choice(len(t), 2000, replace=False)][:, [1, 2, 0]]
    deg = t[rng.choice(len(t), 500, replace=False)].copy()
    deg[:, 2] = deg[:, 0]
    moved = t[rng.choice(len(t), 2000, replace=False)].copy()         # triangles that use the second copy of a vertex
    moved[:, 0] = len(v) - 2000 + rng.integers(0, 2000, 2000)
    return v, np.concatenate([t, dup_t, deg, moved]).astype(np.int32), d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1225)
    ap.add_argument("--samples", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--min-density", type=float, default=9.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_mesh_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.side >= 16
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mesh.py needs a HIP device: there is nothing to time without one")
    import mesh_oracle as O
    from icepy4d_amd.engine import Engine, to_device
    from icepy4d_amd.post_processing import triangle_mesh as TM
    eng = Engine(0)
    dev = eng.device
    rng = np.random.default_rng(16)
    v, t, density = surface(a.side, rng)
    extent = (a.side - 1) * 0.25
    inner = rng.uniform((0.1 * extent, 0.08 * extent, -30.0), (0.9 * extent, 0.93 * extent, 30.0), (50000, 3))
    hull_points = TM.compute_convex_hull(inner)
    facets = TM.hull_facets(hull_points)
    N = a.samples
    res = {"device": torch.cuda.get_device_name(0), "vertices": len(v), "triangles": len(t), "samples": N, "min_mesh_denisty": a.min_density,
           "hull_vertices": len(hull_points), "hull_facets": len(facets), "repeats": a.repeats,
           "clock": "device events around each step (its launches, torch's sorts and the read-back of its counts), one warm-up, median of the repeats; "
                    "the numpy restatement by wall clock, one run"}

    # ---- the chain on the host (the baseline, and what the device must equal) and on the device ----------------------------------------------
    host_s, dev_ms, sizes, equal = {}, {}, {}, {}
    state = {"v": to_device(v, dev, np.float64), "t": to_device(t, dev, np.int32)}
    mesh = O.Mesh(v, t)

    def host(name, fn):
        t0 = time.perf_counter()
        r = fn()
        host_s[name] = round(time.perf_counter() - t0, 3)
        return r

    def take(vlist, tri):
        state["v"], state["t"] = state["v"][vlist.long()].contiguous(), tri.contiguous()

    def step(name, host_fn, dev_fn):
        nonlocal mesh
        V = int(state["v"].shape[0])
        out, vlist, pos = host(name, host_fn)
        _, d_vlist, d_tri, d_pos = dev_fn(V)
        equal[name] = bits_equal(d_vlist.cpu().numpy(), vlist) and bits_equal(d_tri.cpu().numpy(), out.triangles) and bits_equal(d_pos.cpu().numpy(), pos)
        dev_ms[name], dev_ms[name + "_all"] = timed(torch, lambda: dev_fn(V), a.repeats)
        take(d_vlist, d_tri)
        mesh = out
        sizes[name] = [len(out.vertices), len(out.triangles)]

    d_keep = to_device((~(density < a.min_density)).astype(np.uint8), dev, np.uint8)
    step("density_filter", lambda: mesh.remove_vertices_by_mask(density < a.min_density), lambda V: TM.device_select(eng, V, state["t"], vertex_keep=d_keep))
    step("degenerate", lambda: mesh.remove_degenerate_triangles(), lambda V: TM.device_select(eng, V, state["t"], drop_degenerate=True))

    def dup_triangles(V):
        _, keep = TM.device_first_of_segment(eng, TM.device_triangle_keys(eng, state["t"]))
        return TM.device_select(eng, V, state["t"], triangle_keep=keep)

    def dup_vertices(V):
        first, keep = TM.device_first_of_segment(eng, TM.device_vertex_keys(eng, state["v"]))
        return TM.device_select(eng, V, state["t"], vertex_keep=keep, merge=first)
    step("duplicated_triangles", lambda: mesh.remove_duplicated_triangles(), dup_triangles)
    step("duplicated_vertices", lambda: mesh.remove_duplicated_vertices(), dup_vertices)
    census = host("non_manifold_census", lambda: O.edge_census(mesh.triangles))
    got = TM.device_edge_census(eng, state["t"])
    equal["non_manifold_census"] = got == census
    dev_ms["non_manifold_census"], dev_ms["non_manifold_census_all"] = timed(torch, lambda: TM.device_edge_census(eng, state["t"]), a.repeats)
    res["edges_with_more_than_two_triangles"] = got

    def hull_filter(V):
        return TM.device_select(eng, V, state["t"], vertex_keep=TM.device_in_hull(eng, state["v"], facets), drop_unreferenced=True)
    step("hull_filter", lambda: mesh.select_by_index(np.nonzero(O.point_in_hull(mesh.vertices, facets))[0]), hull_filter)

    want = host("sample", lambda: O.sample(mesh.vertices, mesh.triangles, N, 0))
    pts, _, nrm, which, _ = TM.device_sample(eng, state["v"], state["t"], N, 0, want_triangle=True)
    equal["sample"] = bits_equal(pts.cpu().numpy(), want["points"]) and bits_equal(which.cpu().numpy(), want["triangle"]) and bits_equal(nrm.cpu().numpy(), want["normals"])
    dev_ms["sample"], dev_ms["sample_all"] = timed(torch, lambda: TM.device_sample(eng, state["v"], state["t"], N, 0), a.repeats)
    sizes["sample"] = [N]
    V, T = int(state["v"].shape[0]), int(state["t"].shape[0])
    count_end = torch.empty(T, dtype=torch.int64, device=dev)
    from icepy4d_amd._lib import ptr
    out3 = [torch.empty((N, 3), dtype=torch.float64, device=dev) for _ in range(2)]
    dev_ms["sample_table_only"], _ = timed(torch, lambda: eng.ctx.call("im_mesh_sample_table", ptr(state["v"]), V, ptr(state["t"]), T, N, None, ptr(count_end), None,
                                                                     eng.stream_ptr()), a.repeats)
    dev_ms["sample_kernel_only"], _ = timed(torch, lambda: eng.ctx.call("im_mesh_sample", ptr(state["v"]), V, ptr(state["t"]), T, ptr(count_end), N, 0, None, None,
                                                                      ptr(out3[0]), None, ptr(out3[1]), None, eng.stream_ptr()), a.repeats)
    names = ["density_filter", "degenerate", "duplicated_triangles", "duplicated_vertices", "non_manifold_census", "hull_filter", "sample"]
    res.update({"after_each_step_vertices_triangles": sizes, "equal_to_oracle": equal, "device_ms": {k: round(x, 3) if isinstance(x, float) else x for k, x in dev_ms.items()},
                "oracle_cpu_s": host_s, "device_total_ms": round(sum(dev_ms[k] for k in names), 3), "oracle_total_s": round(sum(host_s[k] for k in names), 3)})
    # the sample kernel writes 48 B per sample (points and normals) and reads, per sample, about log2(T) table entries (cached: neighbouring
    # samples walk the same path), 12 B of indices and 72 B of vertices through them
    res["sample_kernel_bytes_written_per_s"] = round(48 * N / (dev_ms["sample_kernel_only"] * 1e-3))
    res["not_determined"] = ("no counter run was made: what bounds mesh_sample_kernel is unmeasured; from reading the code the candidate is the gather of three vertices "
                             "per sample through the triangle index")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not all(equal.values()):
        sys.exit(f"the device output differs from the restatement at the production size: {equal}")


if __name__ == "__main__":
    main()
