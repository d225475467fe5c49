"""Times the reconstruction kernels of csrc/sfm.hip on the device (device events, every shape warmed up, median of the repeats):

  table   the config-4 match table (2048 epochs x 4096 keypoints, about half of them matched, seeded): `im_triangulate_table` with and
          without the fused undistortion, and the colouring of its points (`im_project_colors` on a 24 MP image)
  flat    one production call's worth of points (15 tile pairs x 8196): `im_triangulate_iterative` with the fused undistortion,
          `im_undistort_points` alone

and, on the host, the numpy restatement (tests/sfm_oracle.py) on a sample: a PORT of the reference's per-point loop to whole arrays, not
the reference's own run time. Bytes are counted from the shapes (what the kernels must read and write once) and set against the 6.3 TB/s
copy rate DESIGN uses; the kernels are arithmetic-bound, so that ratio says how far from a copy they are, not how good they are.

    python tools/bench_sfm.py [--epochs 2048] [--kpts 4096] [--repeats 7] [--out profiles/r09_sfm_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
COPY_RATE = 6.3e12


def rig():
    """The fixture's two cameras (the reference's calibrations on a 140 m baseline)."""
    import types
    import sfm_oracle as S
    g = S.load_g13(os.path.join(ROOT, "tests", "golden", "g13_sfm.npz"))
    cams = []
    for k, ext in (("0", g["ro_cam0_extrinsics"]), ("1", g["ro_cam1_extrinsics"])):
        cams.append(types.SimpleNamespace(K=g["K" + k], dist=g["dist" + k], R=ext[:3, :3], t=ext[:3, 3:4], P=g["P" + k]))
    return g, cams


def scene(rng, g, n):
    """n matched float32 keypoint pairs: the fixture's world points resampled with jitter and projected with distortion."""
    from dsm_oracle import project_points_f64
    base = g["world_points"][:5000]
    X = base[rng.integers(0, len(base), n)] + rng.normal(0, 2.0, (n, 3))
    out = []
    for k, ext in (("0", g["ro_cam0_extrinsics"]), ("1", g["ro_cam1_extrinsics"])):
        uv = project_points_f64(X, g["K" + k], g["dist" + k], ext[:3, :3], ext[:3, 3])
        out.append((uv + 0.5 * rng.normal(size=uv.shape)).astype(np.float32))
    return out


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
    return float(np.median(ms)), [round(m, 4) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2048)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--oracle-sample", type=int, default=4000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5 and a.oracle_sample >= 2000
    import torch
    import sfm_oracle as S
    from icepy4d_amd import sfm
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine
    if not torch.cuda.is_available():
        sys.exit("bench_sfm.py needs a HIP device: there is nothing to time without one")
    eng = Engine(0)
    dev = eng.device
    g, cams = rig()
    rng = np.random.default_rng(9)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "copy_rate_bytes_per_s": COPY_RATE, "shapes": {}}

    def report(name, ms, all_ms, points, nbytes, **extra):
        res["shapes"][name] = dict(ms=round(ms, 4), ms_all=all_ms, points=int(points), points_per_s=points / (ms * 1e-3),
                                   bytes=int(nbytes), ms_at_copy_rate=round(nbytes / COPY_RATE * 1e3, 5),
                                   times_the_copy_bound=round(ms / (nbytes / COPY_RATE * 1e3), 1), **extra)
        print(f"{name:34s} {ms:9.3f} ms  {points / (ms * 1e-3) / 1e6:9.1f} Mpoints/s  {nbytes / 1e6:9.1f} MB  "
              f"({nbytes / COPY_RATE * 1e3:.4f} ms at the copy rate)", flush=True)

    # ---- the gathered table, built on the device from one pool of matched pairs
    E, K = a.epochs, a.kpts
    W = 8 + 6 * K
    pool0, pool1 = scene(rng, g, 1 << 20)
    gen = torch.Generator(device="cpu").manual_seed(9)
    table = torch.full((E, W), -1, dtype=torch.int32)
    table[:, 8 + K:] = 0
    matched = torch.rand((E, K), generator=gen) < 0.5
    perm = torch.argsort(torch.rand((E, K), generator=gen), dim=1).to(torch.int32)      # a permutation of the keypoints of image 1 per epoch
    table[:, 8:8 + K] = torch.where(matched, perm, torch.full_like(perm, -1))
    pick = torch.randint(0, len(pool0), (E, K), generator=gen)
    k0 = torch.from_numpy(pool0)[pick]                                                   # [E, K, 2]
    k1 = torch.empty_like(k0)
    k1.scatter_(1, perm.long()[:, :, None].expand(-1, -1, 2), torch.from_numpy(pool1)[pick])   # the partner of keypoint i sits at perm[i]
    table[:, 8 + 2 * K:8 + 4 * K] = k0.reshape(E, 2 * K).view(torch.int32)
    table[:, 8 + 4 * K:] = k1.reshape(E, 2 * K).view(torch.int32)
    table[:, 0] = torch.arange(E, dtype=torch.int32)
    table[:, 1] = K
    table[:, 2] = K
    table[:, 3] = matched.sum(1).to(torch.int32)
    table[:, 4:8] = 0
    M = int(matched.sum())
    dt = table.to(dev)
    dcams = torch.from_numpy(sfm._camera_table(cams, E)).to(dev)
    doff = torch.empty(E + 1, dtype=torch.int64, device=dev)
    dX = torch.empty((M, 3), dtype=torch.float64, device=dev)
    dst = torch.empty(M, dtype=torch.int32, device=dev)
    res["table"] = dict(epochs=E, max_kpts=K, matched_points=M, table_bytes=int(table.numel() * 4))
    # read: the headers + matches0 of every record, the two keypoints of every match; written: X, status, offsets
    moved = E * (8 + K) * 4 + M * 16 + M * (24 + 4) + (E + 1) * 8
    for und in (1, 0):
        ms, all_ms = timed(torch, lambda: eng.ctx.call("im_triangulate_table", ptr(dt), E, K, ptr(dcams), 1, und, 3e-5, 10, M, ptr(doff),
                                                       ptr(dX), ptr(dst), None, None, eng.stream_ptr()), a.repeats)
        report("table_undistort" if und else "table_no_undistort", ms, all_ms, M, moved)
    assert int(doff[-1].item()) == M
    st = dst.cpu().numpy()
    res["table"]["status_counts"] = {str(k): int((st == k).sum()) for k in np.unique(st)}
    image = torch.from_numpy(S.image_pattern(4008, 6012)).to(dev)
    cam = sfm._camera_params(cams[1])
    chmap = np.array([2, 1, 0], np.int32)
    ms, all_ms = timed(torch, lambda: sfm._project_colors_device(eng, dX, cam, image, chmap, want_proj=False), a.repeats)
    report("table_colours", ms, all_ms, M, M * 24 + M * 24 + M * 4 * 3 * 4, note="includes the allocation of the colour array")

    # ---- one production call: 15 tile pairs x 8196 keypoints
    n = 15 * 8196
    f0, f1 = scene(rng, g, n)
    d0, d1 = torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)
    fX = torch.empty((n, 3), dtype=torch.float64, device=dev)
    fst = torch.empty(n, dtype=torch.int32, device=dev)
    P0, P1, i0, i1 = sfm._projection(cams[0]), sfm._projection(cams[1]), sfm._intrinsics(cams[0]), sfm._intrinsics(cams[1])
    ms, all_ms = timed(torch, lambda: eng.ctx.call("im_triangulate_iterative", ptr(d0), ptr(d1), 0, n, P0.ctypes.data, P1.ctypes.data,
                                                   i0.ctypes.data, i1.ctypes.data, 3e-5, 10, ptr(fX), ptr(fst), None, None, eng.stream_ptr()),
                       a.repeats)
    report("flat_fused_15x8196", ms, all_ms, n, n * (16 + 24 + 4))
    ms, all_ms = timed(torch, lambda: eng.ctx.call("im_triangulate_iterative", ptr(d0), ptr(d1), 0, n, P0.ctypes.data, P1.ctypes.data,
                                                   None, None, 3e-5, 1, ptr(fX), ptr(fst), None, None, eng.stream_ptr()), a.repeats)
    report("flat_linear_one_solve_15x8196", ms, all_ms, n, n * (16 + 24 + 4))
    du = torch.empty_like(d0)
    ms, all_ms = timed(torch, lambda: eng.ctx.call("im_undistort_points", ptr(d0), n, i0.ctypes.data, ptr(du), eng.stream_ptr()), a.repeats)
    report("undistort_15x8196", ms, all_ms, n, n * 16)

    # ---- the numpy restatement on the host, a sample of the same points
    m = a.oracle_sample
    t0 = time.perf_counter()
    u0, u1 = S.undistort_points_f64(f0[:m], cams[0].K, cams[0].dist), S.undistort_points_f64(f1[:m], cams[1].K, cams[1].dist)
    Xo, so = S.triangulate_iterative(u0, cams[0].P, u1, cams[1].P)
    dt_o = time.perf_counter() - t0
    res["oracle_port"] = dict(points=m, seconds=round(dt_o, 4), us_per_point=round(dt_o / m * 1e6, 3),
                              note="numpy restatement on whole arrays (tests/sfm_oracle.py), a port: not the reference's per-point Python loop")
    eng.ctx.call("im_triangulate_iterative", ptr(d0), ptr(d1), 0, n, P0.ctypes.data, P1.ctypes.data, i0.ctypes.data, i1.ctypes.data, 3e-5, 10,
                 ptr(fX), ptr(fst), None, None, eng.stream_ptr())
    agree = np.linalg.norm(fX[:m].cpu().numpy() - Xo, axis=1) / np.maximum(1.0, np.linalg.norm(Xo, axis=1))
    res["oracle_port"]["max_relative_difference_to_device"] = float(agree.max())
    res["oracle_port"]["status_equal"] = bool(np.array_equal(fst[:m].cpu().numpy(), so))
    print(f"oracle port: {dt_o / m * 1e6:.2f} us per point on {m} points; device vs port {agree.max():.2e}", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
