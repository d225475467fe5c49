"""Times the ICP co-registration of csrc/icp.hip on the device (device events, one warm-up, median of the repeats) between two synthetic
glacier fronts of `--points` points each (default 2 M): the front of tests/ball_cases.py scaled up to 200 m x 400 m in a world frame; the
source is a second, independently sampled epoch moved by the inverse of a known small motion (0.05 degrees about an axis through the
middle of the front and a shift of (0.15, -0.10, 0.08) m). Point to plane, d_max 1 m, the target's normals from the ball of 1 m, with
100 k source points and with all of them:
  - per iteration, at the initial transform: the transform (`im_transform_points`), the search (`knn_cross`, k = 1 within d_max: the
    whole call with its query sort, and gather + kernel alone), the accumulate pass (`im_icp_accumulate`) and finish + read-back
    (`im_icp_finish` and the download of the record);
  - the whole `registration_icp` on a target binned beforehand with its normals given, the iterations to convergence, fitness and rmse;
  - the recovered motion's error: the largest distance, over the source points, between the recovered and the known transform (the two
    epochs are sampled independently, so it is not zero).
Before timing, the partials of `--check` chunks are compared with the restatement (tests/icp_oracle.py: bits).
What bounds the accumulate pass is NOT measured here (that takes a counter run of its own); it gathers about 84 B per point, which is
reasoning and not a measurement. No time is asserted.

    python tools/bench_registration.py [--points 2000000] [--repeats 5] [--out profiles/r19_registration_bench.json]"""
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
ANGLE_DEG, AXIS, SHIFT = 0.05, (0.3, -0.5, 0.8), (0.15, -0.10, 0.08)
D_MAX, NORMAL_RADIUS, SUBSET = 1.0, 1.0, 100_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_registration_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.points >= 1000
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_registration.py needs a HIP device: there is nothing to time without one")
    import ball_cases as BC
    import icp_cases as IC
    import icp_oracle as O
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.post_processing import registration as R
    from icepy4d_amd.utils import point_cloud_filters as F
    eng = Engine(0)
    dev, st = eng.device, eng.stream_ptr()
    n = a.points
    middle = np.asarray(ORIGIN) + (0.3 * SIZE[0], 0.5 * SIZE[1], 0.3 * SIZE[0])
    M_true = IC.motion(ANGLE_DEG, AXIS, SHIFT, about=middle)
    Minv = np.linalg.inv(M_true)
    host_t = BC.front(n, seed=51, size=SIZE, origin=ORIGIN)
    host_s = np.ascontiguousarray(BC.front(n, seed=52, size=SIZE, origin=ORIGIN) @ Minv[:3, :3].T + Minv[:3, 3])
    res = {"device": torch.cuda.get_device_name(0), "points": n, "repeats": a.repeats, "d_max": D_MAX, "normal_radius": NORMAL_RADIUS,
           "clouds": f"tests/ball_cases.py front, size {SIZE}, seeds 51 (target) / 52 (source, moved by the inverse of {ANGLE_DEG} degrees about "
                     f"{AXIS} through the middle and {SHIFT})",
           "clock": "device events around the calls, one warm-up, median of the repeats",
           "unmeasured": "what bounds im_icp_accumulate (the gather of about 84 B per point is reasoning): no counter run was made", "runs": {}}
    ok = True
    tgt = torch.from_numpy(host_t).to(dev)
    tb = F.bin_cloud(tgt, D_MAX, engine=eng)
    res["normals_ms"], _ = timed(torch, lambda: F.ball_cross(tb.pts, None, NORMAL_RADIUS, want=("normal",), engine=eng, binned=tb), a.repeats)
    nrm = F.ball_cross(tb.pts, None, NORMAL_RADIUS, want=("normal",), engine=eng, binned=tb)["normal"].contiguous()
    host_n = nrm.cpu().numpy()
    lo, hi = F._bounds(tb.pts)
    centre = np.ascontiguousarray((lo + hi) / np.float64(2.0))
    chunk = R.icp_chunk()
    rng = np.random.default_rng(19)
    for tag, m in ((f"{SUBSET // 1000}k", min(SUBSET, n)), ("all", n)):
        sel = np.sort(rng.choice(n, m, replace=False)) if m < n else np.arange(n)
        hs = np.ascontiguousarray(host_s[sel])
        src = torch.from_numpy(hs).to(dev)
        p, chunks = torch.empty_like(src), -(-m // chunk)
        d_M = torch.from_numpy(np.eye(4).reshape(16)).to(dev)
        rec = torch.zeros(R.RECORD, dtype=torch.float64, device=dev)
        parts = torch.empty((chunks, 32), dtype=torch.float64, device=dev)
        run = {"source_points": m, "chunks": chunks}

        def transform():
            eng.ctx.call("im_transform_points", ptr(d_M), ptr(src), ptr(p), m, 0, st)

        transform()
        order = F.query_order(eng, p, tb)
        idx, d2 = torch.empty((m, 1), dtype=torch.int32, device=dev), torch.empty((m, 1), dtype=torch.float64, device=dev)

        def search_kernel():
            eng.ctx.call("im_knn_cross", *F._target_args(tb), ptr(p), ptr(order), m, 1, D_MAX * D_MAX, None, ptr(idx), ptr(d2), None, st)

        def accumulate(out=None):
            eng.ctx.call("im_icp_accumulate", ptr(p), m, ptr(tb.pts), ptr(nrm), n, ptr(idx), ptr(d2), centre.ctypes.data, 1, chunks, out, st)

        def finish():
            eng.ctx.call("im_icp_finish", None, m, chunks, ptr(d_M), centre.ctypes.data, 1, ptr(rec), st)
            return rec.cpu()

        search_kernel()
        accumulate(ptr(parts))
        hp, hidx, hd2 = p.cpu().numpy(), idx.cpu().numpy().reshape(-1), d2.cpu().numpy().reshape(-1)
        got = parts.cpu().numpy()
        equal = True
        for ch in rng.integers(0, chunks, a.check):
            s = slice(ch * chunk, min((ch + 1) * chunk, m))
            want = O.partials(hp[s], host_t, host_n, hidx[s], hd2[s], centre, O.POINT_TO_PLANE)
            equal = equal and np.array_equal(got[ch].view(np.uint64), want[0].view(np.uint64))
        run["checked_chunks"], run["equal_to_the_restatement"] = int(a.check), bool(equal)
        ok = ok and equal
        run["transform_ms"], run["transform_ms_all"] = timed(torch, transform, a.repeats)
        run["search_whole_ms"], run["search_whole_ms_all"] = timed(
            torch, lambda: F.knn_cross(p, None, 1, radius=D_MAX, want=("idx", "d2"), engine=eng, binned=tb), a.repeats)
        run["search_kernel_ms"], run["search_kernel_ms_all"] = timed(torch, search_kernel, a.repeats)
        run["accumulate_ms"], run["accumulate_ms_all"] = timed(torch, accumulate, a.repeats)
        run["finish_readback_ms"], run["finish_readback_ms_all"] = timed(torch, finish, a.repeats)
        kw = dict(target_normals=nrm, engine=eng)
        r = R.registration_icp(src, tb, D_MAX, **kw)
        run["whole_ms"], run["whole_ms_all"] = timed(torch, lambda: R.registration_icp(src, tb, D_MAX, **kw), a.repeats)
        run["iterations"], run["converged"], run["status"] = int(r.iterations), bool(r.converged), r.status
        run["fitness"], run["inlier_rmse"] = [float(v) for v in r.history[:, R.REC_FITNESS]], [float(v) for v in r.history[:, R.REC_RMSE]]
        run["ms_per_iteration"] = round(run["whole_ms"] / (r.iterations + 1), 3)
        T = r.transformation.cpu().numpy()
        err = np.sqrt(((O.apply(T, hs) - O.apply(M_true, hs)) ** 2).sum(1))
        run["motion_error_max_m"], run["motion_error_mean_m"] = float(err.max()), float(err.mean())
        run["initial_offset_mean_m"] = float(np.sqrt(((hs - O.apply(M_true, hs)) ** 2).sum(1)).mean())
        res["runs"][tag] = run
        print(f"{tag}: transform {run['transform_ms']:.3f} ms, search {run['search_whole_ms']:.2f} ms (kernel {run['search_kernel_ms']:.2f}), "
              f"accumulate {run['accumulate_ms']:.3f} ms, finish + read-back {run['finish_readback_ms']:.3f} ms; whole {run['whole_ms']:.1f} ms, "
              f"{run['iterations']} iterations, converged {run['converged']}, rmse {run['inlier_rmse'][-1]:.4f}, motion error max "
              f"{run['motion_error_max_m']:.4f} m, equal {equal}", flush=True)
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
