"""Times the semi-global regularisation of a depth map (csrc/dense_sgm.hip) on the device (device events, one warm-up, median of the
repeats) on the 24 MP synthetic pair of tools/bench_dense.py at downscale 4 and at downscale 2, with the schedule's own number of planes:
  - per downscale, for view 0: `im_dense_costs`, `im_dense_sgm` with eight and with four paths, `im_dense_sgm_choose`, and beside them
    the winner-take-all `im_dense_sweep` timed in the same run; the bytes of the two volumes;
  - the share of pixels either map keeps and the median error of the kept inverse depths in plane steps (the scene is clean: what the
    regularisation gains on noise is pinned in tests/test_sgm_cpu.py, not here);
  - the numpy restatement (tests/sgm_oracle.py) on a 256 x 256 crop with the same schedule, which the device's output on that crop is
    compared with first (bits).
What bounds `im_dense_sgm` - the chain of cross-lane operations behind every pixel of a line, the number of lines in flight or the traffic
of the sums - is NOT measured here (that takes a counter run of its own). No time is asserted and no target is set.

    python tools/bench_sgm.py [--repeats 5] [--out profiles/r22_sgm_bench.json]"""
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
from bench_dense import D_FAR, D_NEAR, F, H, MARGIN, W, Cam, synthetic_pair  # noqa: E402
from bench_pointcloud import timed  # noqa: E402

P1, P2 = 16, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_sgm_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sgm.py needs a HIP device: there is nothing to time without one")
    import sgm_oracle as S
    from icepy4d_amd import dense as D
    from icepy4d_amd.engine import Engine, to_device
    eng = Engine(0)
    im0, im1, disp = synthetic_pair()
    K0 = np.array([[F, 0.0, W / 2.0], [0.0, F, H / 2.0], [0.0, 0.0, 1.0]])
    K1 = K0.copy()
    K1[0, 2] += MARGIN
    cams = [Cam(K0, np.eye(3), np.zeros(3), W, H), Cam(K1, np.eye(3), np.array([-1.0, 0.0, 0.0]), W + MARGIN, H)]
    rng = (F / (D_FAR + 8.0), F / (D_NEAR - 8.0))
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "image": [H, W], "radius": 3, "min_score": 0.8, "min_var": 4, "P1": P1, "P2": P2,
           "scene": f"tools/bench_dense.py's pair: seeded texture, a front slanted along v with {D_NEAR}..{D_FAR} px of disparity at full size; "
                    f"depth range {rng[0]:.2f}..{rng[1]:.2f}",
           "clock": "device events around the calls, one warm-up, median of the repeats; view 0",
           "unmeasured": "what bounds im_dense_sgm (the cross-lane chain behind every pixel of a line, the lines in flight or the traffic of the sums): "
                         "no counter run was made",
           "downscale": {}}
    d_im = [to_device(im0, eng.device), to_device(im1, eng.device)]
    equal_all = True
    for f in (4, 2):
        maps = D.build_depth_maps(d_im, cams, depth_range=rng, downscale=f, engine=eng)
        m, o = maps[0], maps[1]
        small = [D._SmallCam(x.K, x.R, x.t) for x in maps]
        A, B = D.sweep_matrices(m.K, o.K, *D.relative_pose(small[0], small[1]))
        h0, w0 = m.plane.shape
        planes = m.schedule[2]
        r = {"map_shape": [h0, w0], "planes": planes, "cost_bytes": h0 * w0 * planes, "sum_bytes": 2 * h0 * w0 * planes}
        r["sweep_winner_take_all_ms"], r["sweep_winner_take_all_ms_all"] = timed(torch, lambda: D.sweep(m.grey, o.grey, A, B, *m.schedule, 3, 4, 0.8, engine=eng),
                                                                             a.repeats)
        r["costs_ms"], r["costs_ms_all"] = timed(torch, lambda: D.cost_volume(m.grey, o.grey, A, B, *m.schedule, 3, 4, engine=eng), a.repeats)
        cost = D.cost_volume(m.grey, o.grey, A, B, *m.schedule, 3, 4, engine=eng)
        r["aggregate_8_paths_ms"], r["aggregate_8_paths_ms_all"] = timed(torch, lambda: D.sgm_aggregate(cost, P1, P2, 8, engine=eng), a.repeats)
        r["aggregate_4_paths_ms"], r["aggregate_4_paths_ms_all"] = timed(torch, lambda: D.sgm_aggregate(cost, P1, P2, 4, engine=eng), a.repeats)
        total = D.sgm_aggregate(cost, P1, P2, 8, engine=eng)
        r["choose_ms"], r["choose_ms_all"] = timed(torch, lambda: D.sgm_choose(cost, total, m.schedule[0], m.schedule[1], 0.8, engine=eng), a.repeats)
        r["regularised_total_ms"] = round(r["costs_ms"] + r["aggregate_8_paths_ms"] + r["choose_ms"], 3)
        r["aggregate_8_paths_giga_plane_steps_per_s"] = round(8 * h0 * w0 * planes / r["aggregate_8_paths_ms"] / 1e6, 2)
        plane, w, _ = D.sgm_choose(cost, total, m.schedule[0], m.schedule[1], 0.8, engine=eng)
        del total
        rows = (np.arange(h0) * f + (f - 1) / 2.0)
        truth = (D_NEAR + (D_FAR - D_NEAR) * rows / (H - 1.0)) / F
        for name, (pl, wm) in (("winner_take_all", (m.plane, m.w)), ("regularised", (plane, w))):
            k = pl.cpu().numpy() >= 0
            err = np.abs(wm.cpu().numpy() - truth[:, None])[k] / m.schedule[1]
            r[name + "_share_kept"] = round(float(k.mean()), 4)
            r[name + "_error_in_plane_steps_median_p99"] = [round(float(np.median(err)), 4), round(float(np.percentile(err, 99)), 4)]
        # the restatement on a crop, for scale and as a check at this size
        c = 256
        y0, x0 = (h0 - c) // 2, (w0 - c) // 2
        g0, g1 = m.grey.cpu().numpy(), o.grey.cpu().numpy()
        T = np.array([[1.0, 0.0, x0], [0.0, 1.0, y0], [0.0, 0.0, 1.0]])                 # crop pixel -> map pixel
        Ac, Bc = (A.reshape(3, 3) @ T).reshape(9), (B.reshape(3, 3) @ T).reshape(9)
        crop = np.ascontiguousarray(g0[y0:y0 + c, x0:x0 + c])
        t0 = time.perf_counter()
        want = S.sweep(crop, g1, Ac, Bc, *m.schedule, 3, 4, 0.8, P1, P2, 8)
        r["numpy_restatement_256x256_crop_s"] = round(time.perf_counter() - t0, 3)
        run = lambda: D.sweep(to_device(crop, eng.device), o.grey, Ac, Bc, *m.schedule, 3, 4, 0.8, engine=eng, regularisation="sgm", p1=P1, p2=P2, paths=8)  # noqa: E731
        got = run()
        r["device_256x256_crop_ms"], _ = timed(torch, run, a.repeats)
        equal = all(np.array_equal(g.cpu().numpy().view(np.uint8), x.view(np.uint8)) for g, x in zip(got, want))
        r["crop_equal_to_the_restatement"] = bool(equal)
        equal_all = equal_all and equal
        res["downscale"][str(f)] = r
        del cost, maps, m, o, plane, w
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not equal_all:
        sys.exit("the device output differs from the restatement at the production size")


if __name__ == "__main__":
    main()
