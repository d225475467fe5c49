"""Times two-view dense stereo (csrc/dense.hip) on the device (device events, one warm-up, median of the repeats) on a 24 MP synthetic
pair at downscale 4 and at downscale 2, with the schedule's own number of planes:
  - view 1 is a seeded texture, 4000 x 6000 plus a margin; view 0 sees a front slanted along v, every row of it shifted by a whole
    number of pixels (60 .. 200 px: 30 .. 100 m at f = 6000 px and a baseline of 1 m), so that the pair costs seconds to make;
  - per downscale: `im_dense_sweep` of either view, `im_dense_consistency` (ModerateFiltering), `im_dense_cloud` with its read-back of one
    count, the share of pixels kept and the median error of the kept inverse depths in plane steps;
  - for scale, the numpy restatement (tests/dense_oracle.py) on a 256 x 256 crop with the same schedule on this host, which the device's
    output on that crop is compared with first (bits).
What bounds `im_dense_sweep` - the gather of the other view, the float64 of the coordinates or the box sums through LDS - is NOT measured here
(that takes a counter run of its own). No time is asserted and no target is set.

    python tools/bench_dense.py [--repeats 5] [--out profiles/r21_dense_bench.json]"""
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

H, W, F, MARGIN = 4000, 6000, 6000.0, 256
D_NEAR, D_FAR = 60, 200            # disparities of the front, pixels at full size


def synthetic_pair(seed=7):
    """(im0 [H, W], im1 [H, W + MARGIN], disparity per row [H]) uint8."""
    import dense_cases as DC
    tile = DC.texture(seed, 500, 500)
    im1 = np.tile(tile, (H // 500, (W + MARGIN) // 500 + 1))[:, :W + MARGIN]
    rng = np.random.default_rng(seed)
    im1 = np.clip(im1.astype(np.int16) + rng.integers(-20, 21, im1.shape, dtype=np.int16), 0, 255).astype(np.uint8)     # the tiles differ
    disp = np.rint(D_NEAR + (D_FAR - D_NEAR) * np.arange(H) / (H - 1.0)).astype(np.int64)
    im0 = np.empty((H, W), np.uint8)
    for v in range(H):
        im0[v] = im1[v, MARGIN - disp[v]:MARGIN - disp[v] + W]
    return im0, im1, disp


class Cam:
    def __init__(self, K, R, t, w, h):
        self.K, self.R, self.t, self.width, self.height, self.dist = K, R, t, w, h, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_dense_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_dense.py needs a HIP device: there is nothing to time without one")
    import dense_oracle as O
    from icepy4d_amd import dense as D
    from icepy4d_amd.engine import Engine, to_device
    eng = Engine(0)
    im0, im1, disp = synthetic_pair()
    # u1 = u0 - d + MARGIN: X1 = X0 + (-1, 0, 0), cx1 = cx0 + MARGIN, d = F w
    K0 = np.array([[F, 0.0, W / 2.0], [0.0, F, H / 2.0], [0.0, 0.0, 1.0]])
    K1 = K0.copy()
    K1[0, 2] += MARGIN
    cams = [Cam(K0, np.eye(3), np.zeros(3), W, H), Cam(K1, np.eye(3), np.array([-1.0, 0.0, 0.0]), W + MARGIN, H)]
    rng = (F / (D_FAR + 8.0), F / (D_NEAR - 8.0))
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "image": [H, W], "radius": 3, "min_score": 0.8, "min_var": 4,
           "scene": f"seeded texture, a front slanted along v with {D_NEAR}..{D_FAR} px of disparity at full size, f = {F:.0f} px, baseline 1; "
                    f"depth range {rng[0]:.2f}..{rng[1]:.2f}",
           "clock": "device events around the calls, one warm-up, median of the repeats",
           "unmeasured": "what bounds im_dense_sweep (the gather of the other view, the float64 coordinates or the LDS box sums): no counter run was made",
           "downscale": {}}
    d_im = [to_device(im0, eng.device), to_device(im1, eng.device)]
    equal_all = True
    for f in (4, 2):
        maps = D.build_depth_maps(d_im, cams, depth_range=rng, downscale=f, engine=eng)
        r = {"map_shape": [list(m.plane.shape) for m in maps], "planes": [m.schedule[2] for m in maps]}
        small = [D._SmallCam(m.K, m.R, m.t) for m in maps]
        for v in (0, 1):
            m, o = maps[v], maps[1 - v]
            A, B = D.sweep_matrices(m.K, o.K, *D.relative_pose(small[v], small[1 - v]))
            run = lambda: D.sweep(m.grey, o.grey, A, B, *m.schedule, 3, 4, 0.8, engine=eng)  # noqa: E731
            r[f"sweep_view{v}_ms"], r[f"sweep_view{v}_ms_all"] = timed(torch, run, a.repeats)
            px = m.plane.numel() * m.schedule[2]
            r[f"sweep_view{v}_gigasamples_per_s"] = round(px / r[f"sweep_view{v}_ms"] / 1e6, 2)
        r["consistency_ms"], r["consistency_ms_all"] = timed(torch, lambda: D.consistency(maps[0], maps[1], "ModerateFiltering", engine=eng), a.repeats)
        keep = D.consistency(maps[0], maps[1], "ModerateFiltering", engine=eng)
        r["cloud_with_count_readback_ms"], r["cloud_with_count_readback_ms_all"] = timed(torch, lambda: D.cloud_of(maps[0], keep, engine=eng), a.repeats)
        r["points"] = int(keep.sum().item())
        r["share_kept"] = round(r["points"] / keep.numel(), 4)
        k = keep.cpu().numpy() != 0
        w = maps[0].w.cpu().numpy()
        rows = (np.arange(k.shape[0]) * f + (f - 1) / 2.0)
        truth = (D_NEAR + (D_FAR - D_NEAR) * rows / (H - 1.0)) / F
        err = np.abs(w - truth[:, None])[k] / maps[0].schedule[1]
        r["error_in_plane_steps_median_p99"] = [round(float(np.median(err)), 4), round(float(np.percentile(err, 99)), 4)]
        # the restatement on a crop, for scale and as a check at this size
        c = 256
        y0, x0 = (k.shape[0] - c) // 2, (k.shape[1] - c) // 2
        g0, g1 = maps[0].grey.cpu().numpy(), maps[1].grey.cpu().numpy()
        A, B = D.sweep_matrices(maps[0].K, maps[1].K, *D.relative_pose(small[0], small[1]))
        T = np.array([[1.0, 0.0, x0], [0.0, 1.0, y0], [0.0, 0.0, 1.0]])                 # crop pixel -> map pixel
        Ac, Bc = (A.reshape(3, 3) @ T).reshape(9), (B.reshape(3, 3) @ T).reshape(9)
        crop = np.ascontiguousarray(g0[y0:y0 + c, x0:x0 + c])
        t0 = time.perf_counter()
        want = O.sweep(crop, g1, Ac, Bc, *maps[0].schedule, 3, 4, 0.8)
        r["numpy_restatement_256x256_crop_s"] = round(time.perf_counter() - t0, 3)
        got = D.sweep(to_device(crop, eng.device), maps[1].grey, Ac, Bc, *maps[0].schedule, 3, 4, 0.8, engine=eng)
        r["device_256x256_crop_ms"], _ = timed(torch, lambda: D.sweep(to_device(crop, eng.device), maps[1].grey, Ac, Bc, *maps[0].schedule, 3, 4, 0.8, engine=eng),
                                               a.repeats)
        equal = all(np.array_equal(g.cpu().numpy().view(np.uint8), x.view(np.uint8)) for g, x in zip(got, want))
        r["crop_equal_to_the_restatement"] = bool(equal)
        equal_all = equal_all and equal
        res["downscale"][str(f)] = r
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not equal_all:
        sys.exit("the device output differs from the restatement at the production size")


if __name__ == "__main__":
    main()
