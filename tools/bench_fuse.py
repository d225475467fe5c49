"""Times the fusion of the two depth maps (csrc/dense_fuse.hip) on the device (device events, one warm-up, median of the repeats) on the 24 MP
synthetic pair of tools/bench_dense.py at downscale 4 and at downscale 2, on the winner-take-all maps and on the semi-global maps, both
keep masks under ModerateFiltering, view 0 the base, a tolerance of one plane step:
  - `im_dense_fuse_link` and `im_dense_fuse_rest` on outputs allocated once, the whole `dense.fuse` (its allocations included), and beside
    them the sweep that made view 0's map, timed in the same run; per launch, the library's own events;
  - the numbers of kept, linked, claimed and rest pixels, and the point counts of the fused and of the concatenated cloud;
  - at downscale 4 the device's outputs are compared with the numpy restatement (tests/fuse_oracle.py) on the whole map first (bits).
What bounds the link kernel - the gathers from view b's three maps, the float64 divisions or the stores - is NOT measured here (that takes
a counter run of its own). No time is asserted and no target is set.

    python tools/bench_fuse.py [--repeats 5] [--out profiles/r24_fuse_bench.json]"""
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
from bench_depth_clean import launches  # noqa: E402
from bench_pointcloud import timed  # noqa: E402

TOL, FILTER = 1.0, "ModerateFiltering"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_fuse_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fuse.py needs a HIP device: there is nothing to time without one")
    import fuse_oracle as FO
    from icepy4d_amd import dense as D
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine, to_device
    eng = Engine(0)
    im0, im1, _ = synthetic_pair()
    K0 = np.array([[F, 0.0, W / 2.0], [0.0, F, H / 2.0], [0.0, 0.0, 1.0]])
    K1 = K0.copy()
    K1[0, 2] += MARGIN
    cams = [Cam(K0, np.eye(3), np.zeros(3), W, H), Cam(K1, np.eye(3), np.array([-1.0, 0.0, 0.0]), W + MARGIN, H)]
    rng = (F / (D_FAR + 8.0), F / (D_NEAR - 8.0))
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "image": [H, W], "radius": 3, "min_score": 0.8, "min_var": 4,
           "depth_filter": FILTER, "tol_plane_steps": TOL, "base_view": 0,
           "scene": f"tools/bench_dense.py's pair: seeded texture, a front slanted along v with {D_NEAR}..{D_FAR} px of disparity at full size; "
                    f"depth range {rng[0]:.2f}..{rng[1]:.2f}",
           "clock": "device events around the calls, one warm-up, median of the repeats; link_ms and rest_ms on outputs allocated once (the clear of "
                    "the claims is part of link_ms), fuse_whole_ms with the allocations of `dense.fuse`",
           "unmeasured": "what bounds the link kernel (the gathers from view b's maps, the float64 divisions or the stores): no counter run was made",
           "downscale": {}}
    d_im = [to_device(im0, eng.device), to_device(im1, eng.device)]
    equal_all = True
    for f in (4, 2):
        r = {}
        for kind, extra in (("winner_take_all", {}), ("semi_global", dict(regularisation="sgm"))):
            maps = D.build_depth_maps(d_im, cams, depth_range=rng, downscale=f, engine=eng, **extra)
            m, o = maps[0], maps[1]
            small = [D._SmallCam(x.K, x.R, x.t) for x in maps]
            A, B = D.sweep_matrices(m.K, o.K, *D.relative_pose(small[0], small[1]))
            (ha, wa), (hb, wb) = m.plane.shape, o.plane.shape
            q = {"map_shapes": [[ha, wa], [hb, wb]], "planes": [m.schedule[2], o.schedule[2]]}
            q["sweep_ms"], q["sweep_ms_all"] = timed(torch, lambda: D.sweep(m.grey, o.grey, A, B, *m.schedule, 3, 4, 0.8, engine=eng, **extra), a.repeats)
            keep = [D.consistency(maps[v], maps[1 - v], FILTER, engine=eng) for v in (0, 1)]
            ab, ba = D._pose_between(m, o), D._pose_between(o, m)
            tol_b, tol_a = float(TOL * abs(o.schedule[1])), float(TOL * abs(m.schedule[1]))
            link = torch.empty((ha, wa), dtype=torch.int32, device=eng.device)
            w_out, score_out = torch.empty_like(m.w), torch.empty_like(m.score)
            views = torch.empty((ha, wa), dtype=torch.uint8, device=eng.device)
            claimed = torch.empty((hb, wb), dtype=torch.uint8, device=eng.device)
            rest = torch.empty((hb, wb), dtype=torch.uint8, device=eng.device)
            run_link = lambda: eng.ctx.call("im_dense_fuse_link", ptr(keep[0]), ptr(m.w), ptr(m.score), ha, wa, ptr(keep[1]), ptr(o.w), ptr(o.score), hb, wb,  # noqa: E731
                                            ab.ctypes.data, tol_b, ptr(link), ptr(w_out), ptr(score_out), ptr(views), ptr(claimed), eng.stream_ptr())
            run_rest = lambda: eng.ctx.call("im_dense_fuse_rest", ptr(keep[1]), ptr(o.w), hb, wb, ptr(keep[0]), ptr(m.w), ha, wa, ba.ctypes.data, tol_a,  # noqa: E731
                                            ptr(claimed), ptr(rest), eng.stream_ptr())
            q["link_ms"], q["link_ms_all"] = timed(torch, run_link, a.repeats)
            q["rest_ms"], q["rest_ms_all"] = timed(torch, run_rest, a.repeats)
            q["link_launches_ms"] = launches(eng, torch, run_link, a.repeats)
            q["rest_launches_ms"] = launches(eng, torch, run_rest, a.repeats)
            q["fuse_whole_ms"], _ = timed(torch, lambda: D.fuse(m, keep[0], o, keep[1], TOL, engine=eng), a.repeats)
            q["consistency_both_views_ms"], _ = timed(torch, lambda: [D.consistency(maps[v], maps[1 - v], FILTER, engine=eng) for v in (0, 1)], a.repeats)
            q["fuse_over_sweep"] = (q["link_ms"] + q["rest_ms"]) / q["sweep_ms"]
            kept = [int((k != 0).sum().item()) for k in keep]
            q["kept_pixels"] = kept
            q["linked_pixels"], q["claimed_pixels"], q["rest_pixels"] = int((link >= 0).sum().item()), int(claimed.sum().item()), int(rest.sum().item())
            q["unclaimed_pixels_of_view_1_that_link_themselves"] = kept[1] - q["claimed_pixels"] - q["rest_pixels"]
            q["points_concatenated"], q["points_fused"], q["points_fused_min_views_2"] = kept[0] + kept[1], kept[0] + q["rest_pixels"], q["linked_pixels"]
            if f == 4:
                host = [x.cpu().numpy() for x in (keep[0], m.w, m.score, keep[1], o.w, o.score)]
                t0 = time.perf_counter()
                want = FO.fuse(*host, ab, tol_b)
                want = want + (FO.rest(host[3], host[4], host[0], host[1], ba, tol_a, want[4]),)
                q["numpy_restatement_whole_map_s"] = round(time.perf_counter() - t0, 3)
                equal = all(np.array_equal(g.cpu().numpy().view(np.uint8), x.view(np.uint8)) for g, x in zip((link, w_out, score_out, views, claimed, rest), want))
                q["equal_to_the_restatement"] = bool(equal)
                equal_all = equal_all and equal
            for k in list(q):
                if isinstance(q[k], float):
                    q[k] = round(q[k], 4)
            r[kind] = q
            del maps, m, o, keep, link, w_out, score_out, views, claimed, rest
        res["downscale"][str(f)] = r
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
