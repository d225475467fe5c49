"""Times the slanted-window refinement of a depth map (csrc/dense_refine.hip) on the device (device events, one warm-up, median of the
repeats) on the 24 MP synthetic pair of tools/bench_dense.py at downscale 4 and at downscale 2, on view 0's winner-take-all map and on
its semi-global map, with the defaults (two passes, fit_radius 4, max_diff 2, min_count 6, span 1, sub 4, radius 3):
  - per pass `im_dense_slant` and `im_dense_refine` on outputs allocated once, the whole `dense.refine_slanted` (its allocations included),
    and beside them the sweep that made the map, timed in the same run; the share of pixels taken per pass and the median and 99th
    percentile of the error of the kept inverse depths in plane steps before and after each pass;
  - the numpy restatement (tests/refine_oracle.py) of one pass on a 128 x 128 crop of the map, which the device's output on that crop is
    compared with first (bits).
A slanted window shares no sample with its neighbour's: a pass takes (2 span sub + 1) (2 radius + 1)^2 = 441 samples per pixel where the
sweep takes about one per pixel and plane. What bounds `im_dense_refine` - the float64 of the 441 homographies and coordinates per pixel,
their two divisions each, or the gather of the four taps - is NOT measured here (that takes a counter run of its own). No time is
asserted and no target is set.

    python tools/bench_refine.py [--repeats 5] [--out profiles/r25_refine_bench.json]"""
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

PASSES, FIT_RADIUS, MAX_DIFF, MIN_COUNT, SPAN, SUB, RADIUS, MIN_VAR = 2, 4, 2.0, 6, 1, 4, 3, 4
CROP = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_refine_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_refine.py needs a HIP device: there is nothing to time without one")
    import refine_oracle as RO
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
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "image": [H, W], "radius": RADIUS, "min_score": 0.8, "min_var": MIN_VAR,
           "refine": dict(passes=PASSES, fit_radius=FIT_RADIUS, max_diff=MAX_DIFF, min_count=MIN_COUNT, span=SPAN, sub=SUB),
           "samples_per_pixel_and_pass": (2 * SPAN * SUB + 1) * (2 * RADIUS + 1) ** 2,
           "scene": f"tools/bench_dense.py's pair: seeded texture, a front slanted along v with {D_NEAR}..{D_FAR} px of disparity at full size; "
                    f"depth range {rng[0]:.2f}..{rng[1]:.2f}",
           "clock": "device events around the calls, one warm-up, median of the repeats; view 0; slant and refine on outputs allocated once",
           "unmeasured": "what bounds im_dense_refine (the float64 homographies and coordinates of 441 samples per pixel, their divisions, or the "
                         "gather of the four taps): no counter run was made",
           "downscale": {}}
    d_im = [to_device(im0, eng.device), to_device(im1, eng.device)]
    equal_all = True
    for f in (4, 2):
        r = {}
        rows_of = lambda h0: np.arange(h0) * f + (f - 1) / 2.0  # noqa: E731
        for kind, extra in (("winner_take_all", {}), ("semi_global", dict(regularisation="sgm"))):
            maps = D.build_depth_maps(d_im, cams, depth_range=rng, downscale=f, engine=eng, **extra)
            m, o = maps[0], maps[1]
            small = [D._SmallCam(x.K, x.R, x.t) for x in maps]
            A, B = D.sweep_matrices(m.K, o.K, *D.relative_pose(small[0], small[1]))
            h0, w0 = m.plane.shape
            h1, w1 = o.grey.shape
            w_step = float(m.schedule[1])
            kept = (m.plane >= 0).cpu().numpy()
            truth = ((D_NEAR + (D_FAR - D_NEAR) * rows_of(h0) / (H - 1.0)) / F)[:, None]

            def error(w):
                e = (np.abs(w.cpu().numpy() - truth) / abs(w_step))[kept]
                return [round(float(np.median(e)), 4), round(float(np.percentile(e, 99)), 4)]

            q = {"map_shape": [h0, w0], "planes": m.schedule[2], "share_kept": round(float(kept.mean()), 4)}
            q["sweep_ms"], q["sweep_ms_all"] = timed(torch, lambda: D.sweep(m.grey, o.grey, A, B, *m.schedule, RADIUS, MIN_VAR, 0.8, engine=eng, **extra), a.repeats)
            q["error_in_plane_steps_median_p99"] = {"before": error(m.w)}
            q["mean_score"] = {"before": round(float(m.score.cpu().numpy()[kept].astype(np.float64).mean()), 4)}
            slant = torch.empty((h0, w0, 2), dtype=torch.float64, device=eng.device)
            fitted = torch.empty((h0, w0), dtype=torch.uint8, device=eng.device)
            taken = torch.empty((h0, w0), dtype=torch.uint8, device=eng.device)
            cur = m
            for n in range(1, PASSES + 1):
                w_out, score_out = torch.empty_like(cur.w), torch.empty_like(cur.score)
                run_slant = lambda: eng.ctx.call("im_dense_slant", ptr(cur.plane), ptr(cur.w), h0, w0, w_step, FIT_RADIUS, MAX_DIFF, MIN_COUNT, ptr(slant),  # noqa: E731
                                                 ptr(fitted), eng.stream_ptr())
                run_refine = lambda: eng.ctx.call("im_dense_refine", ptr(m.grey), h0, w0, ptr(o.grey), h1, w1, A.ctypes.data, B.ctypes.data, ptr(cur.plane),  # noqa: E731
                                                  ptr(cur.w), ptr(cur.score), ptr(slant), w_step, RADIUS, MIN_VAR, SPAN, SUB, ptr(w_out), ptr(score_out),
                                                  ptr(taken), eng.stream_ptr())
                q[f"pass{n}_slant_ms"], q[f"pass{n}_slant_ms_all"] = timed(torch, run_slant, a.repeats)
                q[f"pass{n}_refine_ms"], q[f"pass{n}_refine_ms_all"] = timed(torch, run_refine, a.repeats)
                q[f"pass{n}_share_fitted"] = round(float(fitted.float().mean().item()), 4)
                q[f"pass{n}_share_taken"] = round(float(taken.float().mean().item()), 4)
                cur = cur._replace(w=w_out, score=score_out)
                q["error_in_plane_steps_median_p99"][f"after_pass{n}"] = error(cur.w)
                q["mean_score"][f"after_pass{n}"] = round(float(cur.score.cpu().numpy()[kept].astype(np.float64).mean()), 4)
            whole = lambda: D.refine_slanted(m, o, PASSES, FIT_RADIUS, MAX_DIFF, MIN_COUNT, SPAN, SUB, RADIUS, MIN_VAR, engine=eng)  # noqa: E731
            q["refine_slanted_whole_ms"], q["refine_slanted_whole_ms_all"] = timed(torch, whole, a.repeats)
            got = whole()
            q["whole_equals_the_passes"] = bool(torch.equal(got.w, cur.w) and torch.equal(got.score, cur.score))
            q["refine_slanted_over_sweep"] = round(q["refine_slanted_whole_ms"] / q["sweep_ms"], 3)
            # the restatement of one pass on a crop of the map, for scale and as a check at this size
            y0, x0 = (h0 - CROP) // 2, (w0 - CROP) // 2
            T = np.array([[1.0, 0.0, x0], [0.0, 1.0, y0], [0.0, 0.0, 1.0]])                 # crop pixel -> map pixel
            Ac, Bc = np.ascontiguousarray((A.reshape(3, 3) @ T).reshape(9)), np.ascontiguousarray((B.reshape(3, 3) @ T).reshape(9))
            crop = [np.ascontiguousarray(t[y0:y0 + CROP, x0:x0 + CROP].cpu().numpy()) for t in (m.grey, m.plane, m.w, m.score)]
            g1 = o.grey.cpu().numpy()
            t0 = time.perf_counter()
            sl, fit = RO.slant(crop[1], crop[2], w_step, FIT_RADIUS, MAX_DIFF, MIN_COUNT)
            want = RO.refine(crop[0], g1, Ac, Bc, crop[1], crop[2], crop[3], sl, w_step, RADIUS, MIN_VAR, SPAN, SUB)
            q[f"numpy_restatement_one_pass_{CROP}x{CROP}_crop_s"] = round(time.perf_counter() - t0, 3)
            d_crop = [to_device(c, eng.device) for c in crop]
            outs = [torch.empty((CROP, CROP, 2), dtype=torch.float64, device=eng.device), torch.empty((CROP, CROP), dtype=torch.uint8, device=eng.device),
                    torch.empty((CROP, CROP), dtype=torch.float64, device=eng.device), torch.empty((CROP, CROP), dtype=torch.float32, device=eng.device),
                    torch.empty((CROP, CROP), dtype=torch.uint8, device=eng.device)]
            eng.ctx.call("im_dense_slant", ptr(d_crop[1]), ptr(d_crop[2]), CROP, CROP, w_step, FIT_RADIUS, MAX_DIFF, MIN_COUNT, ptr(outs[0]), ptr(outs[1]),
                         eng.stream_ptr())
            eng.ctx.call("im_dense_refine", ptr(d_crop[0]), CROP, CROP, ptr(o.grey), h1, w1, Ac.ctypes.data, Bc.ctypes.data, ptr(d_crop[1]), ptr(d_crop[2]),
                         ptr(d_crop[3]), ptr(outs[0]), w_step, RADIUS, MIN_VAR, SPAN, SUB, ptr(outs[2]), ptr(outs[3]), ptr(outs[4]), eng.stream_ptr())
            equal = all(np.array_equal(g.cpu().numpy().view(np.uint8), np.ascontiguousarray(x).view(np.uint8)) for g, x in zip(outs, (sl, fit) + tuple(want)))
            q["crop_equal_to_the_restatement"] = bool(equal)
            equal_all = equal_all and equal
            for k in list(q):
                if isinstance(q[k], float):
                    q[k] = round(q[k], 4)
            r[kind] = q
            del maps, m, o, cur, got, slant, fitted, taken, outs, d_crop
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
