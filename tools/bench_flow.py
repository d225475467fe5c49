"""Times the dense surface displacement between two epochs (csrc/dense_flow.hip) on the device (device events, one warm-up, median of the
repeats) on the 24 MP synthetic pair of tools/bench_dense.py at downscale 4 and at downscale 2. Epoch B is epoch A with both views moved by
(12, 8) pixels at full size, a whole-pixel shift at either downscale; both epochs' maps come from `dense.build_depth_maps`, view 0:
  - `im_flow_match` with the defaults (radius 7, search 8: 289 candidates of 225 products) and with the largest setting (radius 15, search
    16: 1089 candidates of 961 products), `im_flow_check` and `im_flow_lift`, each on outputs allocated once, the whole
    `dense_flow.surface_displacement` (both matches, the check, the lift, its allocations and its compaction included), and beside them
    the sweep that made the map, timed in the same run; the share of pixels valid, kept and lifted and the share whose match is the shift;
  - the numpy restatement (tests/flow_oracle.py) of the default match on a 128 x 128 crop, which the device's output on that crop is
    compared with first (bits).
What bounds `im_flow_match` - the byte reads of LDS in the row sums, the two barriers per candidate, or the integer multiplies - is NOT
measured here (that takes a counter run of its own). No time is asserted and no target is set.

    python tools/bench_flow.py [--repeats 5] [--out profiles/r26_flow_bench.json]"""
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

SHIFT = (12, 8)                     # pixels at full size
SETTINGS = {"radius_7_search_8": (7, 8), "radius_15_search_16": (15, 16)}
RADIUS, MIN_VAR, MIN_SCORE, TOL, MAX_DIFF, CROP = 3, 4, 0.8, 1.0, 2.0, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_flow_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_flow.py needs a HIP device: there is nothing to time without one")
    import flow_oracle as FO
    from icepy4d_amd import dense as D
    from icepy4d_amd import dense_flow as DF
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine, to_device
    eng = Engine(0)
    im0, im1, _ = synthetic_pair()
    K0 = np.array([[F, 0.0, W / 2.0], [0.0, F, H / 2.0], [0.0, 0.0, 1.0]])
    K1 = K0.copy()
    K1[0, 2] += MARGIN
    cams = [Cam(K0, np.eye(3), np.zeros(3), W, H), Cam(K1, np.eye(3), np.array([-1.0, 0.0, 0.0]), W + MARGIN, H)]
    rng = (F / (D_FAR + 8.0), F / (D_NEAR - 8.0))
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "image": [H, W], "sweep_radius": RADIUS, "min_score": MIN_SCORE, "min_var": MIN_VAR,
           "tol": TOL, "max_diff": MAX_DIFF, "settings": {k: dict(radius=r, search=s, candidates=(2 * s + 1) ** 2, products_per_pixel=(2 * s + 1) ** 2 * (2 * r + 1) ** 2)
                                                          for k, (r, s) in SETTINGS.items()},
           "scene": f"tools/bench_dense.py's pair at two epochs, the second with both views moved by {SHIFT} px at full size (torch.roll: the rim wraps "
                    f"around); depth range {rng[0]:.2f}..{rng[1]:.2f}",
           "clock": "device events around the calls, one warm-up, median of the repeats; view 0; match, check and lift on outputs allocated once",
           "unmeasured": "what bounds im_flow_match (the byte reads of LDS in the row sums, the two barriers per candidate, or the integer multiplies): "
                         "no counter run was made",
           "downscale": {}}
    d_a = [to_device(im0, eng.device), to_device(im1, eng.device)]
    d_b = [torch.roll(t, (SHIFT[1], SHIFT[0]), (0, 1)).contiguous() for t in d_a]
    equal_all = True
    for f in (4, 2):
        sx, sy = SHIFT[0] // f, SHIFT[1] // f
        maps_a = D.build_depth_maps(d_a, cams, depth_range=rng, downscale=f, engine=eng)
        maps_b = D.build_depth_maps(d_b, cams, depth_range=rng, downscale=f, engine=eng)
        keep_a = D.consistency(maps_a[0], maps_a[1], "ModerateFiltering", engine=eng)
        keep_b = D.consistency(maps_b[0], maps_b[1], "ModerateFiltering", engine=eng)
        m, o, mb = maps_a[0], maps_a[1], maps_b[0]
        small = [D._SmallCam(x.K, x.R, x.t) for x in maps_a]
        A, B = D.sweep_matrices(m.K, o.K, *D.relative_pose(small[0], small[1]))
        h, w = m.plane.shape
        q = {"map_shape": [h, w], "planes": m.schedule[2], "shift": [sx, sy], "share_kept_a": round(float(keep_a.float().mean().item()), 4),
             "share_kept_b": round(float(keep_b.float().mean().item()), 4)}
        q["sweep_ms"], q["sweep_ms_all"] = timed(torch, lambda: D.sweep(m.grey, o.grey, A, B, *m.schedule, RADIUS, MIN_VAR, MIN_SCORE, engine=eng), a.repeats)
        dev = eng.device
        outs = lambda: (torch.empty((h, w), dtype=torch.float64, device=dev), torch.empty((h, w), dtype=torch.float64, device=dev),  # noqa: E731
                        torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w), dtype=torch.uint8, device=dev))
        fwd, bwd = outs(), outs()

        def match(src, dst, ask, r, s, out, sign=1):
            eng.ctx.call("im_flow_match", ptr(src), ptr(dst), h, w, r, s, sign * sx, sign * sy, MIN_VAR, MIN_SCORE, ptr(ask), *(ptr(t) for t in out), eng.stream_ptr())

        for name, (r, s) in SETTINGS.items():
            # the prior is the shift where the range does not hold it: the prior moves the staged region and costs nothing else
            k = {}
            k["match_forward_kept_pixels_ms"], k["match_forward_kept_pixels_ms_all"] = timed(torch, lambda: match(m.grey, mb.grey, keep_a, r, s, fwd), a.repeats)
            k["match_backward_every_pixel_ms"], k["match_backward_every_pixel_ms_all"] = timed(torch, lambda: match(mb.grey, m.grey, None, r, s, bwd, -1), a.repeats)
            valid = fwd[3] != 0
            k["share_valid_of_kept"] = round(float(valid.float().sum().item() / max(1.0, keep_a.float().sum().item())), 4)
            k["share_of_valid_at_the_shift"] = round(float(((torch.round(fwd[0]) == sx) & (torch.round(fwd[1]) == sy) & valid).float().sum().item()
                                                           / max(1.0, valid.float().sum().item())), 4)
            q[name] = k
        r, s = SETTINGS["radius_7_search_8"]
        match(m.grey, mb.grey, keep_a, r, s, fwd)
        match(mb.grey, m.grey, None, r, s, bwd, -1)
        keep = torch.empty((h, w), dtype=torch.uint8, device=dev)
        run_check = lambda: eng.ctx.call("im_flow_check", ptr(fwd[0]), ptr(fwd[1]), ptr(fwd[3]), ptr(bwd[0]), ptr(bwd[1]), ptr(bwd[3]), h, w, TOL, ptr(keep),  # noqa: E731
                                         eng.stream_ptr())
        q["check_ms"], q["check_ms_all"] = timed(torch, run_check, a.repeats)
        P, Dv = torch.empty((h, w, 3), dtype=torch.float64, device=dev), torch.empty((h, w, 3), dtype=torch.float64, device=dev)
        ok = torch.empty((h, w), dtype=torch.uint8, device=dev)
        cam_a, cam_b = DF._cam(m), DF._cam(mb)
        run_lift = lambda: eng.ctx.call("im_flow_lift", ptr(fwd[0]), ptr(fwd[1]), ptr(fwd[3]), ptr(keep), ptr(m.plane), ptr(m.w), h, w, cam_a.ctypes.data,  # noqa: E731
                                        ptr(mb.plane), ptr(mb.w), ptr(keep_b), h, w, cam_b.ctypes.data, float(mb.schedule[1]), MAX_DIFF, ptr(P), ptr(Dv), ptr(ok),
                                        eng.stream_ptr())
        q["lift_ms"], q["lift_ms_all"] = timed(torch, run_lift, a.repeats)
        q["share_checked_of_valid"] = round(float(keep.float().sum().item() / max(1.0, (fwd[3] != 0).float().sum().item())), 4)
        q["share_lifted_of_kept"] = round(float(ok.float().sum().item() / max(1.0, keep_a.float().sum().item())), 4)
        whole = lambda: DF.surface_displacement(m, keep_a, mb, keep_b, 1.0, engine=eng, radius=r, search=s, prior=(sx, sy), min_var=MIN_VAR,  # noqa: E731
                                                min_score=MIN_SCORE, tol=TOL, max_diff=MAX_DIFF)
        q["surface_displacement_whole_ms"], q["surface_displacement_whole_ms_all"] = timed(torch, whole, a.repeats)
        got = whole()
        sel = ok != 0
        q["whole_equals_the_pieces"] = bool(torch.equal(got.points, P[sel]) and torch.equal(got.displacement, Dv[sel]))
        # the truth: the surface moved by (sx, sy) pixels at its own depth; the error of D in units of the pixel's footprint
        depth = 1.0 / m.w[sel]
        truth = torch.stack([sx * depth / m.K[0, 0], sy * depth / m.K[1, 1], torch.zeros_like(depth)], 1)
        err = (torch.linalg.norm(got.displacement - truth, dim=1) * m.K[0, 0] / depth).cpu().numpy()
        q["error_of_D_in_pixel_footprints_median_p99"] = [round(float(np.median(err)), 4), round(float(np.percentile(err, 99)), 4)] if err.size else None
        q["surface_displacement_over_sweep"] = round(q["surface_displacement_whole_ms"] / q["sweep_ms"], 3)
        # the restatement of the default match on a crop, for scale and as a check at this size
        y0, x0 = (h - CROP) // 2, (w - CROP) // 2
        ca, cb = (np.ascontiguousarray(t[y0:y0 + CROP, x0:x0 + CROP].cpu().numpy()) for t in (m.grey, mb.grey))
        t0 = time.perf_counter()
        want = FO.match(ca, cb, None, r, s, (sx, sy), MIN_VAR, MIN_SCORE)
        q[f"numpy_restatement_match_{CROP}x{CROP}_crop_s"] = round(time.perf_counter() - t0, 3)
        d_ca, d_cb = to_device(ca, dev), to_device(cb, dev)
        c_out = (torch.empty((CROP, CROP), dtype=torch.float64, device=dev), torch.empty((CROP, CROP), dtype=torch.float64, device=dev),
                 torch.empty((CROP, CROP), dtype=torch.float32, device=dev), torch.empty((CROP, CROP), dtype=torch.uint8, device=dev))
        eng.ctx.call("im_flow_match", ptr(d_ca), ptr(d_cb), CROP, CROP, r, s, sx, sy, MIN_VAR, MIN_SCORE, None, *(ptr(t) for t in c_out), eng.stream_ptr())
        equal = all(np.array_equal(g.cpu().numpy().view(np.uint8), np.ascontiguousarray(x).view(np.uint8)) for g, x in zip(c_out, want))
        q["crop_equal_to_the_restatement"] = bool(equal)
        equal_all = equal_all and equal
        for k in list(q):
            if isinstance(q[k], float):
                q[k] = round(q[k], 4)
            elif isinstance(q[k], dict):
                q[k] = {n: (round(v, 4) if isinstance(v, float) else v) for n, v in q[k].items()}
        res["downscale"][str(f)] = q
        del maps_a, maps_b, m, o, mb, fwd, bwd, keep, P, Dv, ok, got
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
