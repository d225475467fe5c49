"""Times the depth-map clean-up (csrc/depth_clean.hip) on the device (device events, one warm-up, median of the repeats) on the 24 MP
synthetic pair of tools/bench_dense.py at downscale 4 and at downscale 2, on view 0's winner-take-all map and on its semi-global map:
  - `im_depth_components` of the surfaces (mode 0, max_diff 1) and of the holes (mode 1), `im_depth_drop_small` (min_size 16),
    `im_depth_fill_holes` (max_hole 64, max_diff 2) on the map without its speckles, and beside them the sweep that made the map, timed
    in the same run; the numbers of components, of dropped and of filled pixels;
  - the numpy restatement (tests/depth_oracle.py) on a 256 x 256 crop of the map, which the device's output on that crop is compared with
    first (bits);
  - per launch of the components and of the fill, the library's own events (`im_profile_begin` / `im_profile_end`).
The scene is clean: what the clean-up gains on noise is pinned in tests/test_depth_clean_cpu.py, not here. What bounds the merge launch of
`im_depth_components` - the chains its threads walk, the atomics on the parents or the strided reads along a column seam - is NOT measured
here (that takes a counter run of its own). No time is asserted and no target is set.

    python tools/bench_depth_clean.py [--repeats 5] [--out profiles/r23_depth_clean_bench.json]"""
import argparse
import ctypes
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

SPECKLE, HOLES = (16, 1), (64, 2)


def launches(eng, torch, fn, repeats):
    """{launch: mean ms} over `repeats` calls of fn, from the library's own events around every launch (im_profile_begin / im_profile_end),
    the reading of an empty event pair subtracted."""
    fn()
    torch.cuda.synchronize()
    eng.ctx.call("im_profile_begin")
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    eng.ctx.call("im_profile_end", buf, len(buf))
    prof = json.loads(buf.value.decode())
    cal = prof.pop("_empty_event_pair", None)
    ov = cal["total_ms"] / cal["count"] if cal and cal["count"] else 0.0
    return {k: round((v["total_ms"] - v["count"] * ov) / repeats, 4) for k, v in prof.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_depth_clean_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_depth_clean.py needs a HIP device: there is nothing to time without one")
    import depth_oracle as DO
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
           "speckle": list(SPECKLE), "holes": list(HOLES),
           "scene": f"tools/bench_dense.py's pair: seeded texture, a front slanted along v with {D_NEAR}..{D_FAR} px of disparity at full size; "
                    f"depth range {rng[0]:.2f}..{rng[1]:.2f}",
           "clock": "device events around the calls (allocation of the outputs included), one warm-up, median of the repeats; view 0",
           "unmeasured": "what bounds the merge launch of im_depth_components (the chains walked, the atomics on the parents or the strided reads of a "
                         "column seam): no counter run was made",
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
            h0, w0 = m.plane.shape
            q = {"map_shape": [h0, w0], "planes": m.schedule[2], "share_kept": round(float((m.plane >= 0).float().mean().item()), 4)}
            q["sweep_ms"], q["sweep_ms_all"] = timed(torch, lambda: D.sweep(m.grey, o.grey, A, B, *m.schedule, 3, 4, 0.8, engine=eng, **extra), a.repeats)
            q["components_surfaces_ms"], q["components_surfaces_ms_all"] = timed(torch, lambda: D.depth_components(m.plane, SPECKLE[1], engine=eng), a.repeats)
            q["components_surfaces_launches_ms"] = launches(eng, torch, lambda: D.depth_components(m.plane, SPECKLE[1], engine=eng), a.repeats)
            label, size = D.depth_components(m.plane, SPECKLE[1], engine=eng)
            q["surface_components"] = int((label == torch.arange(h0 * w0, device=label.device, dtype=torch.int32).reshape(h0, w0)).sum().item())
            q["largest_surface_component"] = int(size.max().item())
            scratch = [m.plane.clone(), m.w.clone(), m.score.clone()]
            count = torch.empty(1, dtype=torch.int64, device=eng.device)

            def drop():
                for dst, src in zip(scratch, (m.plane, m.w, m.score)):
                    dst.copy_(src)
                eng.ctx.call("im_depth_drop_small", ptr(size), h0, w0, SPECKLE[0], ptr(scratch[0]), ptr(scratch[1]), ptr(scratch[2]), ptr(count), eng.stream_ptr())

            def copies():
                for dst, src in zip(scratch, (m.plane, m.w, m.score)):
                    dst.copy_(src)

            with_copies, _ = timed(torch, drop, a.repeats)
            only_copies, _ = timed(torch, copies, a.repeats)
            q["drop_small_ms"], q["drop_small_with_the_copies_of_the_maps_ms"] = round(with_copies - only_copies, 4), round(with_copies, 4)
            clean, dropped = D.remove_speckles(m, *SPECKLE, engine=eng, return_counts=True)
            q["dropped_pixels"] = int(dropped.item())
            q["components_holes_ms"], q["components_holes_ms_all"] = timed(torch, lambda: D.depth_components(clean.plane, 0, holes=True, engine=eng), a.repeats)
            q["components_holes_launches_ms"] = launches(eng, torch, lambda: D.depth_components(clean.plane, 0, holes=True, engine=eng), a.repeats)
            hl, hs = D.depth_components(clean.plane, 0, holes=True, engine=eng)
            q["holes"] = int((hl == torch.arange(h0 * w0, device=hl.device, dtype=torch.int32).reshape(h0, w0)).sum().item())
            outs = [torch.empty_like(clean.plane), torch.empty_like(clean.w), torch.empty_like(clean.score), torch.empty((h0, w0), dtype=torch.uint8, device=eng.device)]
            fill = lambda: eng.ctx.call("im_depth_fill_holes", ptr(clean.plane), ptr(clean.w), ptr(clean.score), ptr(hl), ptr(hs), h0, w0, HOLES[0], HOLES[1],  # noqa: E731
                                        float(m.schedule[0]), float(m.schedule[1]), int(m.schedule[2]), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]),
                                        ptr(count), eng.stream_ptr())
            q["fill_holes_ms"], q["fill_holes_ms_all"] = timed(torch, fill, a.repeats)
            q["fill_holes_launches_ms"] = launches(eng, torch, fill, a.repeats)
            q["filled_pixels"] = int(count.item())
            q["remove_speckles_whole_ms"], _ = timed(torch, lambda: D.remove_speckles(m, *SPECKLE, engine=eng), a.repeats)
            q["fill_holes_whole_ms"], _ = timed(torch, lambda: D.fill_holes(clean, *HOLES, engine=eng), a.repeats)
            q["clean_up_total_ms"] = round(q["components_surfaces_ms"] + q["drop_small_ms"] + q["components_holes_ms"] + q["fill_holes_ms"], 3)
            # the restatement on a crop of the map, for scale and as a check at this size
            c = 256
            y0, x0 = (h0 - c) // 2, (w0 - c) // 2
            crop = [np.ascontiguousarray(t[y0:y0 + c, x0:x0 + c].cpu().numpy()) for t in (m.plane, m.w, m.score)]
            t0 = time.perf_counter()
            want = DO.clean(*crop, m.schedule, SPECKLE, HOLES)
            q["numpy_restatement_256x256_crop_s"] = round(time.perf_counter() - t0, 3)
            mc = m._replace(plane=to_device(crop[0], eng.device), w=to_device(crop[1], eng.device), score=to_device(crop[2], eng.device))
            got = D.fill_holes(D.remove_speckles(mc, *SPECKLE, engine=eng), *HOLES, engine=eng)
            equal = all(np.array_equal(g.cpu().numpy().view(np.uint8), x.view(np.uint8)) for g, x in zip((got.plane, got.w, got.score), want))
            q["crop_equal_to_the_restatement"] = bool(equal)
            equal_all = equal_all and equal
            for k in list(q):
                if isinstance(q[k], float):
                    q[k] = round(q[k], 4)
            r[kind] = q
            del maps, m, o, label, size, hl, hs, clean, outs, scratch
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
