"""Times the coarse-to-fine dense displacement (csrc/dense_flow_field.hip, `dense_flow.match_flow_pyramid`) on the device (device events,
one warm-up, median of the repeats) on view 0 of the 24 MP synthetic pair of tools/bench_dense.py at downscale 4 and at downscale 2.
That image is `dense_cases.texture` in tiles, which has structure at a few pixels only and is flat two levels up, so half of every grey
value here is an octave texture with blocks of 8 to 128 pixels at full size. Epoch B is epoch A moved by (72, 40) pixels at full size,
(18, 10) at downscale 4 and (36, 20) at downscale 2 - beyond the single level's reach at search 8 and at search 16 alike - with noise of
sigma 2 on its grey values. NO prior is given, every pixel is asked:
  - `match_flow_pyramid` with its defaults (3 levels, radius 7, search 8, fine_search 2; reach 38 px) as a whole, its allocations and
    the four `im_pyr_down` calls included, and level by level on outputs allocated once: the reductions, the coarsest level's
    `im_flow_match`, and `im_flow_prior_up` and `im_flow_match_field` of each finer level; per finer level the share of tiles on the direct
    path out of `d_tile_path`; the share of pixels valid and the share at the true shift;
  - in the same run `im_flow_match` at radius 7, search 8 and at radius 15, search 16 on the same images, which time what the single
    level costs and find nothing at this shift;
  - the numpy restatement (tests/pyrflow_oracle.py) of the whole pyramid on a 192 x 192 crop, which the device's output on that crop is
    compared with first (bits).
No time is asserted and no target is set.

    python tools/bench_flow_pyramid.py [--repeats 5] [--out profiles/r27_flow_pyramid_bench.json]"""
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
from bench_dense import H, W, synthetic_pair  # noqa: E402
from bench_pointcloud import timed  # noqa: E402

SHIFT = (72, 40)                    # pixels at full size
LEVELS, RADIUS, SEARCH, FINE, MEDIAN_RADIUS, MIN_COUNT, MIN_VAR, MIN_SCORE, NOISE, CROP = 3, 7, 8, 2, 1, 1, 4, 0.8, 2.0, 192
SINGLE = {"radius_7_search_8": (7, 8), "radius_15_search_16": (15, 16)}


def coarse_octaves(seed, h, w):
    """Seeded noise in blocks of 8, 16, 32, 64 and 128 pixels, summed: [h, w] in 0..1."""
    rng = np.random.default_rng(seed)
    t = np.zeros((h, w), np.float32)
    for s in (8, 16, 32, 64, 128):
        n = rng.random(((h + s - 1) // s, (w + s - 1) // s), dtype=np.float32)
        t += np.kron(n, np.ones((s, s), np.float32))[:h, :w]
    return (t - t.min()) / (t.max() - t.min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_flow_pyramid_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_flow_pyramid.py needs a HIP device: there is nothing to time without one")
    import pyrflow_oracle as PO
    from icepy4d_amd import dense as D
    from icepy4d_amd import dense_flow as DF
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine, to_device
    eng = Engine(0)
    dev = eng.device
    im0 = synthetic_pair()[0]
    im0 = np.rint(0.5 * im0.astype(np.float32) + 127.5 * coarse_octaves(27, H, W)).astype(np.uint8)
    reach = PO.reach(LEVELS, SEARCH, FINE)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "image": [H, W], "shift_at_full_size": list(SHIFT), "noise_sigma_on_b": NOISE,
           "pyramid": dict(levels=LEVELS, radius=RADIUS, search=SEARCH, fine_search=FINE, median_radius=MEDIAN_RADIUS, min_count=MIN_COUNT, min_var=MIN_VAR,
                           min_score=MIN_SCORE, reach_px=reach, candidates_coarsest=(2 * SEARCH + 1) ** 2, candidates_finer=(2 * FINE + 1) ** 2,
                           tiled_spread_px=PO.spread(RADIUS, FINE), lds_bytes_of_a_field_launch=PO.lds_bytes(RADIUS, FINE, PO.spread(RADIUS, FINE), PO.spread(RADIUS, FINE))),
           "single_level": {k: dict(radius=r, search=s, candidates=(2 * s + 1) ** 2) for k, (r, s) in SINGLE.items()},
           "scene": "view 0 of tools/bench_dense.py's pair, half of it replaced by noise in blocks of 8 to 128 px; epoch B is epoch A moved (torch.roll: the rim "
                    "wraps around) with Gaussian noise on the downscaled grey values; no prior, every pixel asked",
           "clock": "device events around the calls, one warm-up, median of the repeats; the levels on outputs allocated once",
           "unmeasured": "what bounds im_flow_match_field on either path: no counter run was made",
           "downscale": {}}
    d_a = to_device(im0, dev)
    d_b = torch.roll(d_a, (SHIFT[1], SHIFT[0]), (0, 1)).contiguous()
    gen = torch.Generator(device="cpu").manual_seed(27)
    equal_all = True
    for f in (4, 2):
        sx, sy = SHIFT[0] // f, SHIFT[1] // f
        ga = D.downscale_image(d_a, f).contiguous()
        gb = D.downscale_image(d_b, f)
        noise = torch.randn(gb.shape, generator=gen).to(dev) * NOISE
        gb = torch.clamp(torch.round(gb.to(torch.float32) + noise), 0, 255).to(torch.uint8).contiguous()
        h, w = ga.shape
        shapes = DF.level_shapes((h, w), LEVELS)
        q = {"shape": [h, w], "shift": [sx, sy], "levels": [list(s) for s in shapes]}
        assert max(sx, sy) > max(s for _, s in SINGLE.values()) and max(sx, sy) <= reach

        def outs(shape):
            return (torch.empty(shape, dtype=torch.float64, device=dev), torch.empty(shape, dtype=torch.float64, device=dev),
                    torch.empty(shape, dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.uint8, device=dev))

        # the whole call
        whole = lambda: DF.match_flow_pyramid(ga, gb, levels=LEVELS, radius=RADIUS, search=SEARCH, fine_search=FINE, min_var=MIN_VAR, min_score=MIN_SCORE,  # noqa: E731
                                              median_radius=MEDIAN_RADIUS, min_count=MIN_COUNT, engine=eng)
        q["match_flow_pyramid_whole_ms"], q["match_flow_pyramid_whole_ms_all"] = timed(torch, whole, a.repeats)
        # level by level, on outputs allocated once
        pyr = [(ga, gb)] + [(torch.empty(s, dtype=torch.uint8, device=dev), torch.empty(s, dtype=torch.uint8, device=dev)) for s in shapes[1:]]

        def reduce_all():
            for lv in range(LEVELS - 1):
                for k in (0, 1):
                    eng.ctx.call("im_pyr_down", ptr(pyr[lv][k]), ptr(pyr[lv + 1][k]), 1, *shapes[lv], 1, eng.stream_ptr())

        q["pyr_down_all_levels_both_images_ms"], _ = timed(torch, reduce_all, a.repeats)
        fields = [outs(s) for s in shapes]
        top = LEVELS - 1
        run_top = lambda: eng.ctx.call("im_flow_match", ptr(pyr[top][0]), ptr(pyr[top][1]), *shapes[top], RADIUS, SEARCH, 0, 0, MIN_VAR, MIN_SCORE, None,  # noqa: E731
                                       *(ptr(t) for t in fields[top]), eng.stream_ptr())
        per_level = {}
        per_level[f"level_{top}_flow_match_ms"], _ = timed(torch, run_top, a.repeats)
        total = q["pyr_down_all_levels_both_images_ms"] + per_level[f"level_{top}_flow_match_ms"]
        for lv in range(top - 1, -1, -1):
            hh, ww = shapes[lv]
            prior = (torch.empty((hh, ww), dtype=torch.int16, device=dev), torch.empty((hh, ww), dtype=torch.int16, device=dev),
                     torch.empty((hh, ww), dtype=torch.uint8, device=dev))
            path = torch.empty(((hh + 15) // 16, (ww + 63) // 64), dtype=torch.uint8, device=dev)
            above = fields[lv + 1]
            run_up = lambda: eng.ctx.call("im_flow_prior_up", ptr(above[0]), ptr(above[1]), ptr(above[3]), *shapes[lv + 1], hh, ww, MEDIAN_RADIUS, MIN_COUNT,  # noqa: E731,B023
                                          *(ptr(t) for t in prior), eng.stream_ptr())  # noqa: B023
            run_field = lambda: eng.ctx.call("im_flow_match_field", ptr(pyr[lv][0]), ptr(pyr[lv][1]), hh, ww, RADIUS, FINE, *(ptr(t) for t in prior), MIN_VAR,  # noqa: E731,B023
                                             MIN_SCORE, None, *(ptr(t) for t in fields[lv]), ptr(path), eng.stream_ptr())  # noqa: B023
            per_level[f"level_{lv}_prior_up_ms"], _ = timed(torch, run_up, a.repeats)
            per_level[f"level_{lv}_match_field_ms"], per_level[f"level_{lv}_match_field_ms_all"] = timed(torch, run_field, a.repeats)
            total += per_level[f"level_{lv}_prior_up_ms"] + per_level[f"level_{lv}_match_field_ms"]
            counts = [int((path == k).sum().item()) for k in (0, 1, 2)]
            per_level[f"level_{lv}_tiles_nothing_tiled_direct"] = counts
            per_level[f"level_{lv}_share_of_tiles_direct"] = round(counts[2] / max(1, sum(counts)), 4)
            have = prior[2] != 0
            per_level[f"level_{lv}_share_of_pixels_with_a_prior"] = round(float(have.float().mean().item()), 4)
        q["per_level"] = per_level
        q["sum_of_the_levels_ms"] = total
        got = whole()
        q["whole_equals_the_levels"] = bool(all(torch.equal(x, y) for x, y in zip(got, fields[0])))
        valid = got.valid != 0
        hit = valid & (torch.round(got.du) == sx) & (torch.round(got.dv) == sy)
        inner = torch.zeros_like(valid)
        inner[RADIUS + max(0, -sy):h - RADIUS - max(0, sy), RADIUS + max(0, -sx):w - RADIUS - max(0, sx)] = True
        q["share_of_pixels_valid"] = round(float(valid.float().mean().item()), 4)
        q["share_of_valid_at_the_true_shift"] = round(float(hit.float().sum().item() / max(1.0, valid.float().sum().item())), 4)
        q["share_of_inner_pixels_valid_at_the_true_shift"] = round(float((hit & inner).float().sum().item() / inner.float().sum().item()), 4)
        # the single level on the same images, no prior
        single = outs((h, w))
        for name, (r, s) in SINGLE.items():
            run = lambda: eng.ctx.call("im_flow_match", ptr(ga), ptr(gb), h, w, r, s, 0, 0, MIN_VAR, MIN_SCORE, None, *(ptr(t) for t in single), eng.stream_ptr())  # noqa: E731,B023
            k = {}
            k["match_ms"], k["match_ms_all"] = timed(torch, run, a.repeats)
            v1 = single[3] != 0
            k["share_of_pixels_valid"] = round(float(v1.float().mean().item()), 4)
            k["share_of_inner_pixels_valid_at_the_true_shift"] = round(float((v1 & inner & (torch.round(single[0]) == sx) & (torch.round(single[1]) == sy)).float().sum().item()
                                                                             / inner.float().sum().item()), 4)
            k["pyramid_whole_over_this"] = round(q["match_flow_pyramid_whole_ms"] / k["match_ms"], 3)
            q[name] = k
        # the restatement of the whole pyramid on a crop, for scale and as a check on these images
        y0, x0 = (h - CROP) // 2, (w - CROP) // 2
        ca, cb = (np.ascontiguousarray(t[y0:y0 + CROP, x0:x0 + CROP].cpu().numpy()) for t in (ga, gb))
        t0 = time.perf_counter()
        want = PO.match_pyramid(ca, cb, None, LEVELS, RADIUS, SEARCH, FINE, (0, 0), MIN_VAR, MIN_SCORE, MEDIAN_RADIUS, MIN_COUNT)
        q[f"numpy_restatement_pyramid_{CROP}x{CROP}_crop_s"] = round(time.perf_counter() - t0, 3)
        c_got = DF.match_flow_pyramid(to_device(ca, dev), to_device(cb, dev), levels=LEVELS, radius=RADIUS, search=SEARCH, fine_search=FINE, min_var=MIN_VAR,
                                      min_score=MIN_SCORE, median_radius=MEDIAN_RADIUS, min_count=MIN_COUNT, engine=eng)
        equal = all(np.array_equal(g.cpu().numpy().view(np.uint8), np.ascontiguousarray(x).view(np.uint8)) for g, x in zip(c_got, want))
        q["crop_equal_to_the_restatement"] = bool(equal)
        q["crop_share_of_pixels_valid"] = round(float((want[3] != 0).mean()), 4)
        equal_all = equal_all and equal
        for k in list(q):
            if isinstance(q[k], float):
                q[k] = round(q[k], 4)
            elif isinstance(q[k], dict):
                q[k] = {n: (round(v, 4) if isinstance(v, float) else v) for n, v in q[k].items()}
        res["downscale"][str(f)] = q
        del ga, gb, pyr, fields, single, got
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not equal_all:
        sys.exit("the device output differs from the restatement on the crop")


if __name__ == "__main__":
    main()
