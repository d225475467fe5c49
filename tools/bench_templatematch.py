#!/usr/bin/env python3
"""Throughput of the template-matching correlation (`im_template_match_oc`, csrc/templatematch.hip) on one MI355X. Prints ONE JSON
line with two configs:
  dense   a displacement field on a 24 MP pair (4000 x 6000): TemplateMatch defaults 128 / 144, grid step 32 (~23 k points)
  track   20 targets x 200 epochs at the TrackTargets defaults 32 / 128 (one A image, 200 B images of 1000 x 1500)
For each: pairs/s and ms of the correlation launch alone (orientation maps already on the device, median of --reps timed calls),
the end-to-end time of `match_many` (uploads and forient included), and the FP32 rate counting 4 T^2 (S - T)^2 FLOP per
correlated pair, also as a fraction of the 157.3 TFLOP/s FP32 vector peak.

    python tools/bench_templatematch.py [--reps 10] [--config dense|track|both]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_VALU_TFLOPS = 157.3


def smooth_image(rng, h, w):
    from scipy import ndimage
    small = ndimage.gaussian_filter(rng.normal(0, 1, (h // 4 + 8, w // 4 + 8)), 2.0)
    big = np.kron(small, np.ones((4, 4)))[:h, :w] + rng.normal(0, 0.15, (h, w))
    return np.clip((big - big.min()) / (big.max() - big.min()) * 255, 0, 255).astype(np.uint8)


def run(eng, A, Bs, pu, pv, T, S, reps):
    import torch
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.matching.templatematch import _device_maps, match_many
    t0 = time.perf_counter()
    r = match_many(A, Bs, pu, pv, T, S, engine=eng)
    e2e_ms = (time.perf_counter() - t0) * 1e3
    dA, dB = _device_maps(eng, [A], False), _device_maps(eng, Bs, False)
    n_b = len(Bs)
    pts = np.stack([pu.ravel(), pv.ravel(), np.zeros(pu.size), np.zeros(pu.size)], 1)
    d_pairs = torch.from_numpy(np.ascontiguousarray(np.tile(pts, (n_b, 1)))).to(eng.device)
    d_bidx = torch.from_numpy(np.repeat(np.arange(n_b, dtype=np.int32), pu.size)).to(eng.device)
    n = pu.size * n_b
    d_out = torch.empty((6, n), dtype=torch.float64, device=eng.device)
    args = (ptr(dA), A.shape[0], A.shape[1], ptr(dB), n_b, Bs[0].shape[0], Bs[0].shape[1], ptr(d_pairs), ptr(d_bidx), n, T, S, 1, ptr(d_out),
            eng.stream_ptr())
    eng.ctx.call("im_template_match_oc", *args)   # warm-up
    eng.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.ctx.call("im_template_match_oc", *args)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    valid = int(np.isfinite(r["meanAbsCorr"]).sum())
    gflop = 4.0 * T * T * (S - T) ** 2 * valid / 1e9
    return {"T": T, "S": S, "pairs": n, "pairs_correlated": valid, "ms": round(ms, 3), "ms_min": round(min(times), 3),
            "pairs_per_s": round(n / ms * 1e3, 1), "gflop": round(gflop, 2), "tflop_per_s": round(gflop / ms, 2),
            "fraction_of_fp32_peak": round(gflop / ms / PEAK_F32_VALU_TFLOPS, 4), "match_many_e2e_ms": round(e2e_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--config", choices=["dense", "track", "both"], default="both")
    a = ap.parse_args()
    from icepy4d_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(0)
    out = {"bench": "templatematch"}
    if a.config in ("dense", "both"):
        A = smooth_image(rng, 4000, 6000)
        B = np.roll(A, (3, -5), axis=(0, 1))
        T, S = 128, 144
        xs = np.arange(S / 2, A.shape[1] - S / 2 + T / 2, 32)
        ys = np.arange(S / 2, A.shape[0] - S / 2 + T / 2, 32)
        pu, pv = np.meshgrid(xs, ys)
        out["dense"] = run(eng, A, [B], pu, pv, T, S, a.reps)
    if a.config in ("track", "both"):
        A = smooth_image(rng, 1000, 1500)
        Bs = [np.roll(A, (int(rng.integers(-8, 9)), int(rng.integers(-8, 9))), axis=(0, 1)) for _ in range(200)]
        tg = np.stack([rng.uniform(100, 1400, 20), rng.uniform(100, 900, 20)], 1)
        out["track"] = run(eng, A, Bs, tg[:, 0], tg[:, 1], 32, 128, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
