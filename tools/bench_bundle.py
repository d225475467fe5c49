"""Times the two-view bundle adjustment of csrc/ba.hip on the device (device events, one warm-up, median of the repeats): `--epochs`
epochs (default 256) of the synthetic stereo scene of tests/ba_cases.py (two cameras 30 m apart, a front 90 .. 150 m away, 0.5 px noise,
a perturbed start) with `--points` tie points (default 2000) and 6 control points each, default mask (both poses and f):
  - per iteration, at the start state, each of the four kernels alone: `im_ba_accumulate`, `im_ba_solve`, `im_ba_step_points`, `im_ba_decide`;
  - the whole run to convergence of all epochs (`sfm.ba_run_device`: uploads, 4 launches per iteration, one read-back), and the residuals;
  - for scale, `scipy.optimize.least_squares` (trf, sparse finite-difference Jacobian) on ONE epoch of the same problem on this host.
Before timing, epoch 0's history is compared with the restatement (tests/ba_oracle.py: bits). What bounds `im_ba_accumulate` is NOT measured
here (that takes a counter run of its own). No time is asserted and no target is set.

    python tools/bench_bundle.py [--epochs 256] [--points 2000] [--repeats 5] [--out profiles/r20_bundle_bench.json]"""
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


def scipy_one_epoch(O, c):
    """Seconds, cost and evaluations of scipy's least squares on one epoch: the same cost from the same start."""
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix
    cams0, X0, obs, sig, prior, cprior = (np.asarray(c[k], np.float64) for k in ("cams", "X", "obs", "sig", "prior", "cprior"))
    free = [p for p in range(O.DIM) if (c["mask"] >> p) & 1]
    n, nf = len(X0), len(free)
    has = prior[:, 3:] > 0

    def fun(v):
        x = np.zeros(O.DIM)
        x[free] = v[:nf]
        cams = np.concatenate([O.step_camera(cams0[24 * k:24 * k + 24], x[14 * k:14 * k + 14]) for k in range(2)])
        X = X0 + v[nf:].reshape(n, 3)
        out = []
        for k in range(2):
            p = O.project(cams[24 * k:24 * k + 24], X)
            out += [(p["u"] - obs[:, 2 * k]) / sig, (p["v"] - obs[:, 2 * k + 1]) / sig]
        out.append(((X - prior[:, :3]) / np.where(has, prior[:, 3:], 1.0))[has])
        for k in range(2):
            out.append((cams[24 * k + 9:24 * k + 12] - cprior[6 * k:6 * k + 3]) / cprior[6 * k + 3:6 * k + 6])
        return np.concatenate(out)

    m = 4 * n + int(has.sum()) + 6
    S = lil_matrix((m, nf + 3 * n), dtype=int)
    for k in range(2):
        cols = [j for j, p in enumerate(free) if p // 14 == k]
        for half in range(2):
            rows = np.arange(n) + (2 * k + half) * n
            for j in cols:
                S[rows, j] = 1
            for a in range(3):
                S[rows, nf + 3 * np.arange(n) + a] = 1
    pi, pa = np.nonzero(has)
    S[4 * n + np.arange(len(pi)), nf + 3 * pi + pa] = 1
    for k in range(2):
        for a in range(3):
            S[4 * n + len(pi) + 3 * k + a, [j for j, p in enumerate(free) if p // 14 == k]] = 1
    t0 = time.perf_counter()
    sol = least_squares(fun, np.zeros(nf + 3 * n), jac_sparsity=S, method="trf", x_scale="jac", xtol=1e-12, ftol=1e-12, gtol=1e-12, max_nfev=300)
    return time.perf_counter() - t0, float(sol.cost), int(sol.nfev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=256)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_bundle_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.epochs >= 1 and a.points >= 8
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_bundle.py needs a HIP device: there is nothing to time without one")
    import ba_cases as BC
    import ba_oracle as O
    from icepy4d_amd import sfm
    from icepy4d_amd._lib import ptr
    from icepy4d_amd.engine import Engine, to_device
    eng = Engine(0)
    dev, st = eng.device, eng.stream_ptr()
    E, n = a.epochs, a.points + BC.N_CONTROL
    cases = [BC.scene(n, seed=2000 + e, noise=0.5) for e in range(E)]
    problems = [{k: c[k] for k in ("cams", "X", "obs", "sig", "prior", "cprior")} for c in cases]
    opts, mask, lam = O.options(ftol=1e-9), O.MASK_DEFAULT, 1e-3
    res = {"device": torch.cuda.get_device_name(0), "epochs": E, "tie_points": a.points, "control_points": BC.N_CONTROL, "repeats": a.repeats,
           "scene": "tests/ba_cases.py scene(noise=0.5), seeds 2000 + epoch; default mask (both poses and f), lambda0 1e-3, ftol 1e-9, max_iter 30",
           "clock": "device events around the calls, one warm-up, median of the repeats",
           "unmeasured": "what bounds im_ba_accumulate: no counter run was made"}
    outs = sfm.ba_run_device(problems, mask, lam, opts, engine=eng)
    want = O.run(cases[0]["cams"], cases[0]["X"], cases[0]["obs"], cases[0]["sig"], cases[0]["prior"], cases[0]["cprior"], mask, opts, O.initial_state(lam))
    equal = np.array_equal(outs[0][3].view(np.uint64), want[3].view(np.uint64)) and np.array_equal(outs[0][1].view(np.uint64), want[1].view(np.uint64))
    res["epoch_0_equal_to_the_restatement"] = bool(equal)
    iters = [len(o[3]) for o in outs]
    res["iterations_min_median_max"] = [int(min(iters)), float(np.median(iters)), int(max(iters))]
    res["statuses"] = {name: int(sum(int(o[2][3]) == code for o in outs)) for code, name in sfm.BA_STATUS.items()}
    res["cost_first_last_epoch_0"] = [float(outs[0][3][0, 0]), float(outs[0][3][-1, 1])]
    res["whole_run_ms"], res["whole_run_ms_all"] = timed(torch, lambda: sfm.ba_run_device(problems, mask, lam, opts, engine=eng), a.repeats)
    res["whole_run_launch_rounds"] = int(opts[3])
    # the four kernels alone at the start state
    M = E * n
    f64 = lambda k, w: to_device(np.concatenate([np.asarray(c[k], np.float64).reshape(-1, w) for c in cases]), dev)
    pts2 = torch.zeros((2, M, 3), dtype=torch.float64, device=dev)
    pts2[0] = f64("X", 3)
    cams2 = torch.zeros((2, E, 48), dtype=torch.float64, device=dev)
    cams2[0] = f64("cams", 48)
    obs, sig, prior, cprior = f64("obs", 4), f64("sig", 1), f64("prior", 6), f64("cprior", 12)
    doff = to_device(np.arange(E + 1, dtype=np.int64) * n, dev)
    state0 = np.zeros((E, 8))
    state0[:, 0], state0[:, 3] = lam, -1.0
    state = to_device(state0, dev)
    keep_state = state.clone()
    sol = torch.zeros((E, 512), dtype=torch.float64, device=dev)
    hist = torch.zeros((30, E, 64), dtype=torch.float64, device=dev)
    h_opts = np.ascontiguousarray(opts)
    call = eng.ctx.call
    acc = lambda: call("im_ba_accumulate", ptr(doff), E, M, n, ptr(pts2), ptr(obs), ptr(sig), ptr(prior), ptr(cams2), ptr(state), None, st)
    slv = lambda: call("im_ba_solve", ptr(doff), E, M, None, ptr(cams2), ptr(cprior), ptr(state), mask, ptr(sol), st)
    stp = lambda: call("im_ba_step_points", ptr(doff), E, M, n, ptr(pts2), ptr(obs), ptr(sig), ptr(prior), ptr(cams2), ptr(state), ptr(sol), None, st)

    def dec():
        state.copy_(keep_state)                                            # the decision moves the state: every repeat decides the first step
        call("im_ba_decide", ptr(doff), E, M, None, ptr(cams2), ptr(cprior), ptr(state), ptr(sol), h_opts.ctypes.data, ptr(hist), 30, st)

    acc(), slv(), stp()
    res["accumulate_ms"], res["accumulate_ms_all"] = timed(torch, acc, a.repeats)
    res["solve_ms"], res["solve_ms_all"] = timed(torch, slv, a.repeats)
    res["step_points_ms"], res["step_points_ms_all"] = timed(torch, stp, a.repeats)
    res["decide_with_state_copy_ms"], res["decide_with_state_copy_ms_all"] = timed(torch, dec, a.repeats)
    res["iteration_ms"] = round(res["accumulate_ms"] + res["solve_ms"] + res["step_points_ms"] + res["decide_with_state_copy_ms"], 4)
    res["accumulate_bytes_kept_per_point"] = 95 * 8
    try:
        secs, cost, nfev = scipy_one_epoch(O, dict(cases[0], mask=mask))
        res["scipy_one_epoch"] = {"seconds": round(secs, 3), "cost": cost, "nfev": nfev, "our_cost": float(outs[0][3][-1, 1]),
                                  "host": "this host's CPU, one process; trf with a sparse finite-difference Jacobian"}
    except ImportError:
        res["scipy_one_epoch"] = None
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not equal:
        sys.exit("the device output differs from the restatement at the production size")


if __name__ == "__main__":
    main()
