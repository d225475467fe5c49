"""Dense surface displacement on the device: the three entry points of csrc/dense_flow.hip on every case of tests/flow_cases.py against the
restatement (tests/flow_oracle.py) bit for bit, every output between two bands of sentinel bytes and pre-filled, every launch run twice,
the inputs unchanged afterwards; the check on the device's own fields and on the restatement's uploaded ones, so that a match bug cannot
hide behind it; `surface_displacement` and `displacement_series` against the restatement's chain on maps that `build_depth_maps` made,
and their table through `compute_binned_stats2D`; the -83 refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_oracle as O  # noqa: E402
import flow_cases as C  # noqa: E402
import flow_oracle as FO  # noqa: E402

from icepy4d_amd.dense_flow import displacement_series, flow_consistency, lift_flow, match_flow, surface_displacement  # noqa: E402,F401  (the feature under test)
from test_gpu_sgm import Framed, bits, dev, p  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def unchanged(held, c, keys):
    assert all(bits(held[k].cpu().numpy(), c[k]) for k in keys if c[k] is not None and np.asarray(c[k]).size), "an input was written"


# ---- the three entry points -------------------------------------------------------------------------------------------------------------------------
def run_match(eng, c, /, outs=None, swap=False, **change):
    """`swap`: the backward match, b into a with the negated prior and every pixel asked."""
    held = {k: dev(eng, c[k]) for k in ("a", "b")}
    held["ask"] = None if c["ask"] is None or swap else dev(eng, c["ask"])
    h, w = c["a"].shape
    outs = outs or (Framed(eng, (h, w), np.float64), Framed(eng, (h, w), np.float64), Framed(eng, (h, w), np.float32), Framed(eng, (h, w), np.uint8))
    sign = -1 if swap else 1
    a = dict(a=held["b" if swap else "a"], b=held["a" if swap else "b"], h=h, w=w, r=c["r"], S=c["S"], pu=sign * c["prior"][0], pv=sign * c["prior"][1],
             min_var=c["min_var"], min_score=float(c["min_score"]), ask=held["ask"], du=outs[0].ptr, dv=outs[1].ptr, score=outs[2].ptr, valid=outs[3].ptr)
    a.update(change)
    rc = eng.ctx.lib.im_flow_match(eng.ctx.h, p(a["a"]), p(a["b"]), a["h"], a["w"], a["r"], a["S"], a["pu"], a["pv"], a["min_var"], a["min_score"], p(a["ask"]),
                                   a["du"], a["dv"], a["score"], a["valid"], eng.stream_ptr())
    eng.synchronize()
    unchanged(held, c, ("a", "b"))
    return rc, outs


def run_check(eng, c, /, fields=None, out=None, **change):
    """`fields`: six device addresses (the match entry point's own outputs) in place of the case's uploaded fields."""
    keys = ("du", "dv", "valid", "du_b", "dv_b", "valid_b")
    held = {k: dev(eng, c[k]) for k in keys}
    h, w = c["du"].shape
    out = out or Framed(eng, (h, w), np.uint8)
    a = dict(zip(keys, fields)) if fields is not None else dict(held)
    a.update(h=h, w=w, tol=float(c["tol"]), keep=out.ptr)
    a.update(change)
    rc = eng.ctx.lib.im_flow_check(eng.ctx.h, *(p(a[k]) for k in keys), a["h"], a["w"], a["tol"], a["keep"], eng.stream_ptr())
    eng.synchronize()
    unchanged(held, c, keys)
    return rc, out


LIFT_KEYS = ("du", "dv", "valid", "keep", "plane_a", "w_a", "plane_b", "w_b", "keep_b")


def run_lift(eng, c, /, outs=None, **change):
    held = {k: dev(eng, c[k]) for k in LIFT_KEYS}
    (h, w), (hb, wb) = c["du"].shape, c["plane_b"].shape
    outs = outs or (Framed(eng, (h, w, 3), np.float64), Framed(eng, (h, w, 3), np.float64), Framed(eng, (h, w), np.uint8))
    a = dict(held)
    a.update(h=h, w=w, hb=hb, wb=wb, cam_a=np.ascontiguousarray(c["cam_a"]), cam_b=np.ascontiguousarray(c["cam_b"]), w_step_b=float(c["w_step_b"]),
             max_diff=float(c["max_diff"]), P=outs[0].ptr, D=outs[1].ptr, ok=outs[2].ptr)
    a.update(change)
    rc = eng.ctx.lib.im_flow_lift(eng.ctx.h, *(p(a[k]) for k in LIFT_KEYS[:6]), a["h"], a["w"], p(a["cam_a"]), *(p(a[k]) for k in LIFT_KEYS[6:]), a["hb"], a["wb"],
                                  p(a["cam_b"]), a["w_step_b"], a["max_diff"], a["P"], a["D"], a["ok"], eng.stream_ptr())
    eng.synchronize()
    unchanged(held, c, LIFT_KEYS)
    return rc, outs


def differing(got, want):
    return [int((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).sum()) for g, w in zip(got, want)]


@pytest.mark.parametrize("name", list(C.matches()))
def test_match_equals_the_restatement_and_repeats(eng, name):
    c, want = C.matches()[name], C.match_expected(name)
    rc, outs = run_match(eng, c)
    got = [o.result(name) for o in outs]
    assert rc == 0 and all(bits(g, w) for g, w in zip(got, want)), (name, differing(got, want))
    rc, outs = run_match(eng, c, outs=outs)
    assert rc == 0 and all(bits(o.result(name), g) for o, g in zip(outs, got)), name


@pytest.mark.parametrize("name", list(C.checks()))
def test_check_equals_the_restatement_and_repeats(eng, name):
    c, want = C.checks()[name], C.check_expected(name)
    rc, out = run_check(eng, c)
    got = out.result(name)
    assert rc == 0 and bits(got, want), (name, int((got != want).sum()))
    rc, out = run_check(eng, c, out=out)
    assert rc == 0 and bits(out.result(name), got), name


@pytest.mark.parametrize("name", C.FROM_MATCH)
def test_check_on_the_devices_own_fields(eng, name):
    c = C.matches()[name]
    rc_f, fwd = run_match(eng, c)
    rc_b, bwd = run_match(eng, c, swap=True)
    assert rc_f == 0 and rc_b == 0 and all(bits(o.result(name), w) for o, w in zip(bwd, C.backward_expected(name)))
    rc, out = run_check(eng, C.checks()["from_match_" + name], fields=[fwd[0].ptr, fwd[1].ptr, fwd[3].ptr, bwd[0].ptr, bwd[1].ptr, bwd[3].ptr])
    assert rc == 0 and bits(out.result(name), C.check_expected("from_match_" + name)), name


@pytest.mark.parametrize("name", list(C.lifts()))
def test_lift_equals_the_restatement_and_repeats(eng, name):
    c, want = C.lifts()[name], C.lift_expected(name)
    rc, outs = run_lift(eng, c)
    got = [o.result(name) for o in outs]
    assert rc == 0 and all(bits(g, w) for g, w in zip(got, want)), (name, differing(got, want))
    rc, outs = run_lift(eng, c, outs=outs)
    assert rc == 0 and all(bits(o.result(name), g) for o, g in zip(outs, got)), name


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------------------
SHIFTS, DAYS, OPTIONS = ((0, 0), (2, 1), (5, -1)), (0, 2, 5), dict(radius=3, search=4, min_score=0.6)


def three_epochs():
    """`test_gpu_dense.python_pair` at three epochs: the same scene with both views moved by whole pixels (np.roll: the rim wraps around)."""
    import test_gpu_dense as TD
    images, cams, rng = TD.python_pair(False)
    return [[np.ascontiguousarray(np.roll(im, (sy, sx), (0, 1))) for im in images] for sx, sy in SHIFTS], cams, rng


def restated_epoch(images, cams, rng, camera):
    """The map of `camera` and its keep mask as the restatement's chain gives them: (dict for flow_oracle, keep)."""
    import test_gpu_dense as TD
    maps = TD.restated_maps(images, cams, rng, 1, 2, 0.6)
    m, o = maps[camera], maps[1 - camera]
    R, t = O.relative_pose(m["R"], m["t"], o["R"], o["t"])
    pose = np.concatenate([O.W.inv3(m["K"]).reshape(9), R.reshape(9), t, o["K"].reshape(9)])
    keep = O.consistency(m["out"][0], m["out"][1], o["out"][0], o["out"][1], pose, 1.0 * abs(o["w_step"]), True)
    return dict(grey=O.grey(m["image"]), plane=m["out"][0], w=m["out"][1], K=m["K"], R=m["R"], t=m["t"], w_step=m["w_step"]), keep


def same_field(got, want):
    return all(bits(g.cpu().numpy(), w) for g, w in zip(got, want))


@pytest.mark.parametrize("camera", [0, 1])
def test_python_layers_equal_the_restatements_chain(eng, camera):
    from icepy4d_amd import dense as D
    from icepy4d_amd.utils.binned_stats import compute_binned_stats2D
    epochs, cams, rng = three_epochs()
    maps = [D.build_depth_maps(images, cams, depth_range=rng, radius=2, min_score=0.6, engine=eng) for images in epochs]
    keeps = [[D.consistency(m[v], m[1 - v], "ModerateFiltering", engine=eng) for v in (0, 1)] for m in maps]
    want_maps = [restated_epoch(images, cams, rng, camera) for images in epochs]
    for e in range(3):
        assert bits(maps[e][camera].w.cpu().numpy(), want_maps[e][0]["w"]) and bits(keeps[e][camera].cpu().numpy(), want_maps[e][1]), e
    a, b = (maps[0][camera], keeps[0][camera]), (maps[1][camera], keeps[1][camera])
    for check in (True, False):
        got = surface_displacement(*a, *b, 2.0, check=check, engine=eng, **OPTIONS)
        want, fwd, keep, lifted = FO.surface_displacement(*want_maps[0], *want_maps[1], 2.0, check, **OPTIONS)
        assert len(want[0]) > 1000 and same_field(got, want), (camera, check, len(got.points), len(want[0]))
        assert (np.rint(fwd[0][lifted[2] != 0]) == SHIFTS[1][0]).mean() > 0.95                       # the seam of the roll goes astray
    # the pieces, against the same restatement
    field = match_flow(a[0].grey, b[0].grey, ask=a[1], engine=eng, **OPTIONS)
    back = match_flow(b[0].grey, a[0].grey, engine=eng, **OPTIONS)
    assert same_field(field, fwd)
    kept = flow_consistency(field, back, 1.0, engine=eng)
    want, fwd, keep, lifted = FO.surface_displacement(*want_maps[0], *want_maps[1], 2.0, True, **OPTIONS)
    assert bits(kept.cpu().numpy(), keep) and same_field(lift_flow(field, kept, a[0], b[0], b[1], 2.0, engine=eng), lifted)
    # the series: two pairs at lag 1, one at lag 2, with a prior that the second needs
    fields, table = displacement_series(maps, keeps, DAYS, camera=camera, engine=eng, **OPTIONS)
    wants = [FO.surface_displacement(*want_maps[e], *want_maps[e + 1], float(DAYS[e + 1] - DAYS[e]), True, **OPTIONS)[0] for e in (0, 1)]
    assert len(fields) == 2 and all(same_field(f, w) for f, w in zip(fields, wants))
    n = [len(w[0]) for w in wants]
    P, Dn, V = (np.concatenate([w[i] for w in wants]) for i in (0, 1, 2))
    assert list(table) == list(DF_COLS()) and all(len(table[k]) == sum(n) for k in table)
    for j, axis in enumerate("XYZ"):
        assert bits(table[f"{axis}_ini"], P[:, j]) and bits(table[f"{axis}_fin"], P[:, j] + Dn[:, j]) and bits(table[f"d{axis}"], Dn[:, j]) and bits(table[f"v{axis}"], V[:, j])
    assert bits(table["V"], np.sqrt((V[:, 0] * V[:, 0] + V[:, 1] * V[:, 1]) + V[:, 2] * V[:, 2]))
    assert bits(table["dt"], np.repeat([2.0, 3.0], n)) and bits(table["ep_ini"], np.repeat(np.array([0, 1], np.int64), n)) and bits(table["ep_fin"], np.repeat(np.array([1, 2], np.int64), n))
    fields, far = displacement_series(maps, keeps, ["2022_05_01", "2022_05_03", "2022_05_06"], camera=camera, lag=2, prior=SHIFTS[2], engine=eng, **OPTIONS)
    want = FO.surface_displacement(*want_maps[0], *want_maps[2], 5.0, True, prior=SHIFTS[2], **OPTIONS)[0]
    assert len(fields) == 1 and len(want[0]) > 1000 and same_field(fields[0], want) and (far["dt"] == 5.0).all() and (far["ep_fin"] == 2).all()
    # the table goes into the binned statistics as it is
    xy = np.stack([table["X_ini"], table["Y_ini"]], 1)
    xx, yy, count = compute_binned_stats2D(xy, table["V"], "count", step=0.5, engine=eng)
    _, _, mean = compute_binned_stats2D(xy, table["V"], "mean", step=0.5, engine=eng)
    assert count.shape == xx.shape == mean.shape and count.sum() == sum(n) and np.isfinite(mean[count > 0]).all()
    assert abs(np.nansum(mean * count) - table["V"].sum()) <= 1e-9 * table["V"].sum()


def DF_COLS():
    from icepy4d_amd.dense_flow import TABLE_COLS
    return TABLE_COLS


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
MATCH_REFUSALS = ([{k: None} for k in ("a", "b", "du", "dv", "score", "valid")]
                  + [dict(h=0), dict(h=16385), dict(w=0), dict(w=16385), dict(r=0), dict(r=16), dict(S=-1), dict(S=17), dict(pu=4097), dict(pu=-4097), dict(pv=4097),
                     dict(pv=-4097), dict(min_var=-1), dict(min_var=(1 << 26) + 1), dict(min_score=NAN), dict(min_score=INF), dict(min_score=-INF)])
CHECK_REFUSALS = ([{k: None} for k in ("du", "dv", "valid", "du_b", "dv_b", "valid_b", "keep")]
                  + [dict(h=0), dict(h=16385), dict(w=0), dict(w=16385), dict(tol=0.0), dict(tol=-1.0), dict(tol=NAN), dict(tol=INF)])
LIFT_REFUSALS = ([{k: None} for k in LIFT_KEYS + ("cam_a", "cam_b", "P", "D", "ok")]
                 + [dict(h=0), dict(h=16385), dict(w=0), dict(w=16385), dict(hb=0), dict(hb=16385), dict(wb=0), dict(wb=16385), dict(max_diff=0.0), dict(max_diff=-2.0),
                    dict(max_diff=NAN), dict(max_diff=INF), dict(w_step_b=0.0), dict(w_step_b=NAN), dict(w_step_b=INF), dict(w_step_b=-INF)])


def ids(changes):
    return [",".join(f"{k}={v}" for k, v in c.items()) for c in changes]


@pytest.mark.parametrize("change", MATCH_REFUSALS, ids=ids(MATCH_REFUSALS))
def test_match_refusals_launch_nothing(eng, change):
    rc, outs = run_match(eng, C.matches()["shape_17x65_r7_S4"], **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)


@pytest.mark.parametrize("change", CHECK_REFUSALS, ids=ids(CHECK_REFUSALS))
def test_check_refusals_launch_nothing(eng, change):
    rc, out = run_check(eng, C.checks()["crafted_15x63"], **change)
    assert rc == -83
    out.untouched(change)


@pytest.mark.parametrize("change", LIFT_REFUSALS, ids=ids(LIFT_REFUSALS))
def test_lift_refusals_launch_nothing(eng, change):
    rc, outs = run_lift(eng, C.lifts()["shape_17x65"], **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)
