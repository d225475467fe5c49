"""Coarse-to-fine dense displacement on the device: the two entry points of csrc/dense_flow_field.hip on every case of
tests/pyrflow_cases.py against the restatement (tests/pyrflow_oracle.py) bit for bit, every output between two bands of sentinel bytes
and pre-filled, every launch run twice, the inputs unchanged afterwards, the path of every tile as the restatement's rule names it; a
constant field against `im_flow_match`'s own output; `match_flow_pyramid`, `surface_displacement` and `displacement_series` with more
than one level against the restatement's chain; the -83 refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyrflow_cases as C  # noqa: E402
import pyrflow_oracle as PO  # noqa: E402

from icepy4d_amd.dense_flow import (FlowField, PriorField, displacement_series, match_flow_field, match_flow_pyramid, prior_field_up,  # noqa: E402,F401
                                    surface_displacement)  # the feature under test: without it nothing here can pass
from test_gpu_flow import OPTIONS, SHIFTS, differing, restated_epoch, same_field, three_epochs, unchanged  # noqa: E402
from test_gpu_sgm import Framed, bits, dev, p  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


# ---- the two entry points ---------------------------------------------------------------------------------------------------------------------------
UP_KEYS = ("du", "dv", "valid")


def run_up(eng, c, /, outs=None, **change):
    held = {k: dev(eng, c[k]) for k in UP_KEYS}
    (hc, wc), (h, w) = c["du"].shape, c["shape"]
    outs = outs or (Framed(eng, (h, w), np.int16), Framed(eng, (h, w), np.int16), Framed(eng, (h, w), np.uint8))
    a = dict(held)
    a.update(hc=hc, wc=wc, h=h, w=w, m=c["m"], min_count=c["min_count"], pu=outs[0].ptr, pv=outs[1].ptr, have=outs[2].ptr)
    a.update(change)
    rc = eng.ctx.lib.im_flow_prior_up(eng.ctx.h, p(a["du"]), p(a["dv"]), p(a["valid"]), a["hc"], a["wc"], a["h"], a["w"], a["m"], a["min_count"], a["pu"], a["pv"],
                                      a["have"], eng.stream_ptr())
    eng.synchronize()
    unchanged(held, c, UP_KEYS)
    return rc, outs


FIELD_KEYS = ("a", "b", "pu", "pv", "have", "ask")


def blocks(shape):
    return ((shape[0] + 15) // 16, (shape[1] + 63) // 64)


def run_field(eng, c, /, outs=None, with_path=True, **change):
    """outs: du, dv, score, valid and, `with_path`, the tile paths."""
    held = {k: (None if c[k] is None else dev(eng, c[k])) for k in FIELD_KEYS}
    h, w = c["a"].shape
    outs = outs or (Framed(eng, (h, w), np.float64), Framed(eng, (h, w), np.float64), Framed(eng, (h, w), np.float32), Framed(eng, (h, w), np.uint8),
                    Framed(eng, blocks((h, w)), np.uint8))
    a = dict(held)
    a.update(h=h, w=w, r=c["r"], S=c["S"], min_var=c["min_var"], min_score=float(c["min_score"]), du=outs[0].ptr, dv=outs[1].ptr, score=outs[2].ptr,
             valid=outs[3].ptr, path=outs[4].ptr if with_path else None)
    a.update(change)
    rc = eng.ctx.lib.im_flow_match_field(eng.ctx.h, p(a["a"]), p(a["b"]), a["h"], a["w"], a["r"], a["S"], p(a["pu"]), p(a["pv"]), p(a["have"]), a["min_var"],
                                         a["min_score"], p(a["ask"]), a["du"], a["dv"], a["score"], a["valid"], a["path"], eng.stream_ptr())
    eng.synchronize()
    unchanged(held, c, FIELD_KEYS)
    return rc, outs


@pytest.mark.parametrize("name", list(C.ups()))
def test_prior_up_equals_the_restatement_and_repeats(eng, name):
    c, want = C.ups()[name], C.up_expected(name)
    rc, outs = run_up(eng, c)
    got = [o.result(name) for o in outs]
    assert rc == 0 and all(bits(g, w) for g, w in zip(got, want)), (name, differing(got, want))
    rc, outs = run_up(eng, c, outs=outs)
    assert rc == 0 and all(bits(o.result(name), g) for o, g in zip(outs, got)), name


@pytest.mark.parametrize("name", list(C.fields()))
def test_field_match_equals_the_restatement_and_repeats(eng, name):
    """With the tile paths given, then again into the same outputs, then with a null d_tile_path: the same bits each time."""
    c, want = C.fields()[name], C.field_expected(name)
    rc, outs = run_field(eng, c)
    got = [o.result(name) for o in outs]
    assert rc == 0 and all(bits(g, w) for g, w in zip(got[:4], want)), (name, differing(got[:4], want))
    assert bits(got[4], C.field_paths(name)), (name, got[4].tolist(), C.field_paths(name).tolist())
    rc, outs = run_field(eng, c, outs=outs)
    assert rc == 0 and all(bits(o.result(name), g) for o, g in zip(outs, got)), name
    rc, plain = run_field(eng, c, with_path=False)
    assert rc == 0 and all(bits(o.result(name), g) for o, g in zip(plain[:4], got)), name
    plain[4].untouched(name)


@pytest.mark.parametrize("name", [n for n, c in C.fields().items() if C.is_constant(c)])
def test_a_constant_field_is_the_single_level_match(eng, name):
    """Against `im_flow_match`'s own output for that global prior, not the restatement's."""
    c = C.fields()[name]
    h, w = c["a"].shape
    a, b = dev(eng, c["a"]), dev(eng, c["b"])
    outs = (Framed(eng, (h, w), np.float64), Framed(eng, (h, w), np.float64), Framed(eng, (h, w), np.float32), Framed(eng, (h, w), np.uint8))
    rc = eng.ctx.lib.im_flow_match(eng.ctx.h, p(a), p(b), h, w, c["r"], c["S"], int(c["pu"][0, 0]), int(c["pv"][0, 0]), c["min_var"], float(c["min_score"]), None,
                                   *(o.ptr for o in outs), eng.stream_ptr())
    eng.synchronize()
    rc_f, field = run_field(eng, c)
    assert rc == 0 and rc_f == 0 and all(bits(f.result(name), o.result(name)) for f, o in zip(field, outs)), name


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.DEVICE_PYRAMIDS)
def test_the_pyramid_equals_the_restatements_chain(eng, name):
    import torch
    c, (want, trace) = C.pyramids()[name], C.pyramid_expected(name)
    a, b = dev(eng, c["a"]), dev(eng, c["b"])
    ask = None if c["ask"] is None else dev(eng, c["ask"])
    paths = []
    got = match_flow_pyramid(a, b, ask=ask, levels=c["levels"], radius=c["r"], search=c["S"], fine_search=c["fine"], prior=c["prior"], min_var=c["min_var"],
                             min_score=c["min_score"], median_radius=c["m"], min_count=c["min_count"], engine=eng, tile_paths=paths)
    assert want[3].sum() > 2000 and same_field(got, want), (name, differing([t.cpu().numpy() for t in got], want))
    assert len(paths) == len(trace) == c["levels"] - 1 and all(bits(g.cpu().numpy(), t[2]) for g, t in zip(paths, trace))
    assert bits(a.cpu().numpy(), c["a"]) and bits(b.cpu().numpy(), c["b"])
    # the pieces by hand on the restatement's coarse field: the prior of level 0 and the match around it
    la, lb = PO.levels_of(c["a"], 2), PO.levels_of(c["b"], 2)
    if c["levels"] == 2:
        import flow_oracle as FO
        coarse = FO.match(la[1], lb[1], None, c["r"], c["S"], (PO.coarse_prior(c["prior"][0], 2), PO.coarse_prior(c["prior"][1], 2)), c["min_var"], c["min_score"])
        field = FlowField(*(torch.from_numpy(np.ascontiguousarray(x)).to(eng.device) for x in coarse))
        pf = prior_field_up(field, c["a"].shape, c["m"], c["min_count"], engine=eng)
        assert isinstance(pf, PriorField) and all(bits(g.cpu().numpy(), x) for g, x in zip(pf, trace[0][1]))
        assert same_field(match_flow_field(a, b, pf, ask=ask, radius=c["r"], search=c["fine"], min_var=c["min_var"], min_score=c["min_score"], engine=eng), want)


def test_the_stage_with_two_levels_equals_the_restatements_chain(eng):
    """`surface_displacement` and `displacement_series` with levels = 2 on maps that `build_depth_maps` made, camera 0, against the
    restatement's chain; levels = 1 equals the call without the option. The pair two epochs apart has moved by (5, -1): beyond search 2
    at one level, inside the reach 2 x 2 + 1 x 1 = 5 of two."""
    from icepy4d_amd import dense as D
    camera = 0
    epochs, cams, rng = three_epochs()
    maps = [D.build_depth_maps(images, cams, depth_range=rng, radius=2, min_score=0.6, engine=eng) for images in epochs]
    keeps = [[D.consistency(m[v], m[1 - v], "ModerateFiltering", engine=eng) for v in (0, 1)] for m in maps]
    want_maps = [restated_epoch(images, cams, rng, camera) for images in epochs]
    a, b, far = ((maps[e][camera], keeps[e][camera]) for e in (0, 1, 2))
    plain = surface_displacement(*a, *b, 2.0, engine=eng, **OPTIONS)
    assert len(plain.points) > 1000 and all(bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(surface_displacement(*a, *b, 2.0, engine=eng, levels=1, **OPTIONS), plain))
    two = dict(OPTIONS, levels=2, search=2, fine_search=1)
    for check in (True, False):
        got = surface_displacement(*a, *far, 5.0, check=check, engine=eng, **two)
        want, fwd, keep, lifted = PO.surface_displacement(*want_maps[0], *want_maps[2], 5.0, check, **two)
        assert len(want[0]) > 1000 and same_field(got, want), (check, len(got.points), len(want[0]))
        assert (np.rint(fwd[0][lifted[2] != 0]) == SHIFTS[2][0]).mean() > 0.9 and (np.rint(fwd[1][lifted[2] != 0]) == SHIFTS[2][1]).mean() > 0.9
    one = surface_displacement(*a, *far, 5.0, engine=eng, **dict(OPTIONS, search=2))                  # one level at the same search does not get there
    assert len(one.points) < len(got.points) / 4
    fields, table = displacement_series(maps, keeps, (0, 2, 5), camera=camera, lag=2, engine=eng, **two)
    want = PO.surface_displacement(*want_maps[0], *want_maps[2], 5.0, True, **two)[0]
    assert len(fields) == 1 and same_field(fields[0], want) and len(table["dt"]) == len(want[0]) and (table["dt"] == 5.0).all() and bits(table["dX"], want[1][:, 0])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
UP_REFUSALS = ([{k: None} for k in ("du", "dv", "valid", "pu", "pv", "have")]
               + [dict(h=0), dict(w=0), dict(h=16385, hc=8193), dict(w=16385, wc=8193), dict(hc=0), dict(wc=0), dict(hc=10), dict(hc=8), dict(wc=34), dict(wc=32),
                  dict(h=19), dict(h=16), dict(w=67), dict(w=64), dict(m=-1), dict(m=3), dict(min_count=0), dict(min_count=10), dict(m=0, min_count=2), dict(m=2, min_count=26)])
FIELD_REFUSALS = ([{k: None} for k in ("a", "b", "pu", "pv", "have", "du", "dv", "score", "valid")]
                  + [dict(h=0), dict(h=16385), dict(w=0), dict(w=16385), dict(r=0), dict(r=16), dict(S=-1), dict(S=17), dict(min_var=-1), dict(min_var=(1 << 26) + 1),
                     dict(min_score=NAN), dict(min_score=INF), dict(min_score=-INF)])


def ids(changes):
    return [",".join(f"{k}={v}" for k, v in c.items()) for c in changes]


@pytest.mark.parametrize("change", UP_REFUSALS, ids=ids(UP_REFUSALS))
def test_prior_up_refusals_launch_nothing(eng, change):
    rc, outs = run_up(eng, C.ups()["up_9x33_to_17x65_m1_count1"], **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)


@pytest.mark.parametrize("change", FIELD_REFUSALS, ids=ids(FIELD_REFUSALS))
def test_field_match_refusals_launch_nothing(eng, change):
    rc, outs = run_field(eng, C.fields()["constant_17x65_r7_S2"], **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)
