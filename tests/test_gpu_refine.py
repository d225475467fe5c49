"""Slanted-window refinement on the device: the two entry points of csrc/dense_refine.hip on every case of tests/refine_cases.py against the
restatement (tests/refine_oracle.py) bit for bit, every output between two bands of sentinel bytes and pre-filled, every launch run twice;
the refinement on the restatement's slant and on the device's own, so that a slant bug cannot hide behind it; `refine_slanted` and
`build_depth_maps(refine=...)` against the restatement's chain, and `refine=None` against today's output; the -83 refusals; one refined
cloud through `fuse` and through the Poisson stage."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_oracle as O  # noqa: E402
import refine_cases as C  # noqa: E402
import refine_oracle as RO  # noqa: E402

from icepy4d_amd.dense import refine_slanted, slant_map  # noqa: E402,F401  (the feature under test: without it nothing here can pass)
from test_gpu_sgm import Framed, bits, dev, p  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


# ---- the two entry points ---------------------------------------------------------------------------------------------------------------------------
def run_slant(eng, c, /, outs=None, **change):
    held = {k: dev(eng, c[k]) for k in ("plane", "w")}
    h, w = c["plane"].shape
    outs = outs or (Framed(eng, (h, w, 2), np.float64), Framed(eng, (h, w), np.uint8))
    a = dict(plane=held["plane"], w=held["w"], h=h, w_=w, w_step=float(c["w_step"]), R=c["R"], max_diff=float(c["max_diff"]), min_count=c["min_count"],
             slant=outs[0].ptr, fitted=outs[1].ptr)
    a.update(change)
    rc = eng.ctx.lib.im_dense_slant(eng.ctx.h, p(a["plane"]), p(a["w"]), a["h"], a["w_"], a["w_step"], a["R"], a["max_diff"], a["min_count"], a["slant"],
                                    a["fitted"], eng.stream_ptr())
    eng.synchronize()
    return rc, outs


def run_refine(eng, c, slant, /, outs=None, **change):
    """`slant`: a device address (the slant entry point's own output) or a host array, which is uploaded."""
    held = {k: dev(eng, c[k]) for k in ("ref", "src", "plane", "w", "score")}
    if isinstance(slant, np.ndarray):
        held["slant"] = dev(eng, slant)
        slant = held["slant"].data_ptr()
    (h0, w0), (h1, w1) = c["ref"].shape, c["src"].shape
    outs = outs or (Framed(eng, (h0, w0), np.float64), Framed(eng, (h0, w0), np.float32), Framed(eng, (h0, w0), np.uint8))
    a = dict(ref=held["ref"], h0=h0, w0=w0, src=held["src"], h1=h1, w1=w1, A=np.ascontiguousarray(c["A"], np.float64), B=np.ascontiguousarray(c["B"], np.float64),
             plane=held["plane"], w=held["w"], score=held["score"], slant=slant, w_step=float(c["w_step"]), r=c["r"], min_var=c["min_var"], span=c["span"],
             sub=c["sub"], w_out=outs[0].ptr, score_out=outs[1].ptr, taken=outs[2].ptr)
    a.update(change)
    rc = eng.ctx.lib.im_dense_refine(eng.ctx.h, p(a["ref"]), a["h0"], a["w0"], p(a["src"]), a["h1"], a["w1"], p(a["A"]), p(a["B"]), p(a["plane"]), p(a["w"]),
                                     p(a["score"]), p(a["slant"]), a["w_step"], a["r"], a["min_var"], a["span"], a["sub"], a["w_out"], a["score_out"], a["taken"],
                                     eng.stream_ptr())
    eng.synchronize()
    before = [held[k].cpu().numpy() for k in ("plane", "w", "score")]
    assert all(bits(b, c[k]) for b, k in zip(before, ("plane", "w", "score"))), "an input was written"
    return rc, outs


@pytest.mark.parametrize("name", list(C.cases()))
def test_both_entry_points_equal_the_restatement_and_repeat(eng, name):
    c, want = C.cases()[name], C.expected(name)
    rc, outs = run_slant(eng, c)
    got = [o.result(name) for o in outs]
    assert rc == 0 and bits(got[0], want[0]) and bits(got[1], want[1]), (name, int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum()))
    rc, outs = run_slant(eng, c, outs=outs)
    assert rc == 0 and all(bits(o.result(name), g) for o, g in zip(outs, got)), name
    for slant in (outs[0].ptr, want[0]):                                          # the device's own slant, then the restatement's uploaded
        rc, r_outs = run_refine(eng, c, slant)
        r_got = [o.result(name) for o in r_outs]
        assert rc == 0 and all(bits(g, w) for g, w in zip(r_got, want[2:])), (name, [int((g.view(np.uint8) != w.view(np.uint8)).sum()) for g, w in zip(r_got, want[2:])])
        rc, r_outs = run_refine(eng, c, slant, outs=r_outs)
        assert rc == 0 and all(bits(o.result(name), g) for o, g in zip(r_outs, r_got)), name


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------------------
def restated_refinement(maps, v, radius, **options):
    """The restatement's chain behind the sweep on view v of `test_gpu_dense.restated_maps`: (w, score, taken)."""
    m, o = maps[v], maps[1 - v]
    R, t = O.relative_pose(m["R"], m["t"], o["R"], o["t"])
    A, B = O.sweep_matrices(m["K"], o["K"], R, t)
    plane, w, score = m["out"]
    return RO.refine_slanted(O.grey(m["image"]), O.grey(o["image"]), A, B, plane, w, score, m["w_step"], r=radius, min_var=4, **options)[:3]


@pytest.mark.parametrize("downscale", [1, 2])
@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_python_layers_equal_the_restatements_chain(eng, downscale, rgb):
    from icepy4d_amd import dense as D
    import test_gpu_dense as TD
    images, cams, rng = TD.python_pair(rgb)
    want_maps = TD.restated_maps(images, cams, rng, downscale, 2, 0.6)
    opts = dict(depth_range=rng, downscale=downscale, radius=2, min_score=0.6, engine=eng)
    plain = D.build_depth_maps(images, cams, **opts)
    none = D.build_depth_maps(images, cams, refine=None, **opts)
    for v in (0, 1):
        for f, w in zip(("plane", "w", "score"), want_maps[v]["out"]):
            assert bits(getattr(plain[v], f).cpu().numpy(), w) and bits(getattr(none[v], f).cpu().numpy(), w), (v, f)      # today's maps, bit for bit
    for passes in (1, 2):
        options = dict(passes=passes, fit_radius=3, sub=2)
        got = D.build_depth_maps(images, cams, refine=options, **opts)
        again = D.build_depth_maps(images, cams, refine=options, **opts)
        for v in (0, 1):
            w, score, taken = restated_refinement(want_maps, v, 2, **options)
            assert taken.sum() > 100 and (score > want_maps[v]["out"][2]).sum() > 100
            assert bits(got[v].plane.cpu().numpy(), want_maps[v]["out"][0])                                               # the label is never changed
            assert bits(got[v].w.cpu().numpy(), w) and bits(got[v].score.cpu().numpy(), score), (v, passes)
            assert all(bits(getattr(got[v], f).cpu().numpy(), getattr(again[v], f).cpu().numpy()) for f in ("plane", "w", "score"))      # two runs
            m, last = refine_slanted(plain[v], plain[1 - v], radius=2, engine=eng, return_taken=True, **options)
            assert bits(m.w.cpu().numpy(), w) and bits(m.score.cpu().numpy(), score) and bits(last.cpu().numpy(), taken), (v, passes)
            assert bits(plain[v].w.cpu().numpy(), want_maps[v]["out"][1])                                                 # the input is as it was
    pair = D.build_depth_maps(images, cams, refine=(2, 4), **opts)
    for v in (0, 1):
        w, score, _ = restated_refinement(want_maps, v, 2, passes=2, fit_radius=4)
        assert bits(pair[v].w.cpu().numpy(), w) and bits(pair[v].score.cpu().numpy(), score), v
    sl, fitted = slant_map(plain[0], 3, 2.0, 6, engine=eng)
    want = RO.slant(want_maps[0]["out"][0], want_maps[0]["out"][1], want_maps[0]["w_step"], 3, 2.0, 6)
    assert bits(sl.cpu().numpy(), want[0]) and bits(fitted.cpu().numpy(), want[1]) and want[1].sum() > 100


def test_a_refined_cloud_goes_through_fuse_and_the_poisson_stage(eng):
    from icepy4d_amd import dense as D
    from icepy4d_amd.post_processing.poisson import poisson_reconstruct
    import test_gpu_dense as TD
    images, cams, rng = TD.python_pair(False)
    opts = dict(depth_filter="ModerateFiltering", depth_range=rng, radius=2, min_score=0.6, engine=eng, views=(0, 1))
    plain = D.build_dense_cloud(images, cams, holes=(16, 2), **opts)
    pcd = D.build_dense_cloud(images, cams, holes=(16, 2), refine=(2, 4), **opts)
    assert len(pcd) > 1000 and pcd.confidence.astype(np.float64).mean() > plain.confidence.astype(np.float64).mean()
    fused = D.build_dense_cloud(images, cams, refine=(2, 4), fuse=(1.0, 1), **opts)
    assert 1000 < len(fused) < len(pcd) and set(np.unique(fused.views)) <= {1, 2} and (fused.views == 2).sum() > 1000
    has = np.linalg.norm(fused.normals, axis=1) > 0
    assert has.mean() > 0.9
    vertices, triangles, densities = poisson_reconstruct(fused.points[has], fused.normals[has], depth=5, engine=eng)
    assert len(vertices) > 0 and len(triangles) > 0 and len(densities) == len(vertices) and np.isfinite(vertices).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
SLANT_REFUSALS = ([{k: None} for k in ("plane", "w", "slant", "fitted")]
                  + [dict(h=0), dict(h=16385), dict(w_=0), dict(w_=16385), dict(R=0), dict(R=8), dict(max_diff=0.0), dict(max_diff=-1.0), dict(max_diff=64.5),
                     dict(max_diff=float("nan")), dict(max_diff=float("inf")), dict(min_count=2), dict(min_count=226), dict(w_step=0.0),
                     dict(w_step=float("nan")), dict(w_step=float("inf")), dict(w_step=float("-inf"))])
REFINE_REFUSALS = ([{k: None} for k in ("ref", "src", "A", "B", "plane", "w", "score", "slant", "w_out", "score_out", "taken")]
                   + [dict(h0=0), dict(h0=16385), dict(w0=0), dict(w0=16385), dict(h1=0), dict(h1=16385), dict(w1=0), dict(w1=16385), dict(r=0), dict(r=8),
                      dict(span=0), dict(span=5), dict(sub=0), dict(sub=9), dict(min_var=-1), dict(min_var=(1 << 26) + 1), dict(w_step=0.0),
                      dict(w_step=float("nan")), dict(w_step=float("inf"))])


def ids(changes):
    return [",".join(f"{k}={v}" for k, v in c.items()) for c in changes]


@pytest.mark.parametrize("change", SLANT_REFUSALS, ids=ids(SLANT_REFUSALS))
def test_slant_refusals_launch_nothing(eng, change):
    rc, outs = run_slant(eng, C.cases()["shape_17x65_r3_R3_span1_sub1"], **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)


@pytest.mark.parametrize("change", REFINE_REFUSALS, ids=ids(REFINE_REFUSALS))
def test_refine_refusals_launch_nothing(eng, change):
    name = "shape_17x65_r3_R3_span1_sub1"
    rc, outs = run_refine(eng, C.cases()[name], C.expected(name)[0], **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)
