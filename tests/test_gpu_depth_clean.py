"""Depth-map clean-up on the device: the three entry points of csrc/depth_clean.hip on every case of tests/depth_cases.py against the
restatement (tests/depth_oracle.py) bit for bit, every output between two bands of sentinel bytes and pre-filled; every labelling run
twice; the drop and the fill on the device's own labels and on uploaded ones, so that a labelling bug cannot hide behind them;
`build_depth_maps` and `build_dense_cloud` with `speckle` and `holes` against the restatement's chain, and without them against today's
output; the three noisy scenes; the -83 refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as C  # noqa: E402
import depth_oracle as DO  # noqa: E402
import sgm_cases as SC  # noqa: E402

from icepy4d_amd.dense import depth_components, remove_speckles, fill_holes  # noqa: E402,F401  (the feature under test: without it nothing here can pass)
from test_gpu_sgm import BAND, Framed, bits, dev  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def test_the_tile_is_the_one_the_cases_are_built_for(eng):
    assert (eng.ctx.lib.im_depth_tile_w(), eng.ctx.lib.im_depth_tile_h()) == (C.TILE_W, C.TILE_H)


# ---- labelling ----------------------------------------------------------------------------------------------------------------------------------
def run_components(eng, plane, mode, max_diff, /, outs=None, **change):
    held = dev(eng, plane)
    h, w = plane.shape
    outs = outs or (Framed(eng, (h, w), np.int32), Framed(eng, (h, w), np.int32))
    a = dict(plane=held.data_ptr(), h=h, w=w, mode=mode, max_diff=max_diff, label=outs[0].ptr, size=outs[1].ptr)
    a.update(change)
    rc = eng.ctx.lib.im_depth_components(eng.ctx.h, a["plane"], a["h"], a["w"], a["mode"], a["max_diff"], a["label"], a["size"], eng.stream_ptr())
    eng.synchronize()
    return rc, outs


@pytest.mark.parametrize("name", list(C.labellings()))
def test_components_equal_the_restatement_and_repeat(eng, name):
    plane, mode, max_diff = C.labellings()[name]
    want = C.label_oracle(name)
    rc, outs = run_components(eng, plane, mode, max_diff)
    got = [o.result(name) for o in outs]
    assert rc == 0 and bits(got[0], want[0]) and bits(got[1], want[1]), (name, int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum()))
    rc, outs = run_components(eng, plane, mode, max_diff, outs=outs)              # over its own result
    again = [o.result(name) for o in outs]
    assert rc == 0 and bits(again[0], got[0]) and bits(again[1], got[1]), name


# ---- speckles -----------------------------------------------------------------------------------------------------------------------------------
def framed_copy(eng, a):
    import torch
    f = Framed(eng, a.shape, a.dtype)
    f.buf[BAND:BAND + f.n] = torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).to(eng.device)
    return f


def run_drop(eng, c, size, /, **change):
    """`im_depth_drop_small` in place on framed copies of the case's maps, with `size` (a device tensor or a host array)."""
    held = size if hasattr(size, "data_ptr") else dev(eng, size)
    maps = [framed_copy(eng, c[k]) for k in ("plane", "w", "score")]
    count = Framed(eng, (1,), np.int64)
    h, w = c["plane"].shape
    a = dict(size=held.data_ptr(), h=h, w=w, min_size=c["min_size"], plane=maps[0].ptr, wmap=maps[1].ptr, score=maps[2].ptr, count=count.ptr)
    a.update(change)
    rc = eng.ctx.lib.im_depth_drop_small(eng.ctx.h, a["size"], a["h"], a["w"], a["min_size"], a["plane"], a["wmap"], a["score"], a["count"], eng.stream_ptr())
    eng.synchronize()
    return rc, maps, count


@pytest.mark.parametrize("name", list(C.speckles()))
def test_speckles_equal_the_restatement_bit_for_bit(eng, name):
    import torch
    c = C.speckles()[name]
    size, plane, w, score, n = C.speckle_oracle(name)
    _, device_size = depth_components(dev(eng, c["plane"]), c["max_diff"], engine=eng)
    assert bits(device_size.cpu().numpy(), size), name
    for sizes in (device_size, size):                                             # the device's own sizes, then uploaded ones
        rc, maps, count = run_drop(eng, c, sizes)
        got = [m.result(name) for m in maps]
        assert rc == 0 and bits(got[0], plane) and bits(got[1], w) and bits(got[2], score) and int(count.result(name)[0]) == n, name
    from icepy4d_amd import dense as D
    m = D.DepthMap(dev(eng, c["plane"]), dev(eng, c["w"]), dev(eng, c["score"]), None, None, np.eye(3), np.eye(3), np.zeros(3), (C.W_FIRST, C.W_STEP, 12))
    out, cnt = remove_speckles(m, c["min_size"], c["max_diff"], engine=eng, return_counts=True)
    assert bits(out.plane.cpu().numpy(), plane) and bits(out.w.cpu().numpy(), w) and bits(out.score.cpu().numpy(), score) and int(cnt.item()) == n
    assert bits(m.plane.cpu().numpy(), c["plane"]) and bits(m.w.cpu().numpy(), c["w"]) and cnt.dtype == torch.int64     # the input is as it was


# ---- holes --------------------------------------------------------------------------------------------------------------------------------------
def run_fill(eng, c, maps, label, size, /, outs=None, **change):
    h, w = maps[0].shape
    held = [m if hasattr(m, "data_ptr") else dev(eng, m) for m in (*maps, label, size)]
    outs = outs or (Framed(eng, (h, w), np.int16), Framed(eng, (h, w), np.float64), Framed(eng, (h, w), np.float32), Framed(eng, (h, w), np.uint8),
                    Framed(eng, (1,), np.int64))
    a = dict(plane=held[0].data_ptr(), wmap=held[1].data_ptr(), score=held[2].data_ptr(), label=held[3].data_ptr(), size=held[4].data_ptr(), h=h, w=w,
             max_hole=c["max_hole"], max_diff=c["max_diff"], w_first=float(c["w_first"]), w_step=float(c["w_step"]), D=c["D"], plane_out=outs[0].ptr,
             w_out=outs[1].ptr, score_out=outs[2].ptr, filled=outs[3].ptr, count=outs[4].ptr)
    a.update(change)
    for k, v in list(a.items()):
        if isinstance(v, str):                                                    # "=plane": the pointer of another argument
            a[k] = a[v[1:]]
    rc = eng.ctx.lib.im_depth_fill_holes(eng.ctx.h, a["plane"], a["wmap"], a["score"], a["label"], a["size"], a["h"], a["w"], a["max_hole"], a["max_diff"],
                                         a["w_first"], a["w_step"], a["D"], a["plane_out"], a["w_out"], a["score_out"], a["filled"], a["count"], eng.stream_ptr())
    eng.synchronize()
    return rc, outs


@pytest.mark.parametrize("name", list(C.holes()))
def test_holes_equal_the_restatement_bit_for_bit(eng, name):
    c = C.holes()[name]
    src = C.hole_input(name)
    label, size, plane, w, score, filled, n = C.hole_oracle(name)
    from icepy4d_amd import dense as D
    m = D.DepthMap(dev(eng, c["plane"]), dev(eng, c["w"]), dev(eng, c["score"]), None, None, np.eye(3), np.eye(3), np.zeros(3), (c["w_first"], c["w_step"], c["D"]))
    if c["speckle"] is not None:
        m = remove_speckles(m, *c["speckle"], engine=eng)
        assert bits(m.plane.cpu().numpy(), src[0]) and bits(m.w.cpu().numpy(), src[1]) and bits(m.score.cpu().numpy(), src[2])
    device_label, device_size = depth_components(m.plane, 0, holes=True, engine=eng)
    assert bits(device_label.cpu().numpy(), label) and bits(device_size.cpu().numpy(), size), name
    for lab, siz in ((device_label, device_size), (label, size)):                 # the device's own labels, then uploaded ones
        rc, outs = run_fill(eng, c, src, lab, siz)
        got = [o.result(name) for o in outs]
        assert rc == 0 and bits(got[0], plane) and bits(got[1], w) and bits(got[2], score) and bits(got[3], filled) and int(got[4][0]) == n, \
            (name, [int((g != x).sum()) for g, x in zip(got[:4], (plane, w, score, filled))], int(got[4][0]), n)
    out, cnt = fill_holes(m, c["max_hole"], c["max_diff"], engine=eng, return_counts=True)
    assert bits(out.plane.cpu().numpy(), plane) and bits(out.w.cpu().numpy(), w) and bits(out.score.cpu().numpy(), score) and int(cnt.item()) == n
    assert bits(m.plane.cpu().numpy(), src[0]) and bits(m.w.cpu().numpy(), src[1])


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regularisation", [None, "sgm"], ids=["plain", "sgm"])
def test_python_layer_equals_the_restatements_chain(eng, regularisation):
    from icepy4d_amd import dense as D
    import test_gpu_dense as TD
    import test_gpu_sgm as TS
    images, cams, rng = TD.python_pair(False)
    base = TD.restated_maps(images, cams, rng, 1, 2, 0.9) if regularisation is None else TS.restated_maps(images, cams, rng, 1, 2, 0.9)
    extra = {} if regularisation is None else dict(regularisation="sgm")
    speckle, holes = (12, 0), (32, 2)                          # at min_score 0.9 both steps act on both views
    today = D.build_depth_maps(images, cams, depth_range=rng, radius=2, min_score=0.9, engine=eng, **extra)
    maps = D.build_depth_maps(images, cams, depth_range=rng, radius=2, min_score=0.9, engine=eng, speckle=speckle, holes=holes, **extra)
    none = D.build_depth_maps(images, cams, depth_range=rng, radius=2, min_score=0.9, engine=eng, speckle=None, holes=None, **extra)
    want = []
    for v in (0, 1):
        assert all(bits(getattr(today[v], f).cpu().numpy(), b) for f, b in zip(("plane", "w", "score"), base[v]["out"])), v       # as before this option
        assert all(bits(getattr(none[v], f).cpu().numpy(), b) for f, b in zip(("plane", "w", "score"), base[v]["out"])), v
        out = DO.clean(*base[v]["out"], maps[v].schedule, speckle, holes)
        got = (maps[v].plane.cpu().numpy(), maps[v].w.cpu().numpy(), maps[v].score.cpu().numpy())
        assert all(bits(g, w) for g, w in zip(got, out)), (v, regularisation)
        before, between = base[v]["out"][0], DO.clean(*base[v]["out"], maps[v].schedule, speckle, None)[0]
        assert ((between < 0) & (before >= 0)).sum() > 5 and ((out[0] >= 0) & (between < 0)).sum() > 100, v           # both steps decide something
        want.append(dict(base[v], out=out))
    for v in (0, 1):
        pcd = D.build_dense_cloud(images, cams, depth_filter="MildFiltering", views=(v,), depth_range=rng, radius=2, min_score=0.9, engine=eng,
                                  speckle=speckle, holes=holes, **extra)
        xyz, col, nrm, conf = TD.restated_cloud(want, v, "MildFiltering")
        assert len(xyz) > 100
        assert bits(pcd.points, xyz) and bits(pcd.colors, col.astype(np.float64) / 255.0) and bits(pcd.normals, nrm) and bits(pcd.confidence, conf)
        plain = D.build_dense_cloud(images, cams, depth_filter="MildFiltering", views=(v,), depth_range=rng, radius=2, min_score=0.9, engine=eng, **extra)
        xyz0, col0, nrm0, conf0 = TD.restated_cloud(base, v, "MildFiltering")
        assert bits(plain.points, xyz0) and bits(plain.normals, nrm0) and bits(plain.confidence, conf0)


@pytest.mark.parametrize("seed", list(SC.NOISY))
def test_the_noisy_scenes_on_the_device_reproduce_the_restatement_and_its_shares(eng, seed):
    from icepy4d_amd import dense as D
    c = SC.noisy(seed)
    wta, _ = SC.noisy_oracle(seed)
    clean, full, filled = C.noisy_chain(seed)
    ref, src = dev(eng, c["ref"]), dev(eng, c["src"])
    maps = D.sweep(ref, src, c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"], c["min_score"], engine=eng)
    assert all(bits(g.cpu().numpy(), w) for g, w in zip(maps, wta))
    m = D.DepthMap(*maps, None, None, np.eye(3), np.eye(3), np.zeros(3), (c["w_first"], c["w_step"], c["D"]))
    a, dropped = remove_speckles(m, *C.SPECKLE, engine=eng, return_counts=True)
    b, n_filled = fill_holes(a, *C.HOLES, engine=eng, return_counts=True)
    got_a, got_b = [t.cpu().numpy() for t in (a.plane, a.w, a.score)], [t.cpu().numpy() for t in (b.plane, b.w, b.score)]
    assert all(bits(g, w) for g, w in zip(got_a, clean)) and all(bits(g, w) for g, w in zip(got_b, full))
    assert int(dropped.item()) == int((wta[0] >= 0).sum() - (clean[0] >= 0).sum()) and int(n_filled.item()) == int(filled.sum())
    (r0, w0), (r1, w1) = C.right_and_wrong(wta[0], c), C.right_and_wrong(got_a[0], c)
    print(seed, "dropped", 1.0 - w1.sum() / w0.sum(), "surviving", r1.sum() / r0.sum())
    assert 1.0 - w1.sum() / w0.sum() >= 0.70 and r1.sum() / r0.sum() >= 0.80
    r = c["r"]
    inner = (got_b[0] >= 0)[r:-r, r:-r] & (got_a[0] < 0)[r:-r, r:-r]
    near = inner & (np.abs((got_b[1][r:-r, r:-r] - c["w_first"]) / c["w_step"] - c["k_true"][r:-r, r:-r]) <= 1.0)
    assert inner.sum() == filled[r:-r, r:-r].sum() and near.sum() >= 0.95 * inner.sum()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
COMPONENT_REFUSALS = [dict(plane=None), dict(label=None), dict(size=None), dict(h=0), dict(h=16385), dict(w=0), dict(w=16385), dict(mode=-1), dict(mode=2),
                      dict(max_diff=-1), dict(max_diff=4096)]
DROP_REFUSALS = [dict(size=None), dict(plane=None), dict(wmap=None), dict(score=None), dict(count=None), dict(h=0), dict(w=16385), dict(min_size=0),
                 dict(min_size=-5)]
FILL_REFUSALS = [dict(plane=None), dict(wmap=None), dict(score=None), dict(label=None), dict(size=None), dict(plane_out=None), dict(w_out=None),
                 dict(score_out=None), dict(filled=None), dict(count=None), dict(h=0), dict(w=16385), dict(max_hole=0), dict(max_hole=4097),
                 dict(max_diff=-1), dict(max_diff=4096), dict(D=0), dict(D=4097), dict(w_step=0.0), dict(w_step=float("nan")), dict(w_step=float("inf")),
                 dict(w_first=float("nan")), dict(w_first=float("-inf")), dict(plane="=plane_out"), dict(wmap="=w_out"), dict(score="=score_out")]


def ids(changes):
    return [",".join(f"{k}={v}" for k, v in c.items()) for c in changes]


@pytest.mark.parametrize("change", COMPONENT_REFUSALS, ids=ids(COMPONENT_REFUSALS))
def test_component_refusals_launch_nothing(eng, change):
    rc, outs = run_components(eng, *C.labellings()["shape_17x65_mode0"], **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)


@pytest.mark.parametrize("change", DROP_REFUSALS, ids=ids(DROP_REFUSALS))
def test_drop_refusals_launch_nothing(eng, change):
    name = "random_65x130"
    c = C.speckles()[name]
    rc, maps, count = run_drop(eng, c, C.speckle_oracle(name)[0], **change)
    assert rc == -83
    count.untouched(change)
    assert all(bits(m.result(name), c[k]) for m, k in zip(maps, ("plane", "w", "score")))


@pytest.mark.parametrize("change", FILL_REFUSALS, ids=ids(FILL_REFUSALS))
def test_fill_refusals_launch_nothing(eng, change):
    name = "random_65x130"
    label, size = C.hole_oracle(name)[:2]
    rc, outs = run_fill(eng, C.holes()[name], C.hole_input(name), label, size, **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)
