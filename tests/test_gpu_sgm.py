"""Semi-global regularisation of dense-stereo depth maps on the device: the three entry points of csrc/dense_sgm.hip on every case of
tests/sgm_cases.py against the numpy restatement (tests/sgm_oracle.py) bit for bit, every output between two bands of sentinel bytes and
pre-filled; the aggregation on uploaded volumes, so that a cost bug cannot mask a path bug, and run twice; `build_depth_maps` and
`build_dense_cloud` with `regularisation="sgm"` against the restatement's chain; a noisy scene whose gain holds on the device; the -83
refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_oracle as O  # noqa: E402
import sgm_cases as SC  # noqa: E402
import sgm_oracle as S  # noqa: E402

from icepy4d_amd.dense import cost_volume, sgm_aggregate, sgm_choose  # noqa: E402,F401  (the feature under test: without it nothing here can pass)

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 512, 0xA5, 0x5C


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def dev(eng, a):
    import torch
    a = np.array(a, order="C")
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a).to(eng.device)


class Framed:
    """An output of `shape` and `dtype` between two bands of sentinel bytes, in one device allocation, pre-filled."""

    def __init__(self, eng, shape, dtype):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        host = np.full(2 * BAND + self.n, SENT, np.uint8)
        host[BAND:BAND + self.n] = FILL
        self.buf = torch.from_numpy(host).to(eng.device)
        self.ptr = self.buf.data_ptr() + BAND

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        return host[BAND:BAND + self.n].view(self.dtype).reshape(self.shape)

    def untouched(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all() and (host[BAND:BAND + self.n] == FILL).all(), what


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def p(v):
    return v.data_ptr() if hasattr(v, "data_ptr") else (v.ctypes.data if isinstance(v, np.ndarray) else v)


# ---- costs --------------------------------------------------------------------------------------------------------------------------------------
def run_costs(eng, c, out=None, **change):
    a = dict(ref=dev(eng, c["ref"]), src=dev(eng, c["src"]), h0=c["ref"].shape[0], w0=c["ref"].shape[1], h1=c["src"].shape[0], w1=c["src"].shape[1],
             A=np.ascontiguousarray(c["A"], np.float64), B=np.ascontiguousarray(c["B"], np.float64), w_first=float(c["w_first"]), w_step=float(c["w_step"]),
             D=c["D"], r=c["r"], min_var=c["min_var"])
    out = out or Framed(eng, (*c["ref"].shape, c["D"]), np.uint8)
    a.update(cost=out.ptr)
    a.update(change)
    rc = eng.ctx.lib.im_dense_costs(eng.ctx.h, p(a["ref"]), a["h0"], a["w0"], p(a["src"]), a["h1"], a["w1"], p(a["A"]), p(a["B"]), a["w_first"], a["w_step"],
                                    a["D"], a["r"], a["min_var"], a["cost"], eng.stream_ptr())
    eng.synchronize()
    return rc, out


@pytest.mark.parametrize("name", list(SC.costs()))
def test_costs_equal_the_restatement_bit_for_bit(eng, name):
    rc, out = run_costs(eng, SC.costs()[name])
    assert rc == 0
    got, want = out.result(name), SC.cost_oracle(name)
    assert bits(got, want), (name, int((got != want).sum()))


def test_costs_at_an_address_that_is_no_multiple_of_four(eng):
    """D = 64 takes whole words where the volume is aligned; one byte further it takes the byte path."""
    c = SC.costs()["planes_64"]
    wide = Framed(eng, (c["ref"].size * c["D"] + 4,), np.uint8)
    rc, _ = run_costs(eng, c, out=wide, cost=wide.ptr + 1)
    assert rc == 0
    got = wide.result("shifted")
    assert got[0] == FILL and (got[-3:] == FILL).all() and bits(got[1:-3].reshape(SC.cost_oracle("planes_64").shape), SC.cost_oracle("planes_64"))


# ---- aggregation --------------------------------------------------------------------------------------------------------------------------------
def run_sgm(eng, volume, P1, P2, paths, /, out=None, **change):
    held = dev(eng, volume)
    a = dict(cost=held.data_ptr(), h0=volume.shape[0], w0=volume.shape[1], D=volume.shape[2], P1=P1, P2=P2, paths=paths)
    out = out or Framed(eng, volume.shape, np.uint16)
    a.update(sum=out.ptr)
    a.update(change)
    rc = eng.ctx.lib.im_dense_sgm(eng.ctx.h, a["cost"], a["h0"], a["w0"], a["D"], a["P1"], a["P2"], a["paths"], a["sum"], eng.stream_ptr())
    eng.synchronize()
    return rc, out


@pytest.mark.parametrize("name", list(SC.aggregations()))
def test_aggregation_equals_the_restatement_and_repeats(eng, name):
    cost, P1, P2, paths = SC.aggregations()[name]
    want = SC.aggregate_oracle(name)
    rc, out = run_sgm(eng, cost, P1, P2, paths)
    got = out.result(name)
    assert rc == 0 and bits(got, want), (name, int((got != want).sum()))
    rc, out = run_sgm(eng, cost, P1, P2, paths, out=out)                         # over its own result: the first walk stores, it does not add
    assert rc == 0 and bits(out.result(name), want), name


# ---- the choice ---------------------------------------------------------------------------------------------------------------------------------
def run_choose(eng, c, outs=None, **change):
    held = [dev(eng, c["cost"]), dev(eng, c["sum"])]
    h0, w0, D = c["cost"].shape
    outs = outs or (Framed(eng, (h0, w0), np.int16), Framed(eng, (h0, w0), np.float64), Framed(eng, (h0, w0), np.float32))
    a = dict(cost=held[0].data_ptr(), sum=held[1].data_ptr(), h0=h0, w0=w0, D=D, w_first=float(c["w_first"]), w_step=float(c["w_step"]),
             min_score=float(c["min_score"]), plane=outs[0].ptr, w=outs[1].ptr, score=outs[2].ptr)
    a.update(change)
    rc = eng.ctx.lib.im_dense_sgm_choose(eng.ctx.h, a["cost"], a["sum"], a["h0"], a["w0"], a["D"], a["w_first"], a["w_step"], a["min_score"], a["plane"], a["w"],
                                         a["score"], eng.stream_ptr())
    eng.synchronize()
    return rc, outs


@pytest.mark.parametrize("name", list(SC.choices()))
def test_choice_equals_the_restatement_bit_for_bit(eng, name):
    rc, outs = run_choose(eng, SC.choices()[name])
    assert rc == 0
    got, want = [o.result(name) for o in outs], SC.choose_oracle(name)
    assert bits(got[0], want[0]), (name, int((got[0] != want[0]).sum()))
    assert bits(got[1], want[1]) and bits(got[2], want[2]), (name, int((got[1] != want[1]).sum()), int((got[2] != want[2]).sum()))


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------
def restated_maps(images, cams, depth_range, downscale, radius, min_score):
    """`test_gpu_dense.restated_maps` with the regularised sweep of the restatement."""
    from icepy4d_amd import dense as D
    small = [O.downscale(im, downscale) for im in images]
    grey = [O.grey(s) for s in small]
    Ks = [O.downscale_K(c.K, downscale) for c in cams]
    poses = [(np.asarray(c.R, np.float64), np.asarray(c.t, np.float64).reshape(3)) for c in cams]
    maps = []
    for v in (0, 1):
        o = 1 - v

        class Cam:
            pass
        cv, co = Cam(), Cam()
        cv.K, cv.R, cv.t = Ks[v], *poses[v]
        co.K, co.R, co.t = Ks[o], *poses[o]
        w_first, w_step, n = D.plane_schedule(cv, co, *depth_range, 1.0, shape=grey[v].shape)
        R, t = O.relative_pose(*poses[v], *poses[o])
        A, B = O.sweep_matrices(Ks[v], Ks[o], R, t)
        maps.append(dict(out=S.sweep(grey[v], grey[o], A, B, w_first, w_step, n, radius, 4, min_score, SC.P1, SC.P2, SC.PATHS), K=Ks[v], R=poses[v][0],
                         t=poses[v][1], w_step=w_step, image=small[v]))
    return maps


@pytest.mark.parametrize("downscale", [1, 2])
@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_python_layer_equals_the_restatement(eng, downscale, rgb):
    from icepy4d_amd import dense as D
    from test_gpu_dense import python_pair, restated_cloud
    images, cams, rng = python_pair(rgb)
    want = restated_maps(images, cams, rng, downscale, 2, 0.6)
    maps = D.build_depth_maps(images, cams, depth_range=rng, downscale=downscale, radius=2, min_score=0.6, engine=eng, regularisation="sgm")
    for v in (0, 1):
        got = (maps[v].plane.cpu().numpy(), maps[v].w.cpu().numpy(), maps[v].score.cpu().numpy())
        assert all(bits(g, w) for g, w in zip(got, want[v]["out"])), (v, downscale, rgb)
        assert (got[0] >= 0).mean() > 0.3
    plain = D.build_depth_maps(images, cams, depth_range=rng, downscale=downscale, radius=2, min_score=0.6, engine=eng)
    assert not bits(plain[0].w.cpu().numpy(), want[0]["out"][1])                 # the option decides something
    for v in (0, 1):
        pcd = D.build_dense_cloud(images, cams, depth_filter="MildFiltering", downscale=downscale, views=(v,), depth_range=rng, radius=2, min_score=0.6,
                                  engine=eng, regularisation="sgm")
        xyz, col, nrm, conf = restated_cloud(want, v, "MildFiltering")
        assert len(xyz) > 100
        assert bits(pcd.points, xyz) and bits(pcd.colors, col.astype(np.float64) / 255.0) and bits(pcd.normals, nrm) and bits(pcd.confidence, conf)


def test_a_noisy_scene_on_the_device_reproduces_the_restatement_and_its_gain(eng):
    from icepy4d_amd import dense as D
    seed = 202
    c = SC.noisy(seed)
    wta, sgm = SC.noisy_oracle(seed)
    ref, src = dev(eng, c["ref"]), dev(eng, c["src"])
    a = (ref, src, c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"], c["min_score"])
    got = [t.cpu().numpy() for t in D.sweep(*a, engine=eng, regularisation="sgm", p1=SC.P1, p2=SC.P2, paths=SC.PATHS)]
    assert all(bits(g, w) for g, w in zip(got, sgm))
    plain = [t.cpu().numpy() for t in D.sweep(*a, engine=eng)]
    assert all(bits(g, w) for g, w in zip(plain, wta))
    gain = SC.share_within_one_plane(got[0], c) - SC.share_within_one_plane(plain[0], c)
    print("gain on the device:", gain)
    assert gain >= 0.25 and (got[0][c["r"]:-c["r"], c["r"]:-c["r"]] >= 0).all()
    cost = D.cost_volume(ref, src, *a[2:9], engine=eng)
    total = D.sgm_aggregate(cost, SC.P1, SC.P2, SC.PATHS, engine=eng)
    want_cost = SC.volume_of(c)
    assert bits(cost.cpu().numpy(), want_cost) and bits(total.cpu().numpy(), S.aggregate(want_cost, SC.P1, SC.P2, SC.PATHS))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
COST_REFUSALS = [dict(ref=None), dict(src=None), dict(A=None), dict(B=None), dict(cost=None), dict(h0=0), dict(w0=16385), dict(h1=0), dict(w1=16385),
                 dict(D=0), dict(D=257), dict(r=0), dict(r=8), dict(min_var=-1), dict(min_var=(1 << 26) + 1), dict(h0=16384, w0=16384, D=17)]
SGM_REFUSALS = [dict(cost=None), dict(sum=None), dict(h0=0), dict(w0=16385), dict(D=0), dict(D=257), dict(P1=-1), dict(P1=129), dict(P2=4096, P1=0),
                dict(paths=0), dict(paths=6), dict(paths=16), dict(h0=16384, w0=16384, D=17)]
CHOOSE_REFUSALS = [dict(cost=None), dict(sum=None), dict(plane=None), dict(w=None), dict(score=None), dict(h0=0), dict(w0=16385), dict(D=0), dict(D=257),
                   dict(h0=16384, w0=16384, D=17)]


def ids(changes):
    return [",".join(f"{k}={v}" for k, v in c.items()) for c in changes]


@pytest.mark.parametrize("change", COST_REFUSALS, ids=ids(COST_REFUSALS))
def test_cost_refusals_launch_nothing(eng, change):
    rc, out = run_costs(eng, SC.costs()["shape_17x65"], **change)
    assert rc == -83
    out.untouched(change)


@pytest.mark.parametrize("change", SGM_REFUSALS, ids=ids(SGM_REFUSALS))
def test_aggregation_refusals_launch_nothing(eng, change):
    rc, out = run_sgm(eng, SC.random_volume(17, 65, 5), 16, 128, 8, **change)
    assert rc == -83
    out.untouched(change)


@pytest.mark.parametrize("change", CHOOSE_REFUSALS, ids=ids(CHOOSE_REFUSALS))
def test_choice_refusals_launch_nothing(eng, change):
    rc, outs = run_choose(eng, SC.choices()["invalid_neighbour"], **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)
