"""Two-view dense stereo on the device: the three entry points of csrc/dense.hip on every case of tests/dense_cases.py against the numpy
restatement (tests/dense_oracle.py) bit for bit, every output between two bands of sentinel bytes and pre-filled; `build_depth_maps` and
`build_dense_cloud` against the restatement; repeatability; the -83 refusals; one pass of a dense cloud through the Poisson stage."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_cases as DC  # noqa: E402
import dense_oracle as O  # noqa: E402

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

    def result(self, what, rows=None):
        """The output; with `rows`, its first rows, the rest of which must be untouched."""
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        out = host[BAND:BAND + self.n].view(self.dtype).reshape(self.shape)
        if rows is None:
            return out
        assert (out[rows:].view(np.uint8) == FILL).all(), (what, "a row beyond the count was written")
        return out[:rows]

    def untouched(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all() and (host[BAND:BAND + self.n] == FILL).all(), what


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_sweep(eng, c, outs=None, **change):
    a = dict(ref=dev(eng, c["ref"]), src=dev(eng, c["src"]), h0=c["ref"].shape[0], w0=c["ref"].shape[1], h1=c["src"].shape[0], w1=c["src"].shape[1],
             A=np.ascontiguousarray(c["A"], np.float64), B=np.ascontiguousarray(c["B"], np.float64), w_first=float(c["w_first"]), w_step=float(c["w_step"]),
             D=c["D"], r=c["r"], min_var=c["min_var"], min_score=float(c["min_score"]))
    shape = c["ref"].shape
    outs = outs or (Framed(eng, shape, np.int16), Framed(eng, shape, np.float64), Framed(eng, shape, np.float32))
    a.update(plane=outs[0].ptr, w=outs[1].ptr, score=outs[2].ptr)
    a.update(change)
    p = lambda v: v.data_ptr() if hasattr(v, "data_ptr") else (v.ctypes.data if isinstance(v, np.ndarray) else v)  # noqa: E731
    rc = eng.ctx.lib.im_dense_sweep(eng.ctx.h, p(a["ref"]), a["h0"], a["w0"], p(a["src"]), a["h1"], a["w1"], p(a["A"]), p(a["B"]), a["w_first"], a["w_step"],
                                    a["D"], a["r"], a["min_var"], a["min_score"], a["plane"], a["w"], a["score"], eng.stream_ptr())
    eng.synchronize()
    return rc, outs


@pytest.mark.parametrize("name", list(DC.sweeps()))
def test_sweep_equals_the_restatement_bit_for_bit(eng, name):
    rc, outs = run_sweep(eng, DC.sweeps()[name])
    assert rc == 0
    plane, w, score = DC.sweep_oracle(name)
    got = [o.result(name) for o in outs]
    assert bits(got[0], plane), (name, int((got[0] != plane).sum()))
    assert bits(got[1], w) and bits(got[2], score), (name, int((got[1] != w).sum()), int((got[2] != score).sum()))


def run_consistency(eng, pname, flt, keep=None, **change):
    c0, c1, m0, m1 = DC.two_maps(pname)
    tau = O.filter_tau(flt)
    pose = np.ascontiguousarray(DC.pose(c0))
    held = [dev(eng, x) for x in (m0[0], m0[1], m1[0], m1[1])]                  # alive until the call has run
    a = dict(p0=held[0].data_ptr(), w0m=held[1].data_ptr(), h0=m0[0].shape[0], w0=m0[0].shape[1],
             p1=held[2].data_ptr(), w1m=held[3].data_ptr(), h1=m1[0].shape[0], w1=m1[0].shape[1], pose=pose.ctypes.data,
             tol=0.0 if tau is None else tau * abs(c1["w_step"]), check=int(tau is not None))
    keep = keep or Framed(eng, m0[0].shape, np.uint8)
    a.update(out=keep.ptr)
    a.update(change)
    rc = eng.ctx.lib.im_dense_consistency(eng.ctx.h, a["p0"], a["w0m"], a["h0"], a["w0"], a["p1"], a["w1m"], a["h1"], a["w1"], a["pose"], a["tol"], a["check"],
                                          a["out"], eng.stream_ptr())
    eng.synchronize()
    return rc, keep


@pytest.mark.parametrize("pname,flt", DC.CONSISTENCY)
def test_consistency_equals_the_restatement(eng, pname, flt):
    rc, keep = run_consistency(eng, pname, flt)
    assert rc == 0 and bits(keep.result((pname, flt)), DC.consistency_oracle(pname, flt))


def test_no_filtering_needs_no_second_map(eng):
    rc, keep = run_consistency(eng, "padded", "NoFiltering", p1=None, w1m=None, pose=None)
    assert rc == 0 and bits(keep.result("no second map"), DC.consistency_oracle("padded", "NoFiltering"))


def run_cloud(eng, name, outs=None, capacity=None, **change):
    case, want = DC.cloud_case(name)
    n, cap = len(want[0]), (case["h"] * case["w_"] if capacity is None else capacity)
    rows = max(cap, 1)
    outs = outs or (Framed(eng, (rows, 3), np.float64), Framed(eng, (rows, 3), np.uint8), Framed(eng, (rows, 3), np.float64), Framed(eng, (rows,), np.float32),
                    Framed(eng, (1,), np.int64))
    cam = np.ascontiguousarray(case["cam"])
    held = [dev(eng, case[k]) for k in ("keep", "w", "score", "img")]           # alive until the call has run
    a = dict(keep=held[0].data_ptr(), w=held[1].data_ptr(), score=held[2].data_ptr(),
             img=held[3].data_ptr(), channels=case["channels"], h=case["h"], w_=case["w_"], cam=cam.ctypes.data, cap=cap)
    a.update(change)
    rc = eng.ctx.lib.im_dense_cloud(eng.ctx.h, a["keep"], a["w"], a["score"], a["img"], a["channels"], a["h"], a["w_"], a["cam"], a["cap"],
                                    outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr, eng.stream_ptr())
    eng.synchronize()
    return rc, outs, want, n


@pytest.mark.parametrize("name", list(DC.CLOUDS))
def test_cloud_equals_the_restatement_and_leaves_the_rows_beyond_the_count(eng, name):
    rc, outs, want, n = run_cloud(eng, name)
    assert rc == 0 and outs[4].result(name)[0] == n
    for o, w in zip(outs[:4], want):
        assert bits(o.result(name, rows=n), w), name


def test_a_capacity_below_the_count_truncates_and_still_counts(eng):
    rc, outs, want, n = run_cloud(eng, "count_257", capacity=100)
    assert rc == 0 and outs[4].result("count")[0] == n == 257
    for o, w in zip(outs[:4], want):
        assert bits(o.result("truncated"), w[:100])


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------------
def python_pair(rgb):
    """A 97 x 70 pair for `build_depth_maps`: (images, cameras, depth_range), images grey or RGB (three textures stacked)."""
    from icepy4d_amd.core.camera import Camera
    h, w, f = 70, 97, 240.0
    K0 = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    K1 = np.array([[f, 0.0, w / 2.0 + 16.0], [0.0, f, h / 2.0 + 2.0], [0.0, 0.0, 1.0]])
    R0, t0 = DC.R_WORLD, DC.T_WORLD
    R = np.eye(3)
    t = np.array([-1.0, 0.0, 0.0])
    A, B = O.sweep_matrices(K0, K1, R, t)
    uu, vv = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    wmap = (16.0 + 0.03 * (uu - w / 2.0) + 0.04 * (vv - h / 2.0)) / f                      # disparities around 16 px, slanted
    chans0, chans1 = [], []
    for ch in range(3 if rgb else 1):
        src = DC.texture(90 + ch, h + 4, w + 32)
        chans1.append(src)
        chans0.append(DC.render(src, A, B, wmap))
    im0, im1 = (np.stack(c, -1) if rgb else c[0] for c in (chans0, chans1))
    cams = [Camera(w, h, K=K0, R=R0, t=t0), Camera(w + 32, h + 4, K=K1, R=R @ R0, t=R @ t0 + t)]
    return [im0, im1], cams, (f / 22.0, f / 10.0)


def restated_maps(images, cams, depth_range, downscale, radius, min_score):
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
        w_first, w_step, n = D.plane_schedule(cv, co, *depth_range, 1.0, shape=grey[v].shape)   # the schedule is host arithmetic, pinned in test_dense_cpu.py
        R, t = O.relative_pose(*poses[v], *poses[o])
        A, B = O.sweep_matrices(Ks[v], Ks[o], R, t)
        maps.append(dict(out=O.sweep(grey[v], grey[o], A, B, w_first, w_step, n, radius, 4, min_score), K=Ks[v], R=poses[v][0], t=poses[v][1],
                         w_step=w_step, image=small[v]))
    return maps


def restated_cloud(maps, v, depth_filter):
    m, other = maps[v], maps[1 - v]
    R, t = O.relative_pose(m["R"], m["t"], other["R"], other["t"])
    tau = O.filter_tau(depth_filter)
    pose = np.concatenate([O.W.inv3(m["K"]).reshape(9), R.reshape(9), t, other["K"].reshape(9)])
    keep = O.consistency(m["out"][0], m["out"][1], other["out"][0], other["out"][1], pose, 0.0 if tau is None else tau * abs(other["w_step"]), tau is not None)
    cam = np.concatenate([O.W.inv3(m["K"]).reshape(9), m["R"].reshape(9), m["t"]])
    return O.cloud(keep, m["out"][1], m["out"][2], m["image"], cam)


@pytest.mark.parametrize("downscale", [1, 2])
@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_python_layer_equals_the_restatement(eng, downscale, rgb):
    from icepy4d_amd import dense as D
    images, cams, rng = python_pair(rgb)
    want = restated_maps(images, cams, rng, downscale, 2, 0.6)
    maps = D.build_depth_maps(images, cams, depth_range=rng, downscale=downscale, radius=2, min_score=0.6, engine=eng)
    for v in (0, 1):
        got = (maps[v].plane.cpu().numpy(), maps[v].w.cpu().numpy(), maps[v].score.cpu().numpy())
        assert all(bits(g, w) for g, w in zip(got, want[v]["out"])), (v, downscale, rgb)
        assert (got[0] >= 0).mean() > 0.3
    twice = D.build_depth_maps(images, cams, depth_range=rng, downscale=downscale, radius=2, min_score=0.6, engine=eng)
    assert all(bits(getattr(maps[v], f).cpu().numpy(), getattr(twice[v], f).cpu().numpy()) for v in (0, 1) for f in ("plane", "w", "score"))
    clouds = {}
    for views in ((0,), (1,), (0, 1)):
        pcd = D.build_dense_cloud(images, cams, depth_filter="MildFiltering", downscale=downscale, views=views, depth_range=rng, radius=2, min_score=0.6,
                                  engine=eng)
        clouds[views] = (pcd.points, pcd.colors, pcd.normals, pcd.confidence)
    for v in (0, 1):
        xyz, col, nrm, conf = restated_cloud(want, v, "MildFiltering")
        assert len(xyz) > 100
        got = clouds[(v,)]
        assert bits(got[0], xyz) and bits(got[1], col.astype(np.float64) / 255.0) and bits(got[2], nrm) and bits(got[3], conf)
    assert all(bits(clouds[(0, 1)][i], np.concatenate([clouds[(0,)][i], clouds[(1,)][i]])) for i in range(4))


def test_a_dense_cloud_is_written_and_read_back(eng, tmp_path):
    from icepy4d_amd import dense as D
    from icepy4d_amd.core.point_cloud import PointCloud
    images, cams, rng = python_pair(True)
    out = D.dense_series([images], cams, out_dir=tmp_path, dates=["2022_05_01"], depth_range=rng, radius=2, min_score=0.6, engine=eng)
    back = PointCloud(pcd_path=str(tmp_path / "dense_2022_05_01.ply"))
    assert len(out) == 1 and len(back) == len(out[0]) > 100 and bits(back.points, out[0].points) and bits(back.normals, out[0].normals)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
SWEEP_REFUSALS = [dict(ref=None), dict(src=None), dict(A=None), dict(B=None), dict(plane=None), dict(w=None), dict(score=None),
                  dict(h0=0), dict(w0=16385), dict(h1=0), dict(w1=16385), dict(D=0), dict(D=4097), dict(r=0), dict(r=8), dict(min_var=-1)]


@pytest.mark.parametrize("change", SWEEP_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in SWEEP_REFUSALS])
def test_sweep_refusals_launch_nothing(eng, change):
    rc, outs = run_sweep(eng, DC.sweeps()["shape_17x65"], **change)
    assert rc == -83
    for o in outs:
        o.untouched(change)


def test_consistency_and_cloud_refusals_launch_nothing(eng):
    for change in (dict(p0=None), dict(w0m=None), dict(out=None), dict(p1=None), dict(w1m=None), dict(pose=None), dict(h0=0), dict(w0=16385), dict(h1=0),
                   dict(w1=16385), dict(tol=-1.0), dict(tol=float("nan")), dict(check=2)):
        keep = Framed(eng, DC.two_maps("padded")[2][0].shape, np.uint8)
        rc, _ = run_consistency(eng, "padded", "MildFiltering", keep=keep, **change)
        assert rc == -83, change
        keep.untouched(change)
    for change in (dict(keep=None), dict(w=None), dict(score=None), dict(img=None), dict(cam=None), dict(channels=2), dict(h=0), dict(w_=16385), dict(cap=-1)):
        rc, outs, _, _ = run_cloud(eng, "count_255", **change)
        assert rc == -83, change
        for o in outs:
            o.untouched(change)
    nan_cam = np.full(21, np.nan)
    rc, outs, _, _ = run_cloud(eng, "count_255", cam=nan_cam.ctypes.data)
    assert rc == -83
    for o in outs:
        o.untouched("a camera that is not finite")


# ---- downstream -------------------------------------------------------------------------------------------------------------------------------
def test_the_slanted_cloud_goes_through_the_poisson_stage(eng):
    from icepy4d_amd import dense as D
    from icepy4d_amd.post_processing.poisson import poisson_reconstruct
    images, cams, rng = python_pair(False)
    pcd = D.build_dense_cloud(images, cams, depth_filter="ModerateFiltering", depth_range=rng, radius=2, min_score=0.6, engine=eng)
    has = np.linalg.norm(pcd.normals, axis=1) > 0                      # the Poisson stage refuses a zero normal: a pixel without kept neighbours
    assert len(pcd) > 1000 and has.mean() > 0.9
    vertices, triangles, densities = poisson_reconstruct(pcd.points[has], pcd.normals[has], depth=5, engine=eng)
    assert len(vertices) > 0 and len(triangles) > 0 and len(densities) == len(vertices) and np.isfinite(vertices).all()
