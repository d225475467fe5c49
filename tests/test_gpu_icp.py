"""The ICP kernels (csrc/icp.hip: im_transform_points, im_icp_accumulate, im_icp_finish) on the device on the shared cases
(tests/icp_cases.py: source sizes around the wave, the block and the chunk, a finish thread with a second chunk, missing and
out-of-range correspondences, non-finite points and normals, flipped normals, a world frame, a far centre, planted singular and
near-singular systems), the Python layers at any cell size and query order, the end-to-end case, the statuses and the refusals.

Bounds. Every output of the three entry points and every record of `registration_icp` and `evaluate_registration` (`history`): equality
of bits with the restatement (tests/icp_oracle.py), a NaN equal to a NaN whatever its payload. Derived, not measured: the
correspondences are those of im_knn_cross, pinned to its own restatement; every sum runs in an order fixed by the source index alone
(chunks, threads, butterfly, waves: csrc/icp_point.h) over the same IEEE float64 operations with contraction off, and float64 division
and sqrt are correctly rounded on the device. The host build of the same text agrees with the restatement on the same cases
(tests/test_icp_cpu.py); what only this file can show is the shuffles, the LDS exchange, the launch shapes and a lost
`#pragma clang fp contract(off)`. `transform` against the reference's recorded values (tests/golden/g21_transformations.npz): within
2 gamma_4 sum_j |M_aj| |x_j| per component, as derived in tests/test_icp_cpu.py.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_cases as IC  # noqa: E402
import icp_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -81
U = 2.0 ** -53
GOLDEN = os.path.join(ROOT, "tests", "golden", "g21_transformations.npz")
NAMES = {0: "point_to_point", 1: "point_to_plane"}


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def p(t):
    from icepy4d_amd._lib import ptr
    return ptr(t)


def dev(eng, a):
    """A copy on the device (the shared inputs are read-only); an empty array becomes one zero row, so that its pointer is not null."""
    import torch
    a = np.array(a, order="C")
    if a.shape[0] == 0:
        a = np.zeros((1,) + a.shape[1:], a.dtype)
    return torch.from_numpy(a).to(eng.device)


def same(a, b):
    """Equality of bits, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


class Framed:
    """An output of `shape` x `dtype` between two bands of sentinel bytes, in one device allocation, pre-filled (or holding `init`)."""

    def __init__(self, eng, shape, dtype=np.float64, init=None):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        host = np.full(2 * BAND + self.n, SENT, np.uint8)
        host[BAND:BAND + self.n] = FILL if init is None else np.ascontiguousarray(init, self.dtype).reshape(-1).view(np.uint8)
        self.buf = torch.from_numpy(host).to(eng.device)
        self.ptr = self.buf.data_ptr() + BAND

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        return host[BAND:BAND + self.n].view(self.dtype).reshape(self.shape)

    def untouched(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all() and (host[BAND:BAND + self.n] == FILL).all(), what


class Case:
    """A case's arrays on the device."""

    def __init__(self, eng, name):
        c = IC.by_name(name)
        self.c, self.n, self.nt, self.chunks = c, len(c["source"]), len(c["target"]), O.n_chunks(len(c["source"]))
        self.src, self.tgt, self.nrm = dev(eng, c["source"]), dev(eng, c["target"]), dev(eng, c["normals"])
        self.idx, self.d2, self.M = dev(eng, c["idx"]), dev(eng, c["d2"]), dev(eng, c["M"].reshape(16))
        self.centre = np.ascontiguousarray(c["centre"], np.float64)

    def accumulate_args(self, method, parts_ptr):
        return (p(self.src), self.n, p(self.tgt), p(self.nrm), self.nt, p(self.idx), p(self.d2), self.centre.ctypes.data, method, self.chunks, parts_ptr)


# ---- the C entry points ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2049])
def test_transform_points_equals_the_restatement(eng, n):
    rng = np.random.default_rng(n)
    pts = rng.normal(0, 50.0, (n, 3)) + IC.WORLD
    if n > 200:
        pts[3], pts[4], pts[5, 1] = np.nan, np.inf, -np.inf
    M = IC.motion(7.0, (0.3, 0.2, -0.9), (12.0, -7.0, 3.0), about=IC.WORLD)
    d_M, d_in, st = dev(eng, M.reshape(16)), dev(eng, pts), eng.stream_ptr()
    for as_vectors in (0, 1):
        out = Framed(eng, (n, 3))
        eng.ctx.call("im_transform_points", p(d_M), p(d_in), out.ptr, n, as_vectors, st)
        assert same(out.result("transform"), O.apply(M, pts, bool(as_vectors)) if n else np.zeros((0, 3))), (n, as_vectors)
    inplace = Framed(eng, (n, 3), init=pts)
    eng.ctx.call("im_transform_points", p(d_M), inplace.ptr, inplace.ptr, n, 0, st)
    assert same(inplace.result("in place"), O.apply(M, pts))


@pytest.mark.parametrize("method", IC.METHODS)
@pytest.mark.parametrize("name", IC.names(big=True))
def test_accumulate_and_finish_equal_the_restatement(eng, name, method):
    k, st = Case(eng, name), eng.stream_ptr()
    want_parts, want_S, want_rec, want_eval = IC.expected(name, method)
    parts = Framed(eng, (k.chunks, O.TERMS))
    eng.ctx.call("im_icp_accumulate", *k.accumulate_args(method, parts.ptr if k.chunks else None), st)
    got = parts.result("partials")
    assert same(got, want_parts), name
    for solve, want in ((1, want_rec), (0, want_eval)):
        rec = Framed(eng, (O.RECORD,))
        eng.ctx.call("im_icp_finish", parts.ptr if k.chunks else None, k.n, k.chunks, p(k.M), k.centre.ctypes.data, solve, rec.ptr, st)
        assert same(rec.result("record"), want), (name, solve)
    # the same through the context's scratch, and with the record's own M_next slot as the M read
    eng.ctx.call("im_icp_accumulate", *k.accumulate_args(method, None), st)
    rec = Framed(eng, (O.RECORD,), init=np.concatenate([k.c["M"].reshape(16), np.full(O.RECORD - 16, -7.0)]))
    eng.ctx.call("im_icp_finish", None, k.n, k.chunks, rec.ptr, k.centre.ctypes.data, 1, rec.ptr, st)
    assert same(rec.result("record in place"), want_rec), name


def test_the_chunk_is_the_oracles():
    from icepy4d_amd.post_processing.registration import icp_chunk
    assert icp_chunk() == O.ICP_CHUNK == 1024


# ---- the Python layers: independence from tunables -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def python_case():
    src, tgt, nrm = IC.moved_sample(1500, seed=21, noise=0.01)
    src[::50] += (0.0, 0.0, 4.0)                                        # a few points without a correspondence
    src[7, 1] = np.nan
    return src, tgt, nrm


@functools.lru_cache(maxsize=None)
def python_expected(method, flipped=False):
    src, tgt, nrm = python_case()
    return O.icp(src, tgt, -nrm if flipped else nrm, IC.D_MAX, method=method)


def check_result(r, expected, n):
    M, records, corr, converged = expected
    import torch
    tr = r.transformation.cpu().numpy() if isinstance(r.transformation, torch.Tensor) else r.transformation
    cs = r.correspondence_set.cpu().numpy() if isinstance(r.correspondence_set, torch.Tensor) else r.correspondence_set
    assert same(r.history, records), (r.history.shape, records.shape)
    assert same(tr, M) and r.converged == converged and r.iterations == len(records) - 1
    assert r.fitness == records[-1, O.REC_FITNESS] and r.inlier_rmse == records[-1, O.REC_RMSE]
    assert r.status == ("OK", "EMPTY", "DEGENERATE")[int(records[-1, O.REC_STATUS])]
    idx = corr[-1][0]
    assert np.array_equal(cs, np.stack([np.nonzero(idx >= 0)[0], idx[idx >= 0]], 1))


@pytest.mark.parametrize("method", IC.METHODS)
def test_registration_does_not_depend_on_cell_size_order_or_kind(eng, method):
    import torch
    from icepy4d_amd.post_processing import registration as R
    from icepy4d_amd.utils import point_cloud_filters as F
    src, tgt, nrm = python_case()
    want = python_expected(method)
    assert want[3] and 2 <= len(want[1]) - 1 <= 30 and 0.9 < want[1][-1, O.REC_FITNESS] < 1.0
    kw = dict(estimation_method=NAMES[method], target_normals=nrm, engine=eng)
    for cell in (0.2, 0.5, 3.0):
        tb = F.bin_cloud(tgt, cell, engine=eng)
        for sort_queries in (True, False):
            check_result(R.registration_icp(src, tb, IC.D_MAX, sort_queries=sort_queries, **kw), want, len(src))
    r = R.registration_icp(src, tgt, IC.D_MAX, **kw)                    # numpy in, numpy out; binned here at d_max
    assert isinstance(r.transformation, np.ndarray) and isinstance(r.correspondence_set, np.ndarray)
    check_result(r, want, len(src))
    t = R.registration_icp(torch.from_numpy(src).to(eng.device), torch.from_numpy(tgt).to(eng.device), IC.D_MAX,
                           **{**kw, "target_normals": torch.from_numpy(nrm).to(eng.device)})
    assert isinstance(t.transformation, torch.Tensor) and isinstance(t.correspondence_set, torch.Tensor)
    check_result(t, want, len(src))
    again = R.registration_icp(src, tgt, IC.D_MAX, **kw)                # two runs are identical
    assert same(again.history, r.history) and np.array_equal(again.correspondence_set, r.correspondence_set)
    flipped = R.registration_icp(src, tgt, IC.D_MAX, **{**kw, "target_normals": -nrm})
    assert same(flipped.history, r.history) and same(python_expected(method, True)[1], want[1])
    # the evaluation at the result and at the identity
    for M in (np.eye(4), r.transformation):
        ev = R.evaluate_registration(src, tgt, IC.D_MAX, transformation=M, engine=eng)
        rec, idx, _ = O.evaluate(src, tgt, None, IC.D_MAX, M, O.default_centre(tgt), O.POINT_TO_POINT, False)
        assert same(ev.history, rec[None]) and ev.iterations == 0 and not ev.converged and same(ev.transformation, M)
        assert ev.fitness == rec[O.REC_FITNESS] and ev.inlier_rmse == rec[O.REC_RMSE]
    assert ev.inlier_rmse == r.inlier_rmse and ev.fitness == r.fitness


def test_max_iteration_and_a_centre_of_ones_own(eng):
    from icepy4d_amd.post_processing import registration as R
    src, tgt, nrm = python_case()
    for max_it in (0, 1, 2):
        want = O.icp(src, tgt, nrm, IC.D_MAX, method=1, max_iteration=max_it, centre=(1.0, 2.0, 3.0), init=IC.motion(0.1))
        r = R.registration_icp(src, tgt, IC.D_MAX, init=IC.motion(0.1), target_normals=nrm, centre=(1.0, 2.0, 3.0), engine=eng,
                               criteria=R.ICPConvergenceCriteria(max_iteration=max_it))
        check_result(r, want, len(src))
        assert r.iterations <= max_it and (max_it > 0 or not r.converged)


def test_normals_estimated_at_a_radius(eng):
    from icepy4d_amd.post_processing import registration as R
    from icepy4d_amd.utils import point_cloud_filters as F
    src, tgt, _ = python_case()
    nrm = F.ball_cross(tgt, tgt, 0.6, want=("normal",), engine=eng)["normal"]
    assert np.isfinite(nrm).all(1).sum() > 0.9 * len(tgt)
    r = R.registration_icp(src, tgt, IC.D_MAX, normal_radius=0.6, engine=eng)
    check_result(r, O.icp(src, tgt, nrm, IC.D_MAX, method=1), len(src))


# ---- same-run identities ---------------------------------------------------------------------------------------------------------------------
def test_a_series_equals_its_per_pair_calls(eng):
    import torch
    from icepy4d_amd import change_detection as C
    from icepy4d_amd.post_processing import registration as R
    tgt, _ = IC.surface(30)
    rng = np.random.default_rng(5)
    epochs = [tgt]
    for k in (1, 2):
        Minv = np.linalg.inv(IC.motion(0.2 * k, shift=(0.02 * k, -0.01, 0.03), about=(3.5, 3.5, 0.5)))
        epochs.append(np.ascontiguousarray(tgt @ Minv[:3, :3].T + Minv[:3, 3] + rng.normal(0, 0.005, tgt.shape)))
    stable = np.array([[1.0, 1.0], [6.5, 1.2], [6.0, 6.4], [0.8, 5.9]])
    inside = [e[_in_polygon(e, stable)] for e in epochs]
    assert all(200 < len(i) < len(tgt) for i in inside)
    kw = dict(normal_radius=0.6, estimation_method="point_to_plane")
    for reference in (0, "previous"):
        results, moved = C.coregister_series(epochs, IC.D_MAX, reference=reference, stable=stable, return_clouds=True, engine=eng, **kw)
        assert results[0] is None and len(results) == 3 and torch.equal(moved[0].cpu(), torch.from_numpy(epochs[0]))
        for i in (1, 2):
            ref = 0 if reference == 0 else i - 1
            pair = R.registration_icp(inside[i], inside[ref], IC.D_MAX, engine=eng, **kw)
            assert same(results[i].history, pair.history) and same(results[i].transformation, pair.transformation)
            assert np.array_equal(results[i].correspondence_set, pair.correspondence_set) and pair.converged
            assert same(moved[i].cpu().numpy(), O.apply(pair.transformation, epochs[i]))
        table = C.coregistration_table(results, reference=reference)
        assert table["converged"].all() and (table["inlier_rmse"][1:] <= IC.D_MAX).all()          # a nearest-point distance: below d_max


def _in_polygon(pts, poly):
    """The even-odd rule of im_crop_polygon (include/icematch.h), in numpy."""
    x, y = pts[:, 0], pts[:, 1]
    inside = np.zeros(len(pts), bool)
    for k in range(len(poly)):
        (x0, y0), (x1, y1) = poly[k - 1], poly[k]
        with np.errstate(divide="ignore", invalid="ignore"):
            inside ^= ((y0 > y) != (y1 > y)) & (x < (x1 - x0) * (y - y0) / (y1 - y0) + x0)
    return inside


def test_transforms_against_the_recorded_reference(eng, tmp_path):
    from icepy4d_amd.core.point_cloud import PointCloud
    from icepy4d_amd.utils import transformations as T
    g = np.load(GOLDEN)
    g4 = 4 * U / (1 - 4 * U)
    for frame in ("local", "world"):
        rt = T.Rotrotranslation(np.array(g[f"T_{frame}"]))
        for pn in ("local", "world"):
            x, fwd = np.array(g[f"pts_{pn}"]), np.array(g[f"fwd_{frame}_{pn}"])
            M = rt.T
            bound = 2 * g4 * (np.abs(x) @ np.abs(M[:3, :3]).T + np.abs(M[:3, 3])[None, :])
            got = rt.transform(x, engine=eng)
            assert same(got, O.apply(M, x)) and (np.abs(got - fwd) <= bound).all(), (frame, pn)
            cloud = PointCloud(points3d=x)
            cloud.normals = np.ascontiguousarray(np.roll(x, 1, axis=1))
            moved = cloud.transform(M, engine=eng)
            assert same(moved.points, got) and same(moved.normals, O.apply(M, cloud.normals, True)) and moved.colors is None
            Minv = rt.T_inv
            back = rt.transform_inverse(fwd, engine=eng)
            bound = 2 * g4 * (np.abs(fwd) @ np.abs(Minv[:3, :3]).T + np.abs(Minv[:3, 3])[None, :])
            assert same(back, O.apply(rt._matrix(Minv), fwd)) and (np.abs(back - g[f"inv_{frame}_{pn}"]) <= bound).all(), (frame, pn)
    src = PointCloud(points3d=np.array(g["pts_local"]), points_col=np.full((48, 3), 0.5))
    src.write_ply(tmp_path / "in.ply")
    out = T.Rotrotranslation(np.array(g["T_local"])).transform_pcd(tmp_path / "in.ply", out_path=str(tmp_path / "out.ply"), engine=eng)
    assert same(out.points, O.apply(g["T_local"], g["pts_local"])) and same(PointCloud(pcd_path=str(tmp_path / "out.ply")).points, out.points)
    inv = T.Rotrotranslation(np.array(g["T_local"])).transform_pcd(tmp_path / "out.ply", inverse=True, engine=eng)
    assert np.abs(inv.points - g["pts_local"]).max() < 1e-12


# ---- the end-to-end case -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True])
@pytest.mark.parametrize("method", IC.METHODS)
def test_end_to_end_equals_the_restatement(eng, world, method):
    from icepy4d_amd.post_processing import registration as R
    src, tgt, nrm, _ = IC.end_to_end(world)
    want = IC.end_to_end_expected(world, method)
    r = R.registration_icp(src, tgt, IC.D_MAX, estimation_method=NAMES[method], target_normals=nrm, engine=eng)
    check_result(r, want, len(src))
    assert r.converged and r.fitness == 1.0 and np.array_equal(r.correspondence_set[:, 0], r.correspondence_set[:, 1])
    assert np.abs(O.apply(r.transformation, src) - tgt).max() <= 4 * np.spacing(np.abs(tgt).max())


def test_a_source_equal_to_the_target_stays(eng):
    from icepy4d_amd.post_processing import registration as R
    tgt, nrm = IC.surface(12, offset=IC.WORLD)
    for method in IC.METHODS:
        init = np.eye(4)
        r = R.registration_icp(tgt, tgt, IC.D_MAX, init=init, estimation_method=NAMES[method], target_normals=nrm, engine=eng)
        assert same(r.transformation, init) and r.inlier_rmse == 0.0 and r.fitness == 1.0 and r.converged and r.status == "OK"


# ---- statuses and refusals -----------------------------------------------------------------------------------------------------------------------
def test_statuses(eng):
    from icepy4d_amd.post_processing import registration as R
    src, tgt, nrm = IC.moved_sample(500, seed=11)
    src[::4] += (0.0, 0.0, 3.0)                                         # a partial overlap
    want = O.icp(src, tgt, nrm, IC.D_MAX, method=1)
    r = R.registration_icp(src, tgt, IC.D_MAX, target_normals=nrm, engine=eng)
    check_result(r, want, len(src))
    assert 0.0 < r.fitness <= 0.75 and r.status == "OK"
    flat = IC.by_name("planar")
    init = IC.motion(0.0, shift=(0.0, 0.0, 0.001))
    d = R.registration_icp(flat["source"], flat["target"], IC.D_MAX, init=init, target_normals=flat["normals"], centre=np.zeros(3), engine=eng)
    assert d.status == "DEGENERATE" and same(d.transformation, init) and d.iterations == 0 and not d.converged and d.fitness == 1.0
    check_result(d, O.icp(flat["source"], flat["target"], flat["normals"], IC.D_MAX, init=init, method=1, centre=np.zeros(3)), len(flat["source"]))
    few = R.registration_icp(src[1:6], tgt, IC.D_MAX, target_normals=nrm, engine=eng)
    assert few.status == "DEGENERATE" and few.history[0, O.REC_COUNT] == 4.0 and same(few.transformation, np.eye(4))
    far = R.registration_icp(src + 100.0, tgt, IC.D_MAX, target_normals=nrm, engine=eng)
    assert far.status == "EMPTY" and far.fitness == 0.0 and far.inlier_rmse == 0.0 and len(far.correspondence_set) == 0 and same(far.transformation, np.eye(4))
    for s, t, n in ((np.zeros((0, 3)), tgt, nrm), (src, np.zeros((0, 3)), np.zeros((0, 3)))):
        e = R.registration_icp(s, t, IC.D_MAX, target_normals=n, engine=eng)
        assert e.status == "EMPTY" and e.fitness == 0.0 and e.iterations == 0
        check_result(e, O.icp(s, t, n, IC.D_MAX, method=1), len(s))


def test_refusals_leave_the_outputs_alone(eng):
    from icepy4d_amd._lib import IcematchError
    k, st = Case(eng, "n1025"), eng.stream_ptr()
    n, nt, ch, c = k.n, k.nt, k.chunks, k.centre.ctypes.data
    src, tgt, nrm, idx, d2, M = p(k.src), p(k.tgt), p(k.nrm), p(k.idx), p(k.d2), p(k.M)
    bad_centres = {what: np.array(v, np.float64) for what, v in (("nan", (0.0, np.nan, 0.0)), ("inf", (np.inf, 0.0, 0.0)), ("-inf", (0.0, 0.0, -np.inf)))}
    out, parts, rec = Framed(eng, (n, 3)), Framed(eng, (ch, O.TERMS)), Framed(eng, (O.RECORD,))
    calls = [("im_transform_points", "null M", (None, src, out.ptr, n, 0)), ("im_transform_points", "null in", (M, None, out.ptr, n, 0)),
             ("im_transform_points", "null out", (M, src, None, n, 0)), ("im_transform_points", "n < 0", (M, src, out.ptr, -1, 0)),
             ("im_transform_points", "n = 2^26 + 1", (M, src, out.ptr, 2 ** 26 + 1, 0))]
    acc = lambda **kw: tuple({**dict(src=src, n=n, tgt=tgt, nrm=nrm, nt=nt, idx=idx, d2=d2, c=c, method=1, ch=ch, parts=parts.ptr), **kw}.values())  # noqa: E731
    calls += [("im_icp_accumulate", what, acc(**kw)) for what, kw in (
        ("null source", dict(src=None)), ("null target", dict(tgt=None)), ("null idx", dict(idx=None)), ("null d2", dict(d2=None)),
        ("null centre", dict(c=None)), ("point to plane without normals", dict(nrm=None)), ("n < 0", dict(n=-1, ch=0)),
        ("n = 2^26 + 1", dict(n=2 ** 26 + 1, ch=2 ** 16 + 1)), ("n_tgt < 0", dict(nt=-1)), ("n_tgt = 2^26 + 1", dict(nt=2 ** 26 + 1)),
        ("method 2", dict(method=2)), ("method -1", dict(method=-1)), ("a chunk too few", dict(ch=ch - 1)), ("a chunk too many", dict(ch=ch + 1)),
        ("no chunks", dict(ch=0)))]
    calls += [("im_icp_accumulate", f"centre {what}", acc(c=arr.ctypes.data)) for what, arr in bad_centres.items()]
    fin = lambda **kw: tuple({**dict(parts=parts.ptr, n=n, ch=ch, M=M, c=c, solve=1, rec=rec.ptr), **kw}.values())  # noqa: E731
    calls += [("im_icp_finish", what, fin(**kw)) for what, kw in (
        ("null M", dict(M=None)), ("null record", dict(rec=None)), ("null centre", dict(c=None)), ("n < 0", dict(n=-1, ch=0)),
        ("n = 2^26 + 1", dict(n=2 ** 26 + 1, ch=2 ** 16 + 1)), ("a chunk too few", dict(ch=ch - 1)), ("a chunk too many", dict(ch=ch + 1)),
        ("solve 2", dict(solve=2)), ("solve -1", dict(solve=-1)))]
    calls += [("im_icp_finish", f"centre {what}", fin(c=arr.ctypes.data)) for what, arr in bad_centres.items()]
    for fn, what, args in calls:
        with pytest.raises(IcematchError) as e:
            eng.ctx.call(fn, *args, st)
        assert e.value.rc == REFUSED, (fn, what, e.value)
    for name, f in (("out", out), ("parts", parts), ("record", rec)):
        f.untouched(name)
    # a finish from the context's scratch before any accumulate of as many chunks
    from icepy4d_amd._lib import Context
    fresh = Context(eng.ctx.device)
    with pytest.raises(IcematchError) as e:
        fresh.call("im_icp_finish", None, n, ch, M, c, 1, rec.ptr, st)
    assert e.value.rc == REFUSED
    rec.untouched("record")
    fresh.close()
