"""Voxel grids, voxel down-sampling and voxel box meshes (csrc/voxel.hip, csrc/voxel_cell.h) on the device, on every case of
tests/voxel_cases.py (each size at which a kernel takes another path: see that file), through the C entry points and through `VoxelGrid`,
`voxel_down_sample`, `PointCloud.voxel_down_sample`, `voxel_series` and `voxelize`, a batch against its single-cloud calls, two runs
against each other, the reference script's outputs in tests/golden/g19_voxel.npz, and the refusals.

Bounds. Everything is equality: cloud bounds, keys, dropped counts, `d_nvox`, grid indices, counts, first indices, every mean, vertices,
vertex colours and triangles are bit-identical to the numpy restatement (tests/voxel_oracle.py). Derived, not measured: the kernels and
the restatement perform the same IEEE float64 operations in the same order with contraction off (float64 division is correctly rounded
on the device, the library is built without a fast-math flag), the minima, maxima and integer counts are order-free, and the order of a
voxel's sum is the input order, which the stable sort keeps. A NaN compares equal to a NaN: its sign and payload are not part of the
definition. The host build of the same text agrees with the restatement on the same cases (tests/test_voxel_cpu.py); what only this file
can show is the launch code, the segment order the sort and the scan produce, and a lost `#pragma clang fp contract(off)`: gfx950 has
fused multiply-add, and origin + (i + 0.5) * s or origin + c * s would contract.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched, and so must the rows beyond the V voxels (U vertices) a call produces."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxel_cases as VC  # noqa: E402
import voxel_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -77
OUTPUTS = ("grid_index", "counts", "first", "points", "colors", "normals")
SPEC = {"grid_index": ((3,), np.int32), "counts": ((), np.int32), "first": ((), np.int32), "points": ((3,), np.float64), "colors": ((3,), np.float64),
        "normals": ((3,), np.float64)}


@pytest.fixture(scope="module")
def g19():
    with np.load(O.GOLDEN, allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


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
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(eng.device)          # a copy: the shared inputs are read-only


def same(a, b):
    """equal bits, a NaN equal to a NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return same(a, b) if a.dtype == np.float64 else (a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b))


class Framed:
    """An output of `shape` x `dtype` between two bands of sentinel bytes, in one device allocation, pre-filled."""

    def __init__(self, eng, shape, dtype):
        import torch
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        host = np.full(2 * BAND + self.n, SENT, np.uint8)
        host[BAND:BAND + self.n] = FILL
        self.buf = torch.from_numpy(host).to(eng.device)
        self.ptr = self.buf.data_ptr() + BAND

    def result(self, what, rows=None):
        """the output; with `rows`, its first rows, the rest still pre-filled"""
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        out = host[BAND:BAND + self.n].view(self.dtype).reshape(self.shape)
        if rows is None:
            return out
        assert (out[rows:].view(np.uint8) == FILL).all(), (what, "a row beyond the result was written")
        return out[:rows]

    def untouched(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all() and (host[BAND:BAND + self.n] == FILL).all(), what


class Batch:
    """Clouds `which` of a case through im_voxel_bounds, im_voxel_keys, torch's sort and im_voxel_reduce, every output framed."""

    def __init__(self, eng, case, which=None, per_cloud=None):
        import torch
        self.eng, self.case, self.name = eng, case, case["name"]
        self.which = list(range(len(case["clouds"]))) if which is None else list(which)
        sub = {k: None if case[k] is None else [case[k][e] for e in self.which] for k in ("clouds", "colors", "normals")}
        self.pts, self.col, self.nrm, self.offsets = VC.packed(sub)
        self.E, self.n = len(self.which), len(self.pts)
        self.per_cloud = case["per_cloud"] if per_cloud is None else per_cloud
        self.cloud_grids = [VC.grid_of(case, e) for e in self.which]
        self.grids = np.ascontiguousarray(self.cloud_grids if self.per_cloud else self.cloud_grids[:1]).reshape(-1, 7)
        self.d_pts, self.d_col, self.d_nrm = dev(eng, self.pts), dev(eng, self.col), dev(eng, self.nrm)
        st = eng.stream_ptr()
        bounds = Framed(eng, (self.E, 6), np.float64)
        eng.ctx.call("im_voxel_bounds", p(self.d_pts), self.offsets.ctypes.data, self.E, bounds.ptr, st)
        self.bounds = bounds.result((self.name, "bounds"))
        key, dropped = Framed(eng, (self.n,), np.int64), Framed(eng, (self.E,), np.int64)
        eng.ctx.call("im_voxel_keys", p(self.d_pts), *self.head(), key.ptr, dropped.ptr, st)
        self.key, self.dropped = key.result((self.name, "keys")), dropped.result((self.name, "dropped"))
        self.skey, self.perm = torch.sort(dev(eng, self.key), stable=True)

    def head(self):
        return (self.offsets.ctypes.data, self.E, self.grids.ctypes.data, int(self.per_cloud))

    def reduce(self, outputs=OUTPUTS, inputs=("points", "colors", "normals")):
        """{output: its first V rows}, nvox [E + 1]; the outputs not asked for are passed as NULL"""
        eng = self.eng
        frames = {k: Framed(eng, (self.n,) + SPEC[k][0], SPEC[k][1]) for k in OUTPUTS}
        nvox = Framed(eng, (self.E + 1,), np.int64)
        ins = [d if k in inputs else None for k, d in (("points", self.d_pts), ("colors", self.d_col), ("normals", self.d_nrm))]
        eng.ctx.call("im_voxel_reduce", *self.head(), p(self.skey), p(self.perm), *[p(d) for d in ins], nvox.ptr,
                     *[frames[k].ptr if k in outputs else None for k in OUTPUTS], eng.stream_ptr())
        nv = nvox.result((self.name, "nvox"))
        V = int(nv[self.E])
        out = {}
        for k, given in zip(OUTPUTS, [True] * 3 + [d is not None for d in ins]):
            if k in outputs and given:
                out[k] = frames[k].result((self.name, k), rows=V)
            else:
                frames[k].untouched((self.name, k, "not asked for"))
        return out, nv

    def want(self):
        return [VC.full(self.name)[e] for e in self.which]

    def check(self, out, nvox, what):
        wants = self.want()
        base = O.key_bases(self.grids, self.per_cloud, self.E)
        for k, (e, w) in enumerate(zip(self.which, wants)):
            a, b = self.offsets[k], self.offsets[k + 1]
            keys = np.where(w["keys"] == O.DROPPED, O.DROPPED, w["keys"] + np.int64(base[k]))
            assert np.array_equal(self.key[a:b], keys) and self.dropped[k] == w["dropped"], (what, e, "keys")
            ob = O.bounds(self.case["clouds"][e])
            assert same(self.bounds[k], np.concatenate(ob)), (what, e, "bounds", self.bounds[k], ob)
        sizes = [len(w["counts"]) for w in wants]
        assert np.array_equal(nvox, np.concatenate([[0], np.cumsum(sizes)])), (what, nvox, sizes)
        for name, got in out.items():
            parts = [w[name] for w in wants]
            if parts[0] is None:
                continue
            assert equal(got, np.concatenate(parts).astype(SPEC[name][1])), (what, name)


# ---- (a) every case through the C entry points -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.names())
def test_c_entry_points_equal_the_oracle(eng, name):
    from icepy4d_amd.post_processing import voxel_grid as VG
    assert VG.max_points() == O.MAX_POINTS
    b = Batch(eng, VC.by_name(name))
    out, nvox = b.reduce()
    case = VC.by_name(name)
    assert set(out) == {"grid_index", "counts", "first", "points"} | ({"colors"} if case["colors"] else set()) | ({"normals"} if case["normals"] else set())
    b.check(out, nvox, name)


@pytest.mark.parametrize("name", ["voxels_257", "batch_3_one_empty"])
def test_each_optional_output_works_alone(eng, name):
    b = Batch(eng, VC.by_name(name))
    everything, nvox = b.reduce()
    for k in OUTPUTS:
        out, nv = b.reduce(outputs=(k,))
        assert list(out) == [k] and equal(out[k], everything[k]) and np.array_equal(nv, nvox), (name, k)
    out, nv = b.reduce(outputs=())
    assert out == {} and np.array_equal(nv, nvox)
    out, nv = b.reduce(inputs=("colors",))                          # an attribute that is not given: its mean is not written
    assert set(out) == {"grid_index", "counts", "first", "colors"} and equal(out["colors"], everything["colors"])


@pytest.mark.parametrize("name", ["voxels_65537", "batch_3_one_empty", "one_voxel_1025"])
def test_two_runs_are_identical(eng, name):
    a, b = Batch(eng, VC.by_name(name)), Batch(eng, VC.by_name(name))
    (oa, na), (ob, nb) = a.reduce(), b.reduce()
    assert np.array_equal(a.key, b.key) and np.array_equal(na, nb) and all(equal(oa[k], ob[k]) for k in oa)


@pytest.mark.parametrize("name", ["batch_3_one_empty", "batch_3_per_cloud", "batch_3_no_colours", "cap_under_3_clouds", "cap_per_cloud_3"])
def test_a_batch_equals_its_single_cloud_calls(eng, name):
    case = VC.by_name(name)
    full, nvox = Batch(eng, case).reduce()
    for order in ([0], [1], [2], [2, 1, 0], [1, 2, 0]):
        b = Batch(eng, case, which=order)
        out, nv = b.reduce()
        b.check(out, nv, (name, order))
        for k, e in enumerate(order):
            for key in out:
                assert equal(out[key][nv[k]:nv[k + 1]], full[key][nvox[e]:nvox[e + 1]]), (name, order, key)


def test_shared_grids_equal_per_cloud_grids(eng):
    case = VC.by_name("batch_3_one_empty")
    shared, per = Batch(eng, case), Batch(eng, case, per_cloud=True)
    assert len(per.grids) == 3 and len(shared.grids) == 1
    (os_, ns), (op, np_) = shared.reduce(), per.reduce()
    assert np.array_equal(shared.key, per.key) and np.array_equal(shared.dropped, per.dropped) and np.array_equal(ns, np_)
    assert all(equal(os_[k], op[k]) for k in os_)


# ---- (b) the box mesh ------------------------------------------------------------------------------------------------------------------------
def run_mesh(eng, c, colours=True):
    import torch
    V = len(c["grid_index"])
    d_index, d_col = dev(eng, c["grid_index"]), dev(eng, c["colors"])
    st = eng.stream_ptr()
    ckey = Framed(eng, (8 * V,), np.int64)
    eng.ctx.call("im_voxel_mesh_corners", c["grid"].ctypes.data, p(d_index), V, ckey.ptr, st)
    keys = ckey.result("corner keys")
    skey, perm = torch.sort(dev(eng, keys), stable=True)
    nvert, vert, vcol, tri = Framed(eng, (1,), np.int64), Framed(eng, (8 * V, 3), np.float64), Framed(eng, (8 * V, 3), np.float64), Framed(eng, (12 * V, 3), np.int32)
    eng.ctx.call("im_voxel_mesh", c["grid"].ctypes.data, V, p(d_col) if colours else None, p(skey), p(perm), nvert.ptr, vert.ptr, vcol.ptr, tri.ptr, st)
    U = int(nvert.result("n_vertices")[0])
    if not colours:
        vcol.untouched("vertex colours without colours")
    return keys, vert.result("vertices", rows=U), vcol.result("vertex colours", rows=U) if colours else None, tri.result("triangles")


@pytest.mark.parametrize("name", VC.mesh_names())
def test_mesh_equals_the_oracle(eng, name):
    c = VC.mesh_by_name(name)
    want_v, want_c, want_t = VC.mesh_full(name)
    keys, vert, vcol, tri = run_mesh(eng, c)
    assert len(np.unique(keys)) == len(want_v), name
    assert same(vert, want_v) and same(vcol, want_c) and equal(tri, want_t), name
    if c["vertices"] is not None:
        assert len(vert) == c["vertices"], name
    if name in ("block_2x2x2", "voxels_32"):
        _, vert2, none, tri2 = run_mesh(eng, c, colours=False)
        assert none is None and same(vert2, want_v) and equal(tri2, want_t)


# ---- (c) the same cases through the Python entry points --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.names())
def test_python_entry_points_equal_the_oracle(eng, name):
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.post_processing import VoxelGrid
    from icepy4d_amd.utils.point_cloud_filters import voxel_down_sample
    case = VC.by_name(name)
    e = len(case["clouds"]) - 1                                          # the last cloud of the case, one of each
    pts, col, nrm, grid, want = case["clouds"][e], VC.attr(case, "colors", e), VC.attr(case, "normals", e), VC.grid_of(case, e), VC.full(name)[e]
    vg = VoxelGrid.create_from_point_cloud_within_bounds(pts, grid[6], grid[:3], grid[3:6], colors=col, engine=eng)
    assert equal(vg.grid_indices, want["grid_index"]) and equal(vg.counts, want["counts"]) and vg.dropped == want["dropped"] and len(vg) == len(want["counts"])
    assert vg.has_colors() == (col is not None) and same(vg.colors, want["colors"] if col is not None else np.zeros((len(vg), 3)))
    assert same(vg.centers(), O.centers(grid, want["grid_index"]).reshape(-1, 3)) and same(vg.origin, grid[:3]) and vg.voxel_size == grid[6]
    pc = PointCloud(points3d=np.array(pts), points_col=None if col is None else np.array(col))
    pc.normals = None if nrm is None else np.array(nrm)
    vg2 = VoxelGrid.create_from_point_cloud_within_bounds(pc, grid[6], grid[:3], grid[3:6], engine=eng)
    assert equal(vg2.grid_indices, vg.grid_indices) and same(vg2.colors, vg.colors)
    # the grid of the cloud's own bounds, and the down-sampling over it
    s = float(grid[6]) * 1.5
    ds = O.down_sample(pts, s, col, nrm)
    auto = VoxelGrid.create_from_point_cloud(pts, s, colors=col, engine=eng)
    got = voxel_down_sample(pts, s, col, nrm, engine=eng)
    thin = pc.voxel_down_sample(s, engine=eng)
    if ds["grid"] is None:
        assert len(auto) == 0 and len(got[0]) == 0 and len(thin) == 0 and auto.dropped == len(pts)
        return
    assert same(auto.grid, ds["grid"]) and equal(auto.grid_indices, ds["grid_index"]) and equal(auto.counts, ds["counts"]) and auto.dropped == ds["dropped"]
    assert same(got[0], ds["points"]) and equal(got[3], ds["counts"]) and equal(got[4], ds["first"])
    for g, w in ((got[1], ds["colors"]), (got[2], ds["normals"]), (thin.colors, ds["colors"]), (thin.normals, ds["normals"])):
        assert (g is None and w is None) or same(g, w), name
    assert same(thin.points, ds["points"]) and len(pc) == len(pts)       # the input is left alone
    if len(auto) and 8 * len(auto) <= 2 ** 16:
        mv, mc, mt = auto.to_box_mesh()
        wv, wc, wt = O.box_mesh(ds["grid"], ds["grid_index"], ds["colors"] if col is not None else np.zeros((len(auto), 3)))
        assert same(mv, wv) and same(mc, wc) and equal(mt, wt), name


@pytest.mark.parametrize("name", ["batch_3_one_empty", "batch_3_no_colours", "cap_under_3_clouds", "voxels_257"])
def test_voxel_series_whole_and_split(eng, name, monkeypatch):
    from icepy4d_amd import voxelization as VX
    from icepy4d_amd.post_processing import voxel_grid as VG
    case, wants = VC.by_name(name), VC.full(name)
    grid = case["grids"][0]
    clouds = [c if case["colors"] is None else (c, case["colors"][e]) for e, c in enumerate(case["clouds"])]

    def check(grids):
        assert len(grids) == len(wants)
        for vg, w in zip(grids, wants):
            assert equal(vg.grid_indices, w["grid_index"]) and equal(vg.counts, w["counts"]) and vg.dropped == w["dropped"], name
            assert same(vg.colors, w["colors"] if w["colors"] is not None else np.zeros((len(vg), 3))), name

    check(VX.voxel_series(clouds, grid[6], grid[:3], grid[3:6], engine=eng))
    sizes = [len(c) for c in case["clouds"]]
    monkeypatch.setattr(VG, "max_points", lambda: max(max(sizes), sum(sizes) - 1))                   # one point too few for one call
    assert len(VG._batches(sizes, VG.max_points())) == (2 if len(sizes) > 1 else 1)
    check(VX.voxel_series(clouds, grid[6], grid[:3], grid[3:6], engine=eng))


# ---- (d) the reference's outputs -------------------------------------------------------------------------------------------------------------
def test_g19_through_voxelize(eng, g19, tmp_path):
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.voxelization import voxelize
    work = tmp_path / "test" / "voxelization"
    path = work / "dense_2022_05_01.ply"
    PointCloud(points3d=np.array(g19["points"]), points_col=g19["colors_u8"] / 255.0).write_ply(path)
    grids = voxelize([path], engine=eng, write_grid=True, write_mesh=True)          # the script's defaults: 0.2 and its box
    assert (work / g19["text_name"].tobytes().decode()).read_bytes() == g19["text"].tobytes()
    vg = grids[0]
    assert equal(vg.grid_indices, g19["grid_index"]) and same(vg.colors, g19["voxel_colors"]) and equal(vg.counts, g19["counts"]) and vg.dropped == 120
    vert, vcol, tri = vg.to_box_mesh()
    mine = {v.tobytes(): c for v, c in zip(vert, vcol)}
    theirs = {v.tobytes(): c for v, c in zip(g19["mesh_vertices"], g19["mesh_vertex_colors"])}
    assert set(mine) == set(theirs) and len(mine) == len(vert) and all(same(mine[k], theirs[k]) for k in mine)
    assert same(vert[tri], g19["mesh_vertices"][g19["mesh_triangles"]])
    assert (work / "voxel_grid.ply").read_text().count("\n") == 17 + 2 + len(vg) and (work / "vox_mesh.ply").stat().st_size > 13 * len(tri)


# ---- (e) refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(eng, name, *args):
    from icepy4d_amd._lib import IcematchError
    with pytest.raises(IcematchError) as e:
        eng.ctx.call(name, *args)
    assert e.value.rc == REFUSED, (name, e.value)


def test_refusals_leave_the_outputs_alone(eng):
    b = Batch(eng, VC.by_name("batch_3_one_empty"))
    st = eng.stream_ptr()
    E, n, off, grids = b.E, b.n, b.offsets, b.grids
    descending, shifted, too_many = off.copy(), off + 1, np.array([0, 2 ** 26 + 1], np.int64)
    descending[2] = descending[1] - 1
    bad_grids = []
    for k, v in ((6, 0.0), (6, -0.3), (6, np.nan), (6, np.inf), (1, np.nan), (4, np.inf), (0, -np.inf), (3, -1.0)):
        g = grids.copy()
        g[0, k] = v
        bad_grids.append(g)
    bad_grids += [VC.cap_grid(1)[0].reshape(1, 7), VC.cap_grid_3(1)[0].reshape(1, 7)]                # over 2^62 alone; over it with E = 3
    per = np.ascontiguousarray(VC.by_name("cap_per_cloud_3")["grids"]).copy()
    per[2, 5] += 1.0                                                                                 # 2^61 + 2^60 + 2^60 + 2^40 voxels
    good = (off.ctypes.data, E, grids.ctypes.data, 0)

    def heads():
        yield (None,) + good[1:]
        yield good[:2] + (None,) + good[3:]
        yield (descending.ctypes.data,) + good[1:]
        yield (shifted.ctypes.data,) + good[1:]
        yield (good[0], -1) + good[2:]
        yield (good[0], 65536) + good[2:]
        yield (too_many.ctypes.data, 1) + good[2:]
        for g in bad_grids:
            yield good[:2] + (g.ctypes.data, 0)
        yield good[:2] + (per.ctypes.data, 1)

    key, dropped = Framed(eng, (n,), np.int64), Framed(eng, (E,), np.int64)
    frames = {k: Framed(eng, (n,) + SPEC[k][0], SPEC[k][1]) for k in OUTPUTS}
    nvox = Framed(eng, (E + 1,), np.int64)
    outs = [frames[k].ptr for k in OUTPUTS]
    ins = (p(b.d_pts), p(b.d_col), p(b.d_nrm))

    def all_untouched(what):
        for f in [key, dropped, nvox] + list(frames.values()):
            f.untouched(what)

    for k, head in enumerate(heads()):
        refused(eng, "im_voxel_keys", p(b.d_pts), *head, key.ptr, dropped.ptr, st)
        refused(eng, "im_voxel_reduce", *head, p(b.skey), p(b.perm), *ins, nvox.ptr, *outs, st)
        all_untouched(("head", k))
    for args in ((None, *good, key.ptr, dropped.ptr), (p(b.d_pts), *good, None, dropped.ptr), (p(b.d_pts), *good, key.ptr, None)):
        refused(eng, "im_voxel_keys", *args, st)
    for tail in ((None, p(b.perm), *ins, nvox.ptr), (p(b.skey), None, *ins, nvox.ptr), (p(b.skey), p(b.perm), *ins, None)):
        refused(eng, "im_voxel_reduce", *good, *tail, *outs, st)
    all_untouched("null pointers")
    bounds = Framed(eng, (E, 6), np.float64)
    for args in ((None, off.ctypes.data, E, bounds.ptr), (p(b.d_pts), None, E, bounds.ptr), (p(b.d_pts), off.ctypes.data, E, None),
                 (p(b.d_pts), descending.ctypes.data, E, bounds.ptr), (p(b.d_pts), shifted.ctypes.data, E, bounds.ptr), (p(b.d_pts), off.ctypes.data, -1, bounds.ptr),
                 (p(b.d_pts), too_many.ctypes.data, 1, bounds.ptr)):
        refused(eng, "im_voxel_bounds", *args, st)
        bounds.untouched(("im_voxel_bounds", args[2]))
    # E == 0 returns 0 and launches nothing
    zero = np.zeros(1, np.int64)
    eng.ctx.call("im_voxel_bounds", p(b.d_pts), zero.ctypes.data, 0, bounds.ptr, st)
    eng.ctx.call("im_voxel_keys", p(b.d_pts), zero.ctypes.data, 0, grids.ctypes.data, 0, key.ptr, dropped.ptr, st)
    eng.ctx.call("im_voxel_reduce", zero.ctypes.data, 0, grids.ctypes.data, 0, p(b.skey), p(b.perm), *ins, nvox.ptr, *outs, st)
    all_untouched("E == 0")
    bounds.untouched("E == 0")
    # the mesh
    c = VC.mesh_by_name("block_2x2x2")
    V = len(c["grid_index"])
    d_index, d_col = dev(eng, c["grid_index"]), dev(eng, c["colors"])
    keys, _, _, _ = run_mesh(eng, c)
    import torch
    skey, perm = torch.sort(dev(eng, keys), stable=True)
    ckey, nvert = Framed(eng, (8 * V,), np.int64), Framed(eng, (1,), np.int64)
    vert, vcol, tri = Framed(eng, (8 * V, 3), np.float64), Framed(eng, (8 * V, 3), np.float64), Framed(eng, (12 * V, 3), np.int32)
    mesh_bad = [g.reshape(7) for g in bad_grids[:8]] + [VC.cap_grid(0)[0]]                          # 2^62 voxels, more corner keys
    gp = c["grid"].ctypes.data
    corner_calls = [(None, p(d_index), V, ckey.ptr), (gp, None, V, ckey.ptr), (gp, p(d_index), V, None), (gp, p(d_index), -1, ckey.ptr), (gp, p(d_index), 2 ** 24 + 1, ckey.ptr)]
    corner_calls += [(g.ctypes.data, p(d_index), V, ckey.ptr) for g in mesh_bad]
    for k, args in enumerate(corner_calls):
        refused(eng, "im_voxel_mesh_corners", *args, st)
        ckey.untouched(("im_voxel_mesh_corners", k))
    ok = (gp, V, p(d_col), p(skey), p(perm), nvert.ptr, vert.ptr, vcol.ptr, tri.ptr)
    mesh_calls = [(None,) + ok[1:], ok[:1] + (-1,) + ok[2:], ok[:1] + (2 ** 24 + 1,) + ok[2:], ok[:3] + (None,) + ok[4:], ok[:4] + (None,) + ok[5:],
                  ok[:5] + (None,) + ok[6:], ok[:6] + (None,) + ok[7:], ok[:8] + (None,)]
    mesh_calls += [(g.ctypes.data,) + ok[1:] for g in mesh_bad]
    for k, args in enumerate(mesh_calls):
        refused(eng, "im_voxel_mesh", *args, st)
        for f in (nvert, vert, vcol, tri):
            f.untouched(("im_voxel_mesh", k))
    eng.ctx.call("im_voxel_mesh_corners", gp, p(d_index), 0, ckey.ptr, st)                           # V == 0 launches nothing
    ckey.untouched("V == 0")
    eng.ctx.call("im_voxel_mesh", gp, 0, p(d_col), p(skey), p(perm), nvert.ptr, vert.ptr, vcol.ptr, tri.ptr, st)
    assert nvert.result("V == 0")[0] == 0
    for f in (vert, vcol, tri):
        f.untouched("V == 0")


def test_wrong_keys_and_permutations_stay_inside(eng):
    """Keys that are not sorted and a permutation that is none give meaningless figures; the bands around every output hold."""
    import torch
    b = Batch(eng, VC.by_name("voxels_257"))
    rng = np.random.default_rng(3)
    b.skey = dev(eng, rng.integers(-5, 600, b.n).astype(np.int64))
    b.perm = dev(eng, rng.integers(-2 ** 40, 2 ** 40, b.n).astype(np.int64))
    eng_out = {k: Framed(eng, (b.n,) + SPEC[k][0], SPEC[k][1]) for k in OUTPUTS}
    nvox = Framed(eng, (b.E + 1,), np.int64)
    eng.ctx.call("im_voxel_reduce", *b.head(), p(b.skey), p(b.perm), p(b.d_pts), p(b.d_col), p(b.d_nrm), nvox.ptr, *[eng_out[k].ptr for k in OUTPUTS], eng.stream_ptr())
    for k in OUTPUTS:
        eng_out[k].result(("wrong keys", k))
    assert 0 <= nvox.result("wrong keys")[b.E] <= b.n
    c = VC.mesh_by_name("voxels_33")
    V = len(c["grid_index"])
    nvert, vert, vcol, tri = Framed(eng, (1,), np.int64), Framed(eng, (8 * V, 3), np.float64), Framed(eng, (8 * V, 3), np.float64), Framed(eng, (12 * V, 3), np.int32)
    skey = dev(eng, rng.integers(-5, 2 ** 62, 8 * V).astype(np.int64))
    perm = dev(eng, rng.integers(-2 ** 40, 2 ** 40, 8 * V).astype(np.int64))
    eng.ctx.call("im_voxel_mesh", c["grid"].ctypes.data, V, p(dev(eng, c["colors"])), p(skey), p(perm), nvert.ptr, vert.ptr, vcol.ptr, tri.ptr, eng.stream_ptr())
    for f in (nvert, vert, vcol, tri):
        f.result("wrong corner keys")
    torch.cuda.synchronize()
