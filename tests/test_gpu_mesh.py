"""Mesh filters, the convex-hull crop and uniform mesh sampling (csrc/mesh.hip, csrc/mesh_tri.h) on the device, on every case of
tests/mesh_cases.py (each size at which a kernel takes another path: see that file), through the C entry points and through
`TriangleMesh`, `point_in_hull` and `MeshingPoisson`, two runs against each other, the reference's call chain in
tests/golden/g20_meshing.npz, wrong inputs and the refusals.

Bounds. Everything is equality: vertex maps, kept lists, renumbered triangles, keys, merge maps, keep flags, the census, hull masks,
areas, allocation tables, sample points, colours, normals and triangle numbers are bit-identical to the numpy restatement
(tests/mesh_oracle.py). Derived, not measured: the kernels and the restatement perform the same IEEE float64 operations in the same order
with contraction off (float64 division and square root are correctly rounded on the device, the library is built without a fast-math
flag); flags, maxima of bit patterns and integer prefix sums are order-free; the stable sort keeps the lowest index first in a run. A NaN
compares equal to a NaN. The host build of the same text agrees with the restatement on the same cases (tests/test_mesh_cpu.py); what only
this file can show is the launch code, the scans, the LDS staging of the facets and a lost `#pragma clang fp contract(off)`.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched, and so must the rows beyond what a call produces."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_cases as MC  # noqa: E402
import mesh_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -78


@pytest.fixture(scope="module")
def g20():
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


def dev(eng, a, dtype=None):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(eng.device)          # a copy: the shared inputs are read-only


def same(a, b):
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


def raw(eng, name, *args):
    """the return code of a C call, without raising"""
    return getattr(eng.ctx.lib, name)(eng.ctx.h, *args)


def u8(eng, a):
    return None if a is None else dev(eng, np.asarray(a).astype(np.uint8))


def c_select(eng, what, V, tri, vkeep=None, merge=None, tkeep=None, degenerate=0, unreferenced=0, check=True):
    T = len(tri)
    d_tri = dev(eng, tri, np.int32)
    vmap, vlist, tout, tpos, counts = Framed(eng, (V,), np.int32), Framed(eng, (V,), np.int32), Framed(eng, (T, 3), np.int32), Framed(eng, (T,), np.int32), Framed(eng, (2,), np.int64)
    d_keep, d_merge, d_tkeep = u8(eng, vkeep), dev(eng, merge, np.int32), u8(eng, tkeep)
    eng.ctx.call("im_mesh_select", p(d_keep), V, p(d_tri), T, p(d_merge), p(d_tkeep), degenerate, unreferenced, vmap.ptr, vlist.ptr, tout.ptr, tpos.ptr, counts.ptr,
                 eng.stream_ptr())
    eng.synchronize()
    nv, nt = (int(c) for c in counts.result((what, "counts")))
    if not check:
        vmap.result(what), vlist.result(what), tout.result(what), tpos.result(what)
        return nv, nt
    return vmap.result((what, "vmap")), vlist.result((what, "vlist"), nv), tout.result((what, "triangles"), nt), tpos.result((what, "pos"), nt)


def c_first(eng, what, keys, perm=None, outputs=("first", "keep")):
    from icepy4d_amd.post_processing.triangle_mesh import sort_keys
    n = len(keys[0])
    d_keys = [dev(eng, k, np.int64) for k in keys] + [None] * (3 - len(keys))
    d_perm = sort_keys([k for k in d_keys if k is not None]) if perm is None else dev(eng, perm, np.int64)
    first, keep = Framed(eng, (n,), np.int32), Framed(eng, (n,), np.uint8)
    eng.ctx.call("im_mesh_first_of_segment", n, p(d_keys[0]), p(d_keys[1]), p(d_keys[2]), p(d_perm), first.ptr if "first" in outputs else None,
                 keep.ptr if "keep" in outputs else None, eng.stream_ptr())
    eng.synchronize()
    for name, f in (("first", first), ("keep", keep)):
        if name not in outputs:
            f.untouched((what, name, "not asked for"))
    return first.result((what, "first")) if "first" in outputs else None, keep.result((what, "keep")) if "keep" in outputs else None


def c_keys(eng, what, v, t):
    V, T = len(v), len(t)
    d_v, d_t = dev(eng, v), dev(eng, t, np.int32)
    tk = [Framed(eng, (T,), np.int64) for _ in range(2)]
    vk = [Framed(eng, (V,), np.int64) for _ in range(3)]
    ek = Framed(eng, (3 * T,), np.int64)
    st = eng.stream_ptr()
    eng.ctx.call("im_mesh_triangle_keys", p(d_t), T, tk[0].ptr, tk[1].ptr, st)
    eng.ctx.call("im_mesh_vertex_keys", p(d_v), V, vk[0].ptr, vk[1].ptr, vk[2].ptr, st)
    eng.ctx.call("im_mesh_edge_keys", p(d_t), T, ek.ptr, st)
    eng.synchronize()
    if T == 0:
        [f.untouched((what, "zero-size")) for f in tk + [ek]]
    if V == 0:
        [f.untouched((what, "zero-size")) for f in vk]
    return [f.result(what) for f in tk], [f.result(what) for f in vk], ek.result(what)


def c_census(eng, what, keys, sort=True):
    import torch
    d = dev(eng, keys, np.int64)
    if sort:
        d, _ = torch.sort(d)
    count = Framed(eng, (1,), np.int64)
    eng.ctx.call("im_mesh_edge_census", p(d), len(keys), count.ptr, eng.stream_ptr())
    eng.synchronize()
    return int(count.result((what, "census"))[0])


def c_sample(eng, what, v, t, N, seed, col=None, nrm=None, outputs=("colors", "normals", "triangle", "area"), table=None):
    V, T = len(v), len(t)
    d_v, d_t, d_c, d_n = dev(eng, v), dev(eng, t, np.int32), dev(eng, col), dev(eng, nrm)
    st = eng.stream_ptr()
    end, area = Framed(eng, (T,), np.int64), Framed(eng, (T,), np.float64)
    total = np.full(1, -7, np.int64)
    if table is None:
        eng.ctx.call("im_mesh_sample_table", p(d_v), V, p(d_t), T, N, area.ptr if "area" in outputs else None, end.ptr, total.ctypes.data, st)
        eng.synchronize()
        out = {"count_end": end.result((what, "count_end")), "C": int(total[0]), "area": area.result((what, "area")) if "area" in outputs and T else None}
        d_end = end.ptr
    else:
        out, d_table = {}, dev(eng, table, np.int64)
        d_end = p(d_table)
    pts, cols, nrms, which = Framed(eng, (N, 3), np.float64), Framed(eng, (N, 3), np.float64), Framed(eng, (N, 3), np.float64), Framed(eng, (N,), np.int32)
    eng.ctx.call("im_mesh_sample", p(d_v), V, p(d_t), T, d_end, N, seed, p(d_c), p(d_n), pts.ptr, cols.ptr if "colors" in outputs else None,
                 nrms.ptr if "normals" in outputs else None, which.ptr if "triangle" in outputs else None, st)
    eng.synchronize()
    out["points"] = pts.result((what, "points"))
    for name, f, written in (("colors", cols, col is not None), ("normals", nrms, True), ("triangle", which, True)):
        if name in outputs and written and N:
            out[name] = f.result((what, name))
        else:
            f.untouched((what, name, "not asked for"))
            out[name] = None
    return out


# ---- the filters through the C entry points --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.names())
def test_filters_through_the_c_abi(eng, name):
    c = MC.by_name(name)
    v, t = c["vertices"], c["triangles"]
    V, T = len(v), len(t)
    keep_index = np.zeros(V, bool)
    keep_index[c["index"]] = True
    variants = {"by_mask": dict(vertex_keep=~c["mask"]), "by_index": dict(vertex_keep=keep_index, drop_unreferenced=True),
                "by_index_no_cleanup": dict(vertex_keep=keep_index), "degenerate": dict(drop_degenerate=True), "unreferenced": dict(drop_unreferenced=True),
                "everything": dict(vertex_keep=~c["mask"], drop_degenerate=True, drop_unreferenced=True)}
    for what, kw in variants.items():
        got = c_select(eng, (name, what), V, t, kw.get("vertex_keep"), None, None, int(kw.get("drop_degenerate", False)), int(kw.get("drop_unreferenced", False)))
        assert all(equal(a, b) for a, b in zip(got, O.select(V, t, **kw))), (name, what)
    (tk, vk, ek) = c_keys(eng, name, v, t)
    assert all(equal(a, b) for a, b in zip(tk, O.triangle_keys(t))) and all(equal(a, b) for a, b in zip(vk, O.vertex_keys(v))) and equal(ek, O.edge_keys(t)), name
    # duplicate triangles: keys, the sorts, the first of every segment, the select
    first, keep = c_first(eng, (name, "triangles"), O.triangle_keys(t))
    wfirst, wkeep = O.first_of_segment(*O.triangle_keys(t))
    assert equal(first, wfirst) and equal(keep.astype(bool), wkeep), name
    got = c_select(eng, (name, "dup_tri"), V, t, tkeep=keep)
    assert all(equal(a, b) for a, b in zip(got, O.select(V, t, triangle_keep=wkeep))), name
    # duplicate vertices: three keys, the merge map
    first, keep = c_first(eng, (name, "vertices"), O.vertex_keys(v))
    wfirst, wkeep = O.first_of_segment(*O.vertex_keys(v))
    assert equal(first, wfirst) and equal(keep.astype(bool), wkeep), name
    got = c_select(eng, (name, "dup_vert"), V, t, vkeep=keep, merge=first)
    assert all(equal(a, b) for a, b in zip(got, O.select(V, t, vertex_keep=wkeep, merge=wfirst))), name
    assert c_census(eng, name, O.edge_keys(t)) == O.edge_census(t), name


@pytest.mark.parametrize("name", MC.names())
def test_sampling_through_the_c_abi(eng, name):
    c = MC.by_name(name)
    v, t = c["vertices"], c["triangles"]
    area = O.areas(v, t)
    for N in c["samples"]:
        if area.sum() == 0 and N > 0:
            continue
        want = O.sample(v, t, N, c["seed"], c["colors"], c["normals"])
        got = c_sample(eng, (name, N), v, t, N, c["seed"], c["colors"], c["normals"])
        assert equal(got["count_end"], want["count_end"]) and got["C"] == O.sample_table(area, N)[2], (name, N)
        assert len(t) == 0 or same(got["area"], area), (name, N)
        assert same(got["points"], want["points"]), (name, N)
        if N:
            assert equal(got["triangle"], want["triangle"]) and same(got["normals"], want["normals"]), (name, N)
            assert (got["colors"] is None and want["colors"] is None) or same(got["colors"], want["colors"]), (name, N)


def test_each_optional_output_alone_and_two_runs(eng):
    c = MC.by_name("strip_257")
    v, t = c["vertices"], c["triangles"]
    col = np.random.default_rng(8).uniform(0, 1, v.shape)
    want = O.sample(v, t, 513, 9, col, c["normals"])
    full = c_sample(eng, "full", v, t, 513, 9, col, c["normals"])
    for only in ((), ("colors",), ("normals",), ("triangle",), ("area",)):
        got = c_sample(eng, ("only", only), v, t, 513, 9, col, c["normals"], outputs=only)
        assert same(got["points"], want["points"]), only
        for k in only:
            assert equal(got[k], full[k]), (only, k)
    assert same(full["colors"], want["colors"]) and same(full["normals"], want["normals"])
    plain = c_sample(eng, "no vertex normals", v, t, 513, 9)
    assert same(plain["normals"], O.sample(v, t, 513, 9)["normals"]) and plain["colors"] is None
    again = c_sample(eng, "again", v, t, 513, 9, col, c["normals"])
    assert all(equal(again[k], full[k]) for k in ("points", "colors", "normals", "triangle", "count_end", "area"))
    other = c_sample(eng, "seed", v, t, 513, 10, col, c["normals"])
    assert not np.array_equal(other["points"], full["points"]) and equal(other["triangle"], full["triangle"])
    for seed in (-1, -2 ** 63, 2 ** 63 - 1):                                           # the seed is 64 bits, whatever its sign
        assert same(c_sample(eng, seed, v, t, 65, seed)["points"], O.sample(v, t, 65, seed)["points"]), seed
    # im_mesh_first_of_segment: d_first alone, d_keep alone, neither
    dup = MC.by_name("field_with_duplicates")
    for keys in (O.vertex_keys(dup["vertices"]), O.triangle_keys(dup["triangles"])):
        wfirst, wkeep = O.first_of_segment(*keys)
        assert not wkeep.all()
        first, none = c_first(eng, "first alone", keys, outputs=("first",))
        assert none is None and equal(first, wfirst)
        none, keep = c_first(eng, "keep alone", keys, outputs=("keep",))
        assert none is None and equal(keep.astype(bool), wkeep)
        assert c_first(eng, "neither", keys, outputs=()) == (None, None)
    a = c_select(eng, "run 1", len(v), t, ~c["mask"], None, None, 1, 1)
    b = c_select(eng, "run 2", len(v), t, ~c["mask"], None, None, 1, 1)
    assert all(equal(x, y) for x, y in zip(a, b))


# ---- the hull -----------------------------------------------------------------------------------------------------------------------------------
def c_in_hull(eng, what, q, facets):
    inside = Framed(eng, (len(q),), np.uint8)
    d_q = dev(eng, q)
    facets = np.ascontiguousarray(facets, np.float64)
    eng.ctx.call("im_mesh_in_hull", p(d_q), len(q), facets.ctypes.data, len(facets), inside.ptr, eng.stream_ptr())
    eng.synchronize()
    return inside.result((what, "inside")).astype(bool)


@pytest.mark.parametrize("F", MC.HULL_FACETS)
def test_hull_through_the_c_abi(eng, F):
    facets = MC.tangent_facets(F)
    for n in (1, 255, 257):
        q = MC.hull_queries(facets)[:n] if n < 255 else MC.hull_queries(facets, n=n)
        assert np.array_equal(c_in_hull(eng, (F, n), q, facets), O.point_in_hull(q, facets)), (F, n)


@pytest.mark.parametrize("n_points", [4, 258, 515])
def test_point_in_hull_of_sphere_points(eng, n_points):
    from icepy4d_amd.post_processing import triangle_mesh as TM
    hull = MC.sphere_points(n_points)
    facets = O.hull_facets(hull)
    assert len(facets) == 2 * n_points - 4                          # 4, 512 and 1026 facets: the LDS chunk and two chunks with a tail
    q = MC.hull_queries(facets, hull)
    want = O.point_in_hull(q, facets)
    assert 0 < want.sum() < len(q) and not want[~np.isfinite(q).all(1)].any()
    assert np.array_equal(TM.point_in_hull(q, hull, engine=eng), want) and np.array_equal(TM.point_in_hull(q, facets=facets, engine=eng), want)


# ---- TriangleMesh ---------------------------------------------------------------------------------------------------------------------------------
def as_mesh(TM, c, eng):
    return TM.TriangleMesh(c["vertices"], c["triangles"], c["colors"], c["normals"], {"density": np.arange(len(c["vertices"]), dtype=np.float64)}, engine=eng)


def mesh_equal(m, o, vlist, what):
    assert same(m.vertices, o.vertices) and equal(m.triangles, o.triangles), what
    assert (m.vertex_colors is None and o.vertex_colors is None) or same(m.vertex_colors, o.vertex_colors), what
    assert (m.vertex_normals is None and o.vertex_normals is None) or same(m.vertex_normals, o.vertex_normals), what
    assert np.array_equal(m.kept_vertices, vlist), what


@pytest.mark.parametrize("name", ["v0_t0", "v3_t1", "special", "special_plain", "fan_3", "fan_4", "fan_4_equal_areas", "two_fans", "strip_256", "strip_65537",
                                  "mask_keeps_nothing", "mask_keeps_all", "select_with_duplicates", "field_with_duplicates", "bad_triangles_between", "wrong_indices"])
def test_triangle_mesh_operations(eng, name):
    from icepy4d_amd.post_processing import triangle_mesh as TM
    c = MC.by_name(name)
    ops = [("remove_vertices_by_mask", (c["mask"],)), ("remove_degenerate_triangles", ()), ("remove_duplicated_triangles", ()), ("remove_duplicated_vertices", ()),
           ("remove_unreferenced_vertices", ()), ("remove_non_manifold_edges", ())]
    for op, args in ops:                                              # each on the case as it is
        m, o = as_mesh(TM, c, eng), MC.mesh_of(c)
        out, vlist, pos = getattr(o, op)(*args)
        assert getattr(m, op)(*args) is m
        mesh_equal(m, out, vlist, (name, op))
        assert np.array_equal(m.kept_triangles, pos) and np.array_equal(m.attributes["density"], vlist.astype(np.float64)), (name, op)
    m, o = as_mesh(TM, c, eng), MC.mesh_of(c)                         # and one after the other, as MeshingPoisson chains them
    assert m.count_non_manifold_edges() == O.edge_census(c["triangles"])
    origin = np.arange(len(c["vertices"]))
    for op, args in ops:
        o, vlist, _ = getattr(o, op)(*args)
        getattr(m, op)(*args)
        origin = origin[vlist]
        mesh_equal(m, o, vlist, (name, "chain", op))
        assert np.array_equal(m.attributes["density"], origin.astype(np.float64)), (name, "chain", op)
    for cleanup in (True, False):
        m, o = as_mesh(TM, c, eng), MC.mesh_of(c)
        out, vlist, pos = o.select_by_index(c["index"], cleanup)
        sel = m.select_by_index(c["index"], cleanup)
        assert sel is not m and len(m.vertices) == len(c["vertices"])
        mesh_equal(sel, out, vlist, (name, "select_by_index", cleanup))
    m = as_mesh(TM, c, eng)
    for N in c["samples"]:
        if O.areas(c["vertices"], c["triangles"]).sum() == 0 and N > 0:
            continue                                                  # the refusal: test_refusals_leave_the_outputs_untouched
        want = O.sample(c["vertices"], c["triangles"], N, c["seed"], c["colors"], c["normals"])
        pcd = m.sample_points_uniformly(N, seed=c["seed"])
        assert same(pcd.points, want["points"]) and same(pcd.normals, want["normals"]), (name, N)
        assert (pcd.colors is None and want["colors"] is None) or same(pcd.colors, want["colors"]), (name, N)


def test_box_mesh_through_every_operation(eng):
    import voxel_cases as VC
    from icepy4d_amd.post_processing import triangle_mesh as TM
    from icepy4d_amd.post_processing.voxel_grid import VoxelGrid
    case = VC.mesh_by_name("block_2x2x2")
    vg = VoxelGrid(case["grid"], {"grid_index": case["grid_index"], "counts": np.ones(len(case["grid_index"]), np.int32), "dropped": 0, "colors": case["colors"]}, eng)
    m = TM.TriangleMesh.from_arrays(*vg.to_box_mesh(), engine=eng)
    o = O.Mesh(m.vertices, m.triangles, m.vertex_colors)
    assert len(m.vertices) == 27 and len(m.triangles) == 96 and m.has_vertex_colors()
    mask = np.arange(27) == 13                                        # the centre vertex: the 8 cubes lose the triangles at it
    for op, args in (("remove_vertices_by_mask", (mask,)), ("remove_degenerate_triangles", ()), ("remove_duplicated_triangles", ()), ("remove_duplicated_vertices", ()),
                     ("remove_non_manifold_edges", ()), ("remove_unreferenced_vertices", ())):
        o, vlist, _ = getattr(o, op)(*args)
        getattr(m, op)(*args)
        mesh_equal(m, o, vlist, op)
    assert O.edge_census(o.triangles) == 0 and len(o.triangles) < 96        # the inner faces met four at an edge: the rounds thinned them
    inside = TM.point_in_hull(m.vertices, m.vertices, engine=eng)
    assert np.array_equal(inside, O.point_in_hull(m.vertices, O.hull_facets(m.vertices)))
    sel = m.filter_by_hull(m.vertices * 0.75 + m.vertices.mean(0) * 0.25)
    keep = O.point_in_hull(m.vertices, O.hull_facets(m.vertices * 0.75 + m.vertices.mean(0) * 0.25))
    out, vlist, _ = o.select_by_index(np.nonzero(keep)[0])
    mesh_equal(sel, out, vlist, "filter_by_hull")
    want = O.sample(m.vertices, m.triangles, 1000, 5, m.vertex_colors)
    pcd = m.sample_points_uniformly(1000, seed=5)
    assert same(pcd.points, want["points"]) and same(pcd.colors, want["colors"]) and same(pcd.normals, want["normals"])


# ---- wrong inputs stay inside ----------------------------------------------------------------------------------------------------------------------
def test_wrong_indices_stay_inside(eng):
    """Index validation (include/icematch.h): a triangle with an index outside [0, V) is SKIPPED where triangles are judged (dropped by
    im_mesh_select, area 0 in im_mesh_sample_table) and CLAMPED where a caller's table leads to it (im_mesh_sample); a permutation entry
    that is none is clamped. The figures are meaningless or defined as above; the bands around every output hold."""
    rng = np.random.default_rng(3)
    c = MC.by_name("wrong_indices")
    v, t = c["vertices"], c["triangles"]
    V, T = len(v), len(t)
    vmap, vlist, tout, pos = c_select(eng, "wrong triangles", V, t)
    assert pos.tolist() == [k for k in range(T) if not 10 <= k < 14] and len(vlist) == V
    wild = rng.integers(-2 ** 31, 2 ** 31, (300, 3)).astype(np.int32)
    for merge in (None, rng.integers(-5, V + 5, V).astype(np.int32), wild[:V, 0]):
        nv, nt = c_select(eng, "wild triangles", V, np.concatenate([wild, t]), merge=merge, unreferenced=1, check=False)
        assert 0 <= nv <= V and 0 <= nt <= T + 300
    area = c_sample(eng, "wild areas", v, np.concatenate([wild, t]), 100, 1)
    assert (area["area"][:300] == 0).all() and (area["triangle"] >= 300).all()
    # a table that is none: not ascending, too small, too large
    for table in (rng.integers(-50, 150, T), np.zeros(T, np.int64), np.full(T, 2 ** 62), np.arange(T)[::-1].copy()):
        got = c_sample(eng, "wrong table", v, t, 100, 1, c["colors"], table=table)
        assert got["points"].shape == (100, 3) and (got["triangle"] >= 0).all() and (got["triangle"] < T).all()
    keys = rng.integers(0, 50, 1000)
    assert c_census(eng, "unsorted keys", keys, sort=False) >= 0
    for perm in (rng.integers(0, 1000, 1000), rng.integers(-2 ** 40, 2 ** 40, 1000), np.zeros(1000, np.int64)):
        first, keep = c_first(eng, "wrong permutation", [keys, keys[::-1].copy()], perm=perm)
        assert first.shape == (1000,)                                 # entries no sorted position names stay pre-filled: meaningless, inside


# ---- the reference's chain (g20) through MeshingPoisson --------------------------------------------------------------------------------------------
def test_g20_through_meshing_poisson(eng, g20, tmp_path):
    from icepy4d_amd import meshing
    from icepy4d_amd.core import PointCloud
    from icepy4d_amd.core.point_cloud import read_ply
    from icepy4d_amd.post_processing import MeshingPoisson, read_triangle_mesh
    PointCloud(points3d=np.array(g20["points"])).write_ply(tmp_path / "dense_2022_05_01.ply")
    np.savetxt(tmp_path / "crop.poly", g20["polyline"], delimiter=" ")
    seen = []

    def reconstruct(points, normals, **kw):
        seen.append((len(points), normals is not None and len(normals) == len(points), kw))
        return g20["surface_vertices"], g20["surface_triangles"], g20["surface_density"]

    class Recording(MeshingPoisson):
        steps = {}

        def filter_mesh_by_density(self):
            for op, key in (("remove_vertices_by_mask", "by_mask"), ("remove_degenerate_triangles", "degenerate_triangles"),
                            ("remove_duplicated_triangles", "duplicated_triangles"), ("remove_duplicated_vertices", "duplicated_vertices"),
                            ("remove_non_manifold_edges", "non_manifold_edges")):
                inner = getattr(self.mesh, op)

                def wrapped(*a, _inner=inner, _key=key, **k):
                    r = _inner(*a, **k)
                    self.steps[_key] = (self.mesh.vertices.copy(), self.mesh.triangles.copy(), self.mesh.attributes["density"].copy())
                    return r
                setattr(self.mesh, op, wrapped)
            super().filter_mesh_by_density()

    cfg = {"num_sampled_points": 2000, "crop_polyline_path": str(tmp_path / "crop.poly")}
    m = Recording(tmp_path / "dense_2022_05_01.ply", tmp_path / "out", cfg, reconstruct=reconstruct, engine=eng)
    assert m.run() is True
    calls = dict((c[0], c[1]) for c in json.loads(g20["calls"].tobytes().decode()))
    want_kw = {k: calls["TriangleMesh.create_from_point_cloud_poisson"][k] for k in ("depth", "width", "scale", "linear_fit")}
    assert seen == [(len(g20["sor_ind"]), True, want_kw)] and same(m.pcd.points, g20["points"][g20["sor_ind"]])
    assert same(m.convex_hull, g20["hull_vertices"])
    surface, density = g20["surface_vertices"], g20["surface_density"]
    for key, (vert, tri, dens) in m.steps.items():
        origin = g20[key + "_vertices"]
        assert same(vert, surface[origin]) and equal(tri, g20[key + "_triangles"]) and same(dens, density[origin]), key
    assert sorted(m.steps) == sorted(["by_mask", "degenerate_triangles", "duplicated_triangles", "duplicated_vertices", "non_manifold_edges"])
    origin = g20["by_hull_vertices"]
    assert same(m.mesh.vertices, surface[origin]) and equal(m.mesh.triangles, g20["by_hull_triangles"]) and same(m.density, density[origin])
    assert same(m.sampled_pcd.points, g20["cropped_points"]) and same(m.sampled_pcd.normals, g20["cropped_normals"])
    assert sorted(f.name for f in (tmp_path / "out").iterdir()) == json.loads(g20["files"].tobytes().decode())
    assert list(m.timer.times.keys()) == json.loads(g20["timer_labels"].tobytes().decode())
    pts, _, nrm = read_ply(tmp_path / "out" / "sampled_2022_05_01.ply")
    assert same(pts, g20["cropped_points"]) and same(nrm, g20["cropped_normals"])
    back = read_triangle_mesh(tmp_path / "out" / "mesh_2022_05_01.ply")
    assert same(back.vertices, m.mesh.vertices) and equal(back.triangles, m.mesh.triangles) and same(back.attributes["density"], m.density)
    # the other route: the saved surface as cfg["mesh_path"]; and mesh_series, which leaves the sampled cloud where dod_series looks for it
    from icepy4d_amd.post_processing.triangle_mesh import TriangleMesh, write_mesh
    write_mesh(tmp_path / "surface.ply", TriangleMesh(surface, g20["surface_triangles"], attributes={"density": density}))
    out = meshing.mesh_series([tmp_path / "dense_2022_05_01.ply"], tmp_path / "series", {**cfg, "mesh_path": str(tmp_path / "surface.ply"), "do_SOR": True,
                                                                                       "min_mesh_denisty": 11}, engine=eng)
    assert out == [tmp_path / "series" / "sampled_2022_05_01.ply"] and same(read_ply(out[0])[0], g20["cropped_points"])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(eng):
    c = MC.by_name("strip_256")
    v, t = c["vertices"], c["triangles"]
    V, T = len(v), len(t)
    d_v, d_t = dev(eng, v), dev(eng, t, np.int32)
    st = eng.stream_ptr()
    big = 2 ** 26 + 1
    outs = [Framed(eng, (V,), np.int32), Framed(eng, (V,), np.int32), Framed(eng, (T, 3), np.int32), Framed(eng, (T,), np.int32), Framed(eng, (2,), np.int64)]
    o = [f.ptr for f in outs]
    sel = lambda V_=V, T_=T, tri=p(d_t), out=o: raw(eng, "im_mesh_select", None, V_, tri, T_, None, None, 0, 0, out[0], out[1], out[2], out[3], out[4], st)
    assert [sel(V_=-1), sel(T_=-1), sel(V_=big), sel(T_=big), sel(tri=None), sel(out=o[:4] + [None]), sel(out=[None] + o[1:]), sel(out=o[:2] + [None] + o[3:])] == [REFUSED] * 8
    k = [Framed(eng, (3 * T,), np.int64) for _ in range(3)]
    assert raw(eng, "im_mesh_triangle_keys", p(d_t), -1, k[0].ptr, k[1].ptr, st) == REFUSED and raw(eng, "im_mesh_triangle_keys", p(d_t), T, k[0].ptr, None, st) == REFUSED
    assert raw(eng, "im_mesh_triangle_keys", None, T, k[0].ptr, k[1].ptr, st) == REFUSED and raw(eng, "im_mesh_triangle_keys", p(d_t), big, k[0].ptr, k[1].ptr, st) == REFUSED
    assert raw(eng, "im_mesh_vertex_keys", p(d_v), V, k[0].ptr, k[1].ptr, None, st) == REFUSED and raw(eng, "im_mesh_vertex_keys", None, V, k[0].ptr, k[1].ptr, k[2].ptr, st) == REFUSED
    assert raw(eng, "im_mesh_vertex_keys", p(d_v), -1, k[0].ptr, k[1].ptr, k[2].ptr, st) == REFUSED and raw(eng, "im_mesh_vertex_keys", p(d_v), big, k[0].ptr, k[1].ptr, k[2].ptr, st) == REFUSED
    assert raw(eng, "im_mesh_edge_keys", p(d_t), -1, k[0].ptr, st) == REFUSED and raw(eng, "im_mesh_edge_keys", None, T, k[0].ptr, st) == REFUSED
    assert raw(eng, "im_mesh_edge_keys", p(d_t), T, None, st) == REFUSED and raw(eng, "im_mesh_edge_keys", p(d_t), big, k[0].ptr, st) == REFUSED
    d_k = dev(eng, np.arange(T), np.int64)
    first, keep = Framed(eng, (T,), np.int32), Framed(eng, (T,), np.uint8)
    seg = lambda n=T, k0=p(d_k), k1=None, k2=None, perm=p(d_k): raw(eng, "im_mesh_first_of_segment", n, k0, k1, k2, perm, first.ptr, keep.ptr, st)
    assert [seg(n=-1), seg(n=big), seg(k0=None), seg(perm=None), seg(k2=p(d_k))] == [REFUSED] * 5
    count = Framed(eng, (1,), np.int64)
    assert raw(eng, "im_mesh_edge_census", p(d_k), -1, count.ptr, st) == REFUSED and raw(eng, "im_mesh_edge_census", None, T, count.ptr, st) == REFUSED
    assert raw(eng, "im_mesh_edge_census", p(d_k), T, None, st) == REFUSED and raw(eng, "im_mesh_edge_census", p(d_k), 3 * 2 ** 26 + 1, count.ptr, st) == REFUSED
    inside = Framed(eng, (V,), np.uint8)
    good = MC.tangent_facets(8)
    hull = lambda n=V, pts=p(d_v), f=good, F=8, out=inside.ptr: raw(eng, "im_mesh_in_hull", pts, n, None if f is None else f.ctypes.data, F, out, st)
    bad_nan, bad_inf = good.copy(), good.copy()
    bad_nan[7, 3], bad_inf[0, 0] = np.nan, np.inf
    assert [hull(n=-1), hull(n=big), hull(pts=None), hull(f=None), hull(F=0), hull(F=-3), hull(F=2 ** 22 + 1), hull(f=bad_nan), hull(f=bad_inf), hull(out=None)] == [REFUSED] * 10
    end, area, pts = Framed(eng, (T,), np.int64), Framed(eng, (T,), np.float64), Framed(eng, (64, 3), np.float64)
    total = np.full(1, -7, np.int64)
    tab = lambda V_=V, T_=T, N=64, vert=p(d_v), tri=p(d_t), out=end.ptr: raw(eng, "im_mesh_sample_table", vert, V_, tri, T_, N, area.ptr, out, total.ctypes.data, st)
    flat = dev(eng, np.zeros((V, 3)))                                 # every triangle has area 0: C == 0
    assert [tab(V_=-1), tab(T_=-1), tab(N=-1), tab(V_=big), tab(T_=big), tab(N=big), tab(vert=None), tab(tri=None), tab(out=None), tab(T_=0), tab(vert=p(flat))] == [REFUSED] * 11
    assert total[0] == -7 and tab(vert=p(flat), N=0) == 0 and total[0] == 0
    eng.synchronize()
    assert (end.result("C == 0 and N == 0") == 0).all() and (area.result("C == 0 and N == 0") == 0).all()
    end, area = Framed(eng, (T,), np.int64), Framed(eng, (T,), np.float64)
    d_end = dev(eng, O.sample_table(O.areas(v, t), 64)[3], np.int64)
    smp = lambda V_=V, T_=T, N=64, vert=p(d_v), tri=p(d_t), table=p(d_end), out=pts.ptr: raw(eng, "im_mesh_sample", vert, V_, tri, T_, table, N, 0, None, None, out, None, None, None, st)
    assert [smp(V_=-1), smp(T_=-1), smp(N=-1), smp(V_=big), smp(T_=big), smp(N=big), smp(V_=0), smp(T_=0), smp(vert=None), smp(tri=None), smp(table=None), smp(out=None)] == [REFUSED] * 12
    eng.synchronize()
    for f in outs + k + [first, keep, count, inside, end, area, pts]:
        f.untouched("a refused call wrote an output")
    assert "im_mesh_sample" in eng.ctx.lib.im_last_error(eng.ctx.h).decode()
    # zero-size calls return 0 and launch nothing
    assert sel(V_=0, T_=0) == 0 and seg(n=0) == 0 and hull(n=0) == 0 and smp(N=0) == 0 and raw(eng, "im_mesh_edge_census", None, 0, count.ptr, st) == 0
    eng.synchronize()
    assert outs[4].result("counts").tolist() == [0, 0] and count.result("census").tolist() == [0]
    for f in outs[:4] + [first, keep, inside, pts]:
        f.untouched("a zero-size call wrote an output")
