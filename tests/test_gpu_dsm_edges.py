"""The DSM and orthophoto kernels (csrc/dsm.hip, csrc/dsm_cell.h) through the C ABI, at every boundary between two code paths
(tests/dsm_cases.py: cloud sizes and group counts around the scan's block of 256 and around 256 blocks, ties at half a step, signed zero
keys, NaN and infinite z; triangle lists around the scan's block and beyond 65 536, empty triangles at the start, the end and in runs,
degenerate, overlapping and identical triangles, horizontal edges, margin rows, more spans than the raster kernel's grid covers at once,
grids of one row and one column; every position a projection can take against the image, every distortion length, every channel
count), and the public layer on lattice clouds.

Bounds. Equality of bits with the restatement (tests/dsm_oracle.py: `bin_points`, `rasterize`, `project_colors`, `ortho_bytes`) on every
element and every cell of every case: no cell is exempt and none is left out. Derived, not measured: the kernels and the restatement
perform the same IEEE float64 / float32 operations in the same order with contraction off; float32 and float64 division are correctly
rounded on the device and the library is built without a fast-math flag; the triangle of a cell is the lowest index that contains it,
kept by an integer atomicMin, so it does not depend on the order in which spans run; the sorts of the binning are stable sorts of integer
keys. That holds for the binned x / y / z, every grid, the projections and the orthophoto bytes, NaNs with their sign and payload
included. The float64 colours are the one exception: IEEE 754 leaves the sign of a NaN result open, and the colours of an item whose
projection is NaN or infinite come out of the device with the other sign than numpy's (a NaN that passes through `x1 - u`), so for the
colours alone a NaN on both sides counts as equal and every other element is compared by its bits. The host build of the same
text agrees with the restatement on the same lists (tests/test_dsm_cpu.py); what only this file can show is the scans, the binary search
over the span offsets, the grid-stride loop, the scratch reuse and a lost `#pragma clang fp contract(off)`: gfx950 has fused multiply-add.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched, and so must every byte the call has no business writing (rows beyond the group count, cells with a NaN z, outputs
of a refused or empty call)."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dsm_cases as DC  # noqa: E402
import dsm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -72
WIN_NONE = 0x7F7F7F7F
INF, NAN = float("inf"), float("nan")


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
    return torch.from_numpy(np.array(a, order="C")).to(eng.device)          # a copy: the shared inputs are read-only


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

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        return host[BAND:BAND + self.n].view(self.dtype).reshape(self.shape)

    def untouched(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all() and (host[BAND:BAND + self.n] == FILL).all(), what


def prefilled(a):
    return (np.ascontiguousarray(a).view(np.uint8) == FILL).all()


# ---- binning ---------------------------------------------------------------------------------------------------------------------------
def round_outputs(eng, n):
    return [Framed(eng, (n,), t) for t in (np.float32, np.float32, np.int64, np.int64, np.int64)]


def mean_outputs(eng, n):
    return [Framed(eng, (n,), np.float32) for _ in range(3)] + [Framed(eng, (1,), np.int64)]


def device_bin(eng, points, step, what):
    """`im_dsm_round`, torch's three stable sorts (as `_bin_on_device`), `im_dsm_group_mean`: (bx, by, bz) of the groups, (xr, yr)."""
    import torch
    n, st = len(points), eng.stream_ptr()
    d_pts = dev(eng, points)
    ro = round_outputs(eng, n)
    eng.ctx.call("im_dsm_round", p(d_pts), n, float(np.float32(step)), *[f.ptr for f in ro], st)
    xr, yr, xykey, ykey, zkey = (f.result((what, "round")) for f in ro)
    d_xykey, d_ykey, d_zkey = dev(eng, xykey), dev(eng, ykey), dev(eng, zkey)
    pa = torch.sort(d_ykey, stable=True).indices
    pb = pa[torch.sort(d_zkey[pa], stable=True).indices].contiguous()
    pc = pb[torch.sort(d_xykey[pb], stable=True).indices].contiguous()
    mo = mean_outputs(eng, n)
    eng.ctx.call("im_dsm_group_mean", p(d_pts), ro[0].ptr, ro[1].ptr, ro[2].ptr, p(pb), p(pc), n, *[f.ptr for f in mo], st)
    bx, by, bz, ng = (f.result((what, "group mean")) for f in mo)
    G = int(ng[0])
    assert 0 < G <= n and prefilled(bx[G:]) and prefilled(by[G:]) and prefilled(bz[G:]), (what, "rows beyond the groups were written")
    return (bx[:G], by[:G], bz[:G]), (xr, yr)


@pytest.mark.parametrize("name", DC.binning_names())
def test_binning_equals_the_oracle_bit_for_bit(eng, name):
    c = DC.binning_case(name)
    (bx, by, bz), (xr, yr) = device_bin(eng, c["points"], c["step"], name)
    assert O.bits_equal(xr, O.round_to_step(c["points"][:, 0], c["step"])) and O.bits_equal(yr, O.round_to_step(c["points"][:, 1], c["step"]))
    wx, wy, wz = DC.binned(name)
    assert len(bx) == len(wx), (len(bx), len(wx))
    assert O.bits_equal(bx, wx) and O.bits_equal(by, wy) and O.bits_equal(bz, wz)


def test_binning_after_a_larger_cloud(eng):
    """The scratch grows for 65 537 points and is reused by 2: nothing of the larger call shows in the smaller one, or in its repeat."""
    for name in ("n65537", "n2", "n65537", "zero_key_x_neg_first"):
        c = DC.binning_case(name)
        got = device_bin(eng, c["points"], c["step"], name)[0]
        assert all(O.bits_equal(g, w) for g, w in zip(got, DC.binned(name))), name


# ---- raster ----------------------------------------------------------------------------------------------------------------------------
class Raster:
    """A raster case on the device."""

    def __init__(self, eng, c):
        self.c, self.eng = c, eng
        self.d = {k: dev(eng, c[k]) for k in ("bx", "by", "bz", "simplices", "transform", "xq", "yq")}
        self.nx, self.ny = len(c["xq"]), len(c["yq"])

    def args(self, out_ptr, **over):
        c, d = self.c, self.d
        a = {"bx": p(d["bx"]), "by": p(d["by"]), "bz": p(d["bz"]), "simplices": p(d["simplices"]), "transform": p(d["transform"]),
             "T": len(c["simplices"]), "bounds": c["bounds"].ctypes.data, "xq": p(d["xq"]), "nx": self.nx, "yq": p(d["yq"]), "ny": self.ny,
             "x0": float(c["xq"][0]), "dx": abs(c["step"]), "y0": float(c["yq"][0]), "dy": abs(c["step"]), "fill": c["fill"], "z": out_ptr}
        a.update(over)
        return list(a.values()) + [self.eng.stream_ptr()]

    def run(self, what):
        z = Framed(self.eng, (self.ny, self.nx), np.float64)
        self.eng.ctx.call("im_dsm_rasterize", *self.args(z.ptr))
        return z.result(what)


def differing(z, want):
    return int((np.ascontiguousarray(z).view(np.uint64) != np.ascontiguousarray(want).view(np.uint64)).sum())


@pytest.mark.parametrize("name", DC.raster_names())
def test_raster_equals_the_oracle_on_every_cell(eng, name):
    c = DC.raster_case(name)
    r = Raster(eng, c)
    want = DC.raster_expected(name)
    for turn in (0, 1):
        z = r.run((name, turn))
        assert O.bits_equal(z, want), (name, turn, differing(z, want), z.size)


def test_raster_stride_loop_on_this_device(eng):
    """More spans than the raster kernel's 16 x CUs blocks of 256 threads cover at once, built for this device's CU count. The triangles
    that reach the grid's columns are listed last, so every cell is won by a span numbered 16 * 256 * CUs or higher, which only a thread
    in its second turn of the grid-stride loop reaches (about 50 000 threads at 256 CUs): without that turn every cell would be fill."""
    import torch
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    c = DC.stride_case(cus)
    beyond, inside = DC.second_turn_cells(c, cus)
    assert DC.spans_of(c) > 16 * 256 * cus and beyond == inside == len(c["xq"]) * len(c["yq"])
    want = DC.rasterized(c)
    z = Raster(eng, c).run(c["name"])
    assert not np.isnan(want).any() and O.bits_equal(z, want), differing(z, want)


def test_raster_large_then_small_then_large(eng):
    """One context: the scratch grows for the large case, the small one reuses it (a stale winner would show), the large one again."""
    names = ("lattice_step_025", "grid_1x1", "lattice_step_025", "xlim_outside", "strip_65537_far_end", "zoo", "lattice_step_025")
    rasters = {n: Raster(eng, DC.raster_case(n)) for n in set(names)}
    for turn, n in enumerate(names):
        z = rasters[n].run((n, turn))
        assert O.bits_equal(z, DC.raster_expected(n)), (n, turn, differing(z, DC.raster_expected(n)))


# ---- colours ---------------------------------------------------------------------------------------------------------------------------
class Colours:
    """A colour case on the device: as a cloud of points, as a grid of cells with dense planes, and with the axes' own strides."""

    def __init__(self, eng, c):
        self.c, self.eng = c, eng
        self.rows, self.cols = c["z"].shape
        self.n = self.rows * self.cols
        gx, gy = np.meshgrid(c["xq"], c["yq"])
        self.pts, self.gx, self.gy, self.z = dev(eng, DC.colour_points(c)), dev(eng, gx), dev(eng, gy), dev(eng, c["z"])
        self.xq, self.yq, self.img = dev(eng, c["xq"]), dev(eng, c["yq"]), dev(eng, c["image"])

    def planes(self, mode):
        if mode == "points":
            b = p(self.pts)
            return [b, 0, 3, b + 8, 0, 3, b + 16, 0, 3, 1, self.n, 0]
        if mode == "dense":
            return [p(self.gx), self.cols, 1, p(self.gy), self.cols, 1, p(self.z), self.cols, 1, self.rows, self.cols, 1]
        return [p(self.xq), 0, 1, p(self.yq), 1, 0, p(self.z), self.cols, 1, self.rows, self.cols, 1]

    def run(self, mode, chmap, ask=("proj", "col", "ortho")):
        cout, im = len(chmap), self.c["image"]
        out = {"proj": Framed(self.eng, (self.n, 2), np.float32), "col": Framed(self.eng, (self.n, cout), np.float64),
               "ortho": Framed(self.eng, (self.n, 3), np.uint8)}
        ask = [a for a in ask if a != "ortho" or cout == 3]
        self.eng.ctx.call("im_project_colors", *self.planes(mode), self.c["cam"].ctypes.data, p(self.img), im.shape[0], im.shape[1], im.shape[2],
                          chmap.ctypes.data, cout, *[out[k].ptr if k in ask else None for k in ("proj", "col", "ortho")], self.eng.stream_ptr())
        for k in out:
            if k not in ask:
                out[k].untouched((self.c["name"], mode, k, "not asked for"))
        return {k: out[k].result((self.c["name"], mode, k)) for k in ask}


def check_colours(got, want, z, cells, what):
    """The outputs asked for against the oracle's; in cell mode the items with a NaN z keep their pre-fill in proj and col and are black."""
    live = ~np.isnan(z.ravel()) if cells else np.ones(z.size, bool)
    for k, w in zip(("proj", "col"), want[:2]):
        if k in got:
            # col alone: a NaN equals a NaN. Measured on an MI355X: the colours of an item whose projection is NaN or infinite come out
            # as 0xfff8... where numpy has 0x7ff8... (and the reverse), the sign of a NaN that passes through `x1 - u`; nothing else differs
            assert (O.same_bits if k == "col" else O.bits_equal)(got[k][live], w[live]), (what, k)
            assert prefilled(got[k][~live]), (what, k, "an item with a NaN z was written")
    if "ortho" in got:
        assert np.array_equal(got["ortho"], want[2]), (what, "ortho", int((got["ortho"] != want[2]).sum()))


@pytest.mark.parametrize("name", DC.colour_names())
def test_colours_equal_the_oracle_bit_for_bit(eng, name):
    c = DC.colour_case(name)
    dc = Colours(eng, c)
    for k, chmap in enumerate(c["chmaps"]):
        want = DC.colour_expected(name, k)
        for mode in ("points", "dense", "broadcast"):
            check_colours(dc.run(mode, chmap), want, c["z"], mode != "points", (name, k, mode))


@pytest.mark.parametrize("name", ["camera_d5", "probe_cin3", "one_cell_nan_z"])
def test_each_optional_output_alone(eng, name):
    """proj, col and ortho are each requested alone. With one cell, a NaN z and proj requested, the proj row stays at its pre-fill."""
    c = DC.colour_case(name)
    dc = Colours(eng, c)
    want = DC.colour_expected(name, 0)
    for mode in ("points", "broadcast"):
        for ask in (("proj",), ("col",), ("ortho",), ("proj", "ortho"), ("col", "ortho")):
            got = dc.run(mode, c["chmaps"][0], ask)
            assert set(got) == set(ask)
            check_colours(got, want, c["z"], mode != "points", (name, mode, ask))
    if name == "one_cell_nan_z":
        got = dc.run("dense", c["chmaps"][0], ("proj",))
        assert prefilled(got["proj"])


# ---- refusals and empty inputs ---------------------------------------------------------------------------------------------------------------
def refused(eng, name, *args):
    from icepy4d_amd._lib import IcematchError
    with pytest.raises(IcematchError) as e:
        eng.ctx.call(name, *args)
    assert e.value.rc == REFUSED, (name, e.value)


def test_refusals_leave_the_outputs_alone(eng):
    st = eng.stream_ptr()
    c = DC.binning_case("n257")
    n = len(c["points"])
    d_pts = dev(eng, c["points"])
    ro = round_outputs(eng, n)
    o = [f.ptr for f in ro]
    bad = {f"null {k}": (p(d_pts), n, 0.5, *[None if j == k else v for j, v in enumerate(o)]) for k in range(5)}
    bad.update({"null points": (None, n, 0.5, *o), "n < 0": (p(d_pts), -1, 0.5, *o), "n = 2^31 - 1": (p(d_pts), 2 ** 31 - 1, 0.5, *o),
                "step 0": (p(d_pts), n, 0.0, *o), "step -0": (p(d_pts), n, -0.0, *o), "step inf": (p(d_pts), n, INF, *o),
                "step -inf": (p(d_pts), n, -INF, *o), "step nan": (p(d_pts), n, NAN, *o)})
    for what, args in bad.items():
        refused(eng, "im_dsm_round", *args, st)
        for f in ro:
            f.untouched(("im_dsm_round", what))
    eng.ctx.call("im_dsm_round", p(d_pts), n, 0.5, *o, st)
    perm = dev(eng, np.arange(n, dtype=np.int64))
    mo = mean_outputs(eng, n)
    m = [f.ptr for f in mo]
    good = [p(d_pts), o[0], o[1], o[2], p(perm), p(perm)]
    bad = {f"null input {k}": (*[None if j == k else v for j, v in enumerate(good)], n, *m) for k in range(6)}
    bad.update({f"null output {k}": (*good, n, *[None if j == k else v for j, v in enumerate(m)]) for k in range(4)})
    bad.update({"n < 0": (*good, -1, *m), "n = 2^31 - 1": (*good, 2 ** 31 - 1, *m)})
    for what, args in bad.items():
        refused(eng, "im_dsm_group_mean", *args, st)
        for f in mo:
            f.untouched(("im_dsm_group_mean", what))

    r = Raster(eng, DC.raster_case("zoo"))
    z = Framed(eng, (r.ny, r.nx), np.float64)
    bad = {f"null {k}": {k: None} for k in ("bx", "by", "bz", "simplices", "transform", "bounds", "xq", "yq", "z")}
    bad.update({"T < 0": {"T": -1}, "T = 2^31 - 1": {"T": 2 ** 31 - 1}, "T = the no-triangle mark": {"T": WIN_NONE}, "T above it": {"T": WIN_NONE + 1},
                "nx < 0": {"nx": -1}, "ny < 0": {"ny": -1}, "dx = 0": {"dx": 0.0}, "dx < 0": {"dx": -0.5}, "dx nan": {"dx": NAN}, "dy = 0": {"dy": 0.0},
                "dy < 0": {"dy": -0.5}, "dy nan": {"dy": NAN}, "x0 inf": {"x0": INF}, "x0 nan": {"x0": NAN}, "y0 -inf": {"y0": -INF}, "y0 nan": {"y0": NAN}})
    for what, over in bad.items():
        args = r.args(z.ptr, **over)
        refused(eng, "im_dsm_rasterize", *args)
        z.untouched(("im_dsm_rasterize", what))

    c = DC.colour_case("camera_d5")
    dc = Colours(eng, c)
    im, cam = c["image"], c["cam"].ctypes.data
    out = {"proj": Framed(eng, (dc.n, 2), np.float32), "col": Framed(eng, (dc.n, 4), np.float64), "ortho": Framed(eng, (dc.n, 3), np.uint8)}
    P, C, Og = out["proj"].ptr, out["col"].ptr, out["ortho"].ptr
    rgb, one, far, neg = (np.array(v, np.int32) for v in ([2, 1, 0], [0, 0, 0, 0, 0], [0, 3, 1], [0, -1, 1]))
    h, w, cin = im.shape
    pl = dc.planes("dense")

    def image(h=h, w=w, cin=cin, img=p(dc.img), chmap=rgb, cout=3):
        return [img, h, w, cin, None if chmap is None else chmap.ctypes.data, cout]

    bad = {"null x": ([None] + pl[1:], cam, image(), P, C, Og), "null y": (pl[:3] + [None] + pl[4:], cam, image(), P, C, Og),
           "null z": (pl[:6] + [None] + pl[7:], cam, image(), P, C, Og), "null camera": (pl, None, image(), P, C, Og),
           "rows < 0": (pl[:9] + [-1, dc.cols, 1], cam, image(), P, C, Og), "cols < 0": (pl[:9] + [dc.rows, -1, 1], cam, image(), P, C, Og),
           "cout 0": (pl, cam, image(cout=0), P, C, None), "cout 5": (pl, cam, image(chmap=one, cout=5), P, C, None),
           "cout 0, ortho": (pl, cam, image(cout=0), P, None, Og), "cout 5, proj alone": (pl, cam, image(chmap=one, cout=5), P, None, None),
           "cout -1, proj alone": (pl, cam, image(cout=-1), P, None, None), "cout 5, nothing asked": (pl, cam, image(chmap=one, cout=5), None, None, None),
           "ortho with 1 channel": (pl, cam, image(cout=1), P, None, Og), "ortho with 2 channels": (pl, cam, image(cout=2), P, C, Og),
           "ortho with 4 channels": (pl, cam, image(chmap=one, cout=4), P, C, Og),
           "channel map beyond cin": (pl, cam, image(chmap=far), P, C, Og), "channel map negative": (pl, cam, image(chmap=neg), None, C, None),
           "no image, col": (pl, cam, image(img=None), P, C, None), "no image, ortho": (pl, cam, image(img=None), None, None, Og),
           "no channel map": (pl, cam, image(chmap=None), P, C, None), "h = 0": (pl, cam, image(h=0), P, C, Og), "w = 0": (pl, cam, image(w=0), P, C, Og),
           "cin = 0": (pl, cam, image(cin=0), P, C, Og), "w < 0": (pl, cam, image(w=-3), None, None, Og)}
    for what, (planes, cam_ptr, img_args, a, b, o3) in bad.items():
        refused(eng, "im_project_colors", *planes, cam_ptr, *img_args, a, b, o3, st)
        for f in out.values():
            f.untouched(("im_project_colors", what))


def test_empty_inputs_touch_nothing_but_the_group_count(eng):
    st = eng.stream_ptr()
    c = DC.binning_case("n257")
    d_pts = dev(eng, c["points"])
    ro, mo = round_outputs(eng, 4), mean_outputs(eng, 4)
    eng.ctx.call("im_dsm_round", p(d_pts), 0, 0.5, *[f.ptr for f in ro], st)
    for f in ro:
        f.untouched("im_dsm_round, n == 0")
    perm = dev(eng, np.arange(4, dtype=np.int64))
    eng.ctx.call("im_dsm_group_mean", p(d_pts), ro[0].ptr, ro[1].ptr, ro[2].ptr, p(perm), p(perm), 0, *[f.ptr for f in mo], st)
    for f in mo[:3]:
        f.untouched("im_dsm_group_mean, n == 0")
    assert mo[3].result("n_groups")[0] == 0
    r = Raster(eng, DC.raster_case("zoo"))
    z = Framed(eng, (r.ny, r.nx), np.float64)
    for over in ({"nx": 0}, {"ny": 0}, {"nx": 0, "ny": 0}):
        eng.ctx.call("im_dsm_rasterize", *r.args(z.ptr, **over))
        z.untouched(("im_dsm_rasterize", over))
    zero = Raster(eng, dict(DC.raster_case("zoo"), fill=-9999.0))              # no triangle at all: every cell is the fill value
    zz = Framed(eng, (zero.ny, zero.nx), np.float64)
    eng.ctx.call("im_dsm_rasterize", *zero.args(zz.ptr, T=0))
    assert (zz.result("T == 0") == -9999.0).all()
    dc = Colours(eng, DC.colour_case("camera_d5"))
    c = dc.c
    out = [Framed(eng, (dc.n, 2), np.float32), Framed(eng, (dc.n, 3), np.float64), Framed(eng, (dc.n, 3), np.uint8)]
    pl = dc.planes("dense")
    for rows, cols in ((0, dc.cols), (dc.rows, 0), (0, 0)):
        eng.ctx.call("im_project_colors", *pl[:9], rows, cols, 1, c["cam"].ctypes.data, p(dc.img), *c["image"].shape, c["chmaps"][0].ctypes.data, 3,
                     *[f.ptr for f in out], st)
        for f in out:
            f.untouched(("im_project_colors", rows, cols))


# ---- the public layer ------------------------------------------------------------------------------------------------------------------------
def oracle_dsm(points, step, xlim=None, ylim=None, fill=np.nan):
    bx, by, bz = O.bin_points(points, step)
    tri = O.triangulate(bx, by)
    dx, dy = O.default_limits(points)
    xq, yq = O.grid_axes(dx if xlim is None else xlim, dy if ylim is None else ylim, step)
    z = O.rasterize(bx, by, bz, tri.simplices, tri.transform, np.r_[tri.min_bound, tri.max_bound], xq, yq, O.fill_of(fill, bz))
    return xq, yq, z


@pytest.mark.parametrize("name", list(DC.LATTICE))
def test_build_dsm_equals_rasterize_on_every_cell(eng, name):
    from icepy4d_amd.utils.dsm_orthophoto import build_dsm
    n, seed, step = DC.LATTICE[name]
    d = build_dsm(DC.lattice_cloud(n, seed), dsm_step=step, engine=eng)
    want = DC.raster_expected(name)
    assert d.z.dtype == np.float64 and O.bits_equal(d.z, want), differing(d.z, want)


def test_build_dsm_fills_and_grids(eng):
    from icepy4d_amd.utils.dsm_orthophoto import build_dsm
    pts = np.r_[DC.lattice_cloud(300, 8), [[20.0, 20.0, np.nan]]]                  # a bin of its own whose only z is NaN: the mean is NaN
    assert np.isnan(O.bin_points(pts, 1.0)[2]).any()
    cases = {"mean with a NaN bin": dict(fill="mean"), "mean": dict(fill="mean", pts=DC.lattice_cloud(60, 9)[np.isfinite(DC.lattice_cloud(60, 9)[:, 2])]),
             "wholly outside": dict(xlim=[100.0, 104.0], fill=-9999.0), "1 x 1": dict(xlim=[3.0, 4.0], ylim=[5.0, 6.0]),
             "empty": dict(xlim=[3.0, 3.0]), "a number": dict(fill=0.0)}
    for what, k in cases.items():
        q = k.get("pts", pts)
        xq, yq, want = oracle_dsm(q, 1.0, k.get("xlim"), k.get("ylim"), k.get("fill", np.nan))
        d = build_dsm(q, dsm_step=1.0, xlim=k.get("xlim"), ylim=k.get("ylim"), fill_value=k.get("fill", np.nan), engine=eng)
        assert d.z.shape == want.shape == (len(yq), len(xq)) and O.bits_equal(np.ascontiguousarray(d.z), want), what
    assert oracle_dsm(pts, 1.0, [3.0, 4.0], [5.0, 6.0])[2].shape == (1, 1) and oracle_dsm(pts, 1.0, [3.0, 3.0])[2].size == 0
    assert (oracle_dsm(pts, 1.0, [100.0, 104.0], None, -9999.0)[2] == -9999.0).all() and np.isnan(O.fill_of("mean", O.bin_points(pts, 1.0)[2]))


def test_orthophoto_from_a_device_dsm_and_from_a_plain_one(eng):
    from icepy4d_amd.utils.dsm_orthophoto import DSM, _DeviceDSM, build_dsm, generate_ortophoto
    n, seed, step = DC.LATTICE["lattice_step_05"]
    d = build_dsm(DC.lattice_cloud(n, seed), dsm_step=step, engine=eng)
    assert isinstance(d, _DeviceDSM) and np.isnan(d.z).any()
    cam = types.SimpleNamespace(K=np.array([[70.0, 0.0, 31.5], [0.0, 72.0, 23.25], [0.0, 0.0, 1.0]]), dist=np.array([-0.1, 0.02, 1e-3, -1e-3, 0.005]),
                                R=np.eye(3), t=np.array([-6.2, -5.9, 9.0]))
    image = DC.image_bytes(48, 64, 3, 70)
    plain = DSM(d.x.copy(), d.y.copy(), np.array(d.z), step)
    a = generate_ortophoto(image, d, cam, engine=eng)
    b = generate_ortophoto(image, plain, cam, engine=eng)
    want = O.orthophoto(plain.x, plain.y, plain.z, image, cam.K, cam.dist, cam.R, cam.t)
    assert a.dtype == np.uint8 and a.shape == want.shape and (want > 0).any() and (want == 0).all(axis=2).any()
    assert np.array_equal(a, b) and np.array_equal(a, want), (int((a != b).sum()), int((a != want).sum()))
