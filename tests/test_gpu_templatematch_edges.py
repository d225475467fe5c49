"""The template-matching kernels (csrc/templatematch.hip, arithmetic in csrc/tm_pair.h) on the device through the C ABI, on every case of
tests/tm_cases.py: the smallest shapes at every boundary between two code paths of the plan, the window rule at every edge, exact ties of
the maximum, peaks on and near the border of C, a flat image, and windows that hold a NaN or an infinity.

Bound: equality of bits with the numpy restatement (tests/tm_oracle.py), a NaN equal to a NaN: every element of C of every valid pair
(`im_template_match_corr`), all six outputs of every pair (`im_template_match_oc`), every value of `im_forient`. No point is exempt.
Derived, not measured: C is defined by the order of its float32 fused multiply-adds and of the additions of its partial sums
(tm_pair.h), a fused multiply-add and an addition are correctly rounded on the device, and the restatement emulates the fused
multiply-add exactly (tests/test_templatematch_host_cpu.py compares it with the C library's); the sum of |C| is a fixed tree of float64
additions; the tail runs with contraction off; float32 and float64 division and the float64 square root are correctly rounded in the
library's build. forient: the squares of float32 values are exact in float64, so fusing their sum changes nothing, the root and the two
quotients are rounded once, and oc_oracle.forient performs the same three operations: its bits are the kernel's.

Batches: `im_template_match_oc` splits a call into batches of 64 Mi / R^2 pairs, so a second batch (pair0 > 0) needs more than 64 Mi
pairs at R = 1 and cannot be made small; it stays with test_gpu_templatematch.py::test_many_pairs_several_images_deterministic (8910
pairs in batches of 7281). `im_template_match_corr` has no batches.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oc_oracle  # noqa: E402
import tm_cases as TC  # noqa: E402
import tm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -72
F32 = np.float32


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


def interleaved(m):
    return np.ascontiguousarray(np.stack([m.real, m.imag], -1), F32)


class Framed:
    """An output of `nbytes` between two bands of sentinel bytes, in one device allocation."""

    def __init__(self, eng, nbytes):
        import torch
        self.n = int(nbytes)
        host = np.full(2 * BAND + self.n, SENT, np.uint8)
        host[BAND:BAND + self.n] = FILL
        self.buf = torch.from_numpy(host).to(eng.device)
        self.ptr = self.buf.data_ptr() + BAND

    def result(self, what, dtype=np.uint8):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        return host[BAND:BAND + self.n].copy().view(dtype)


def same_bits(got, want, what):
    """Equal bit for bit, a NaN equal to any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = (got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want))
    if diff.any():
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        raise AssertionError((what, f"{int(diff.sum())} of {diff.size} values differ, first at {at}: {got[at]!r} here, {want[at]!r} expected"))


def run_forient(eng, imgs, what):
    n, h, w = imgs.shape
    out = Framed(eng, n * h * w * 8)
    d = dev(eng, imgs)
    eng.ctx.call("im_forient", p(d), 0 if imgs.dtype == np.uint8 else 1, n, h, w, out.ptr, eng.stream_ptr())
    return out.result(what, F32).reshape(n, h, w, 2)


def device_inputs(eng, c):
    """(d_a, d_b, d_pairs, d_bidx): the maps as given, or, for a case made of images, im_forient's own output (checked on the way)."""
    if "img_a" in c:
        a = run_forient(eng, c["img_a"][None], c["name"] + " forient a")[0]
        b = run_forient(eng, c["img_b"], c["name"] + " forient b")
        same_bits(a, interleaved(c["A"]), c["name"] + " forient a")
        same_bits(b, interleaved(c["B"]), c["name"] + " forient b")
    else:
        a, b = interleaved(c["A"]), interleaved(c["B"])
    return dev(eng, a), dev(eng, b), dev(eng, c["pairs"]), dev(eng, c["bidx"])


def call_args(c, d):
    ha, wa = c["A"].shape
    n_b, hb, wb = c["B"].shape
    return (p(d[0]), ha, wa, p(d[1]), n_b, hb, wb, p(d[2]), p(d[3]), len(c["pairs"]), c["T"], c["S"], c["conj_b"])


def run_case(eng, c):
    """(C planes [n, R, R] float32 as written over the fill, outputs [6, n] float64)."""
    d = device_inputs(eng, c)
    n, R = len(c["pairs"]), c["S"] - c["T"]
    planes = Framed(eng, n * R * R * 4)
    eng.ctx.call("im_template_match_corr", *call_args(c, d), planes.ptr, eng.stream_ptr())
    out = Framed(eng, 6 * n * 8)
    eng.ctx.call("im_template_match_oc", *call_args(c, d), out.ptr, eng.stream_ptr())
    eng.synchronize()
    return planes.result(c["name"] + " C", F32).reshape(n, R, R), out.result(c["name"] + " outputs", np.float64).reshape(6, n)


def check_case(eng, name):
    c = TC.cases()[name]
    planes, out = run_case(eng, c)
    want = TC.expected_corr(name)
    untouched = int.from_bytes(bytes([FILL]) * 4, "little")
    for i in range(len(c["pairs"])):
        if i in want:
            same_bits(planes[i], want[i], f"{name}: C of pair {i}")
        else:
            assert (planes[i].view(np.uint32) == untouched).all(), f"{name}: the plane of invalid pair {i} was written"
    same_bits(out, np.array(TC.expected_oc(name)), f"{name}: pu pv du dv peakCorr meanAbsCorr")
    return out


@pytest.mark.parametrize("name", list(TC.cases()))
def test_every_case_equals_the_restatement_bit_for_bit(eng, name):
    check_case(eng, name)


def test_scratch_is_reused_across_shapes_large_then_small(eng):
    """One context: R = 96 grows the scratch of C, R = 3 and R = 1 then run in the larger buffer, and R = 96 again."""
    for name in ("default_32_128", "R3_stage_above_reduce", "R1_ks5_idle_lanes", "default_32_128"):
        check_case(eng, name)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
def test_forient_is_bit_identical_with_the_oracle(eng, dtype):
    """1 x 1 (nothing but padding), one row, one column, and widths on either side of the 256-pixel block, several images per call."""
    rng = np.random.default_rng(8)
    for n, h, w in ((3, 1, 1), (2, 1, 9), (2, 9, 1), (2, 255, 3), (2, 3, 255), (2, 257, 3), (3, 3, 257), (1, 2, 2)):
        imgs = rng.integers(0, 256, (n, h, w), dtype=np.uint8) if dtype == np.uint8 else rng.standard_normal((n, h, w)).astype(F32)
        if dtype == np.uint8:
            imgs[0].flat[0] = 255                                  # the full range of a difference
            imgs[0].flat[-1] = 0
        want = np.stack([interleaved(oc_oracle.forient(i)) for i in imgs])
        same_bits(run_forient(eng, imgs, f"forient {n}x{h}x{w}"), want, f"forient {n}x{h}x{w} {np.dtype(dtype).name}")


def test_public_entry_points_return_the_bits_of_the_c_abi(eng):
    from icepy4d_amd.matching.templatematch import OC, match_many
    # OC: one B image, the points of the case as a 1 x n array with per-point initial displacements
    c = TC.cases()["gy16"]
    pu, pv = c["pairs"][None, :, 0].copy(), c["pairs"][None, :, 1].copy()
    r = OC(c["img_a"], c["img_b"][0], pu, pv, c["T"], c["S"], c["pairs"][None, :, 2], c["pairs"][None, :, 3], engine=eng)
    got = np.stack([r.pu[0], r.pv[0], r.du[0], r.dv[0], r.peakCorr[0], r.meanAbsCorr[0]])
    same_bits(got, np.array(TC.expected_oc("gy16")), "OC")
    assert r.pu is pu and np.isfinite(r.du).any()
    # match_many: every point against every B image
    c = TC.cases()["B_larger_than_A_three_B_images"]
    n, n_b = len(c["pairs"]), len(c["B"])
    every = dict(c, pairs=np.tile(c["pairs"], (n_b, 1)), bidx=np.repeat(np.arange(n_b, dtype=np.int32), n))
    want = O.oc(every)
    m = match_many(c["img_a"], list(c["img_b"]), c["pairs"][:, 0], c["pairs"][:, 1], c["T"], c["S"], c["pairs"][:, 2], c["pairs"][:, 3], engine=eng)
    got = np.stack([m[k].reshape(-1) for k in ("pu", "pv", "du", "dv", "peakCorr", "meanAbsCorr")])
    same_bits(got, want, "match_many")
    assert np.isfinite(want[2]).sum() >= n_b * n - 2
    _, abi = run_case(eng, every)
    same_bits(got, abi, "match_many against the C ABI")


def test_refusals_return_the_code_and_write_nothing(eng):
    lib, ctx, s = eng.ctx.lib, eng.ctx.h, eng.stream_ptr()
    c = TC.cases()["R3_stage_above_reduce"]
    d = device_inputs(eng, c)
    n, R = len(c["pairs"]), c["S"] - c["T"]
    good = list(call_args(c, d))
    out, planes = Framed(eng, 6 * n * 8), Framed(eng, n * R * R * 4)
    img = dev(eng, c["img_a"][None])
    fo = Framed(eng, c["img_a"].size * 8)
    count = 0

    def refused(fn, rc, what):
        nonlocal count
        assert rc == REFUSED, (fn, what, rc)
        msg = lib.im_last_error(ctx).decode()
        assert msg.startswith(fn + ": "), (fn, what, msg)
        count += 1

    A_, HA, WA, B_, NB, HB, WB, PAIRS, BIDX, NP, T_, S_, CONJ = range(13)
    changes = [("null A", {A_: None}), ("null B", {B_: None}), ("null pairs", {PAIRS: None}), ("null bidx", {BIDX: None}),
               ("ha < 0", {HA: -1}), ("wa < 0", {WA: -1}), ("hb < 0", {HB: -1}), ("wb < 0", {WB: -1}), ("n_pairs < 0", {NP: -1}),
               ("n_b = 0", {NB: 0}), ("n_b < 0", {NB: -1}), ("T = 0", {T_: 0}), ("T < 0", {T_: -3}), ("S = T", {S_: c["T"]}), ("S < T", {S_: c["T"] - 1})]
    for fn, dst in (("im_template_match_oc", out), ("im_template_match_corr", planes)):
        for what, change in changes:
            args = list(good)
            for k, v in change.items():
                args[k] = v
            refused(fn, getattr(lib, fn)(ctx, *args, dst.ptr, s), what)
        refused(fn, getattr(lib, fn)(ctx, *good, None, s), "null output")
    h, w = c["img_a"].shape
    F = lambda *a: lib.im_forient(ctx, *a, s)                     # noqa: E731  (d_img, dtype, n_images, h, w, d_out)
    refused("im_forient", F(None, 0, 1, h, w, fo.ptr), "null image")
    refused("im_forient", F(p(img), 0, 1, h, w, None), "null output")
    for dtype in (2, -1):
        refused("im_forient", F(p(img), dtype, 1, h, w, fo.ptr), f"dtype {dtype}")
    for bad in ((-1, h, w), (1, -1, w), (1, h, -1), (65536, h, w), (1, 65536, w)):
        refused("im_forient", F(p(img), 0, *bad, fo.ptr), f"n_images, h, w = {bad}")
    assert count == 2 * 16 + 9
    # the empty calls: 0, and nothing written
    assert lib.im_template_match_oc(ctx, *good[:NP], 0, *good[NP + 1:], out.ptr, s) == 0
    assert lib.im_template_match_corr(ctx, *good[:NP], 0, *good[NP + 1:], planes.ptr, s) == 0
    for empty in ((0, h, w), (1, 0, w), (1, h, 0)):
        assert F(p(img), 0, *empty, fo.ptr) == 0, empty
    eng.synchronize()
    for f, what in ((out, "outputs"), (planes, "C"), (fo, "forient")):
        assert (f.result(what) == FILL).all(), what
    # the Python layer raises the library's error
    from icepy4d_amd._lib import IcematchError
    with pytest.raises(IcematchError) as ei:
        eng.ctx.call("im_template_match_corr", *good[:S_], c["T"], good[CONJ], planes.ptr, s)
    assert ei.value.rc == REFUSED and "template width" in str(ei.value)
    # and the context still works
    check_case(eng, "R3_stage_above_reduce")
