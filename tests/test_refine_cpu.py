"""Slanted-window refinement without a device: (a) the cases reach what they are named for, the two consequences of the definition (no
score falls; with a zero slant, candidate 0 of a pixel on plane k scores what the sweep scored at k), the fit against numpy's least squares
and its degenerate ends, the error against the truth of rendered scenes, (b) a host build of the kernels' own rules (csrc/refine_pixel.h
behind the stub <hip/hip_runtime.h>, in tests/refine_host_harness.cpp, a stand-alone program built plain and with the address and
undefined-behaviour sanitizers) against the restatement (tests/refine_oracle.py) bit for bit, (c) the ABI, the compiled resources of the
kernels and the options on `icepy4d_amd.dense`. The device run is tests/test_gpu_refine.py."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import toolchain  # noqa: E402
import dense_oracle as O  # noqa: E402
import refine_cases as C  # noqa: E402
import refine_oracle as RO  # noqa: E402

from icepy4d_amd import dense as D  # noqa: E402
from icepy4d_amd.dense import refine_slanted, slant_map  # noqa: E402,F401  (the feature under test: without it nothing here can pass)
from icepy4d_amd.core.camera import Camera  # noqa: E402

NAMES = ["im_dense_slant", "im_dense_refine"]


# ---- (a) the cases and the restatement ----------------------------------------------------------------------------------------------------------
def test_the_cases_reach_what_they_are_named_for():
    cases, E = C.cases(), C.expected
    shapes = {c["ref"].shape for c in cases.values()}
    assert {(15, 63), (16, 64), (17, 65), (33, 97), (1, 70), (70, 1), (5, 9)} <= shapes
    assert {c["r"] for c in cases.values()} >= {1, 3, 7} and {c["R"] for c in cases.values()} >= {1, 3, 4, 7}
    assert {(c["span"], c["sub"]) for c in cases.values()} >= {(1, 1), (1, 4), (4, 8)}
    assert [n for n, c in cases.items() if (c["span"], c["sub"], c["r"]) == (4, 8, 7)] == ["shape_17x65_r7_R7_span4_sub8"]
    for name, c in cases.items():
        assert c["plane"].dtype == np.int16 and c["w"].dtype == np.float64 and c["score"].dtype == np.float32 and c["ref"].dtype == np.uint8, name
        assert c["plane"].shape == c["w"].shape == c["score"].shape == c["ref"].shape, name
    for name in cases:
        if name.startswith("shape_") and "x70" not in name and "70x" not in name:
            sl, fitted, _, _, taken = E(name)
            assert fitted.sum() > 100 and taken.sum() > 100 and np.abs(sl).max() > 0.01, name
    # one line of pixels: det = 0 whatever is kept
    for name in ("shape_1x70", "shape_70x1"):
        sl, fitted, w, score, taken = E(name)
        assert (cases[name]["plane"] >= 0).sum() > 50 and not fitted.any() and not sl.any() and not taken.any(), name
        s = RO.slant_sums(cases[name]["plane"], cases[name]["w"], cases[name]["w_step"], 3, 2.0)
        assert (s[0] >= 3).sum() > 20                                                     # enough neighbours count: it is the determinant that refuses
    c = cases["ref_smaller_than_window"]
    assert c["ref"].shape == (5, 9) and c["r"] == 3 and E("ref_smaller_than_window")[1].all() and not E("ref_smaller_than_window")[4].any()
    assert np.array_equal(E("ref_smaller_than_window")[2], c["w"])
    # samples that leave src: candidates of kept pixels are invalid on one side only
    c = cases["samples_leave_src_crafted"]
    valid, _ = RO.candidate_scores(c["ref"], c["src"], c["A"], c["B"], c["w"], E("samples_leave_src_crafted")[0], c["w_step"], c["r"], c["min_var"], c["span"], c["sub"])
    inner = np.zeros(c["ref"].shape, bool)
    inner[c["r"]:-c["r"], c["r"]:-c["r"]] = True
    some = inner & (c["plane"] >= 0) & valid.any(0) & ~valid.all(0)
    assert c["src"].shape == c["ref"].shape and some.sum() > 50
    c = cases["z_not_positive"]
    assert (c["plane"] >= 0).sum() > 100 and E("z_not_positive")[4].sum() > 0
    c = cases["nan_in_A"]
    assert np.isnan(c["A"]).sum() == 1 and (c["plane"] >= 0).sum() > 500 and not E("nan_in_A")[4].any()
    assert cases["negative_w_step"]["w_step"] < 0.0 and E("negative_w_step")[4].sum() > 500
    assert not (cases["every_pixel_dropped"]["plane"] >= 0).any() and not any(E("every_pixel_dropped")[i].any() for i in range(5))
    for name in ("crafted_view0", "crafted_view1"):
        c = cases[name]
        kept = c["plane"] >= 0
        beyond = (c["w"] - c["w_first"]) / c["w_step"]
        assert (kept & (c["w"] < 0.0)).sum() > 50 and (kept & (beyond > c["D"] + 5)).sum() > 50 and E(name)[4].sum() > 100, name
    for name in ("constant_patch_in_ref", "constant_patch_in_src"):
        assert cases[name]["min_var"] == 4 and cases[name + "_min_var_0"]["min_var"] == 0
        assert (cases[name]["plane"] < 0).sum() > 100 and E(name)[4].sum() > 0
    c = cases["every_score_is_one"]
    assert (c["score"][c["plane"] >= 0] == 1.0).all() and (c["plane"] >= 0).sum() > 500 and not E("every_score_is_one")[4].any()
    assert np.array_equal(E("every_score_is_one")[2], c["w"]) and np.array_equal(E("every_score_is_one")[3], c["score"])
    c, (_, _, w, score, taken) = cases["filled_pixels_with_score_0"], E("filled_pixels_with_score_0")
    block = (slice(6, 12), slice(20, 40))
    kept = c["plane"][block] >= 0
    assert kept.sum() > 80 and (c["score"][block][kept] == 0.0).all()
    assert taken[block][kept].all() and (score[block][kept] > 0.5).all()                  # any valid candidate is taken: a measured confidence
    # exact ties between candidates -2, +1 and +4 (no mirrored pair): the order 0, -1, +1, -2, ... keeps +1, with the parabola around +1
    c, (sl, _, w, score, taken) = cases["periodic_tie"], E("periodic_tie")
    valid, s = RO.candidate_scores(c["ref"], c["src"], c["A"], c["B"], c["w"], sl, c["w_step"], c["r"], c["min_var"], c["span"], c["sub"])
    inner = (slice(c["r"], -c["r"]), slice(c["r"], -c["r"]))
    assert (c["span"], c["sub"]) == (4, 1) and not sl.any() and valid[:, inner[0], inner[1]].all()
    assert np.array_equal(s[2][inner], s[5][inner]) and np.array_equal(s[5][inner], s[8][inner]) and (s[5][inner] == s.max(0)[inner]).all()
    assert (s[[0, 1, 3, 4, 6, 7]][:, inner[0], inner[1]] < s[5][inner]).all()                 # the three tied candidates are the only best ones
    moved = (w - c["w"])[inner] / c["w_step"]
    assert taken[inner].all() and (np.abs(moved - 1.0) < 0.5).all() and (score[inner] == s[5][inner].astype(np.float32)).all()
    # the gates of the fit
    c = cases["max_diff_gates_every_neighbour"]
    s = RO.slant_sums(c["plane"], c["w"], c["w_step"], c["R"], c["max_diff"])
    assert (s[0] == 1).all() and not E("max_diff_gates_every_neighbour")[1].any() and not E("max_diff_gates_every_neighbour")[0].any()
    c = cases["fewer_than_min_count"]
    s = RO.slant_sums(c["plane"], c["w"], c["w_step"], c["R"], c["max_diff"])
    assert s[0].max() == 9 < c["min_count"] and not E("fewer_than_min_count")[1].any()
    c = cases["max_diff_64_min_count_225"]
    s = RO.slant_sums(c["plane"], c["w"], c["w_step"], 7, 64.0)
    assert np.array_equal(E("max_diff_64_min_count_225")[1] != 0, s[0] == 225) and 0 < (s[0] == 225).sum() < s[0].size


@pytest.mark.parametrize("name", list(C.cases()))
def test_no_score_falls_and_what_is_not_taken_is_copied(name):
    """Consequence (a) of the definition, on every case: score' >= score; taken pixels are kept pixels whose window lies inside ref and
    whose score rose strictly; every other pixel has the bits it had."""
    c = C.cases()[name]
    sl, fitted, w, score, taken = C.expected(name)
    assert sl.dtype == np.float64 and sl.shape == c["plane"].shape + (2,) and fitted.dtype == taken.dtype == np.uint8
    assert w.dtype == np.float64 and score.dtype == np.float32
    kept, t = c["plane"] >= 0, taken != 0
    assert not (score < c["score"]).any() and not (t & ~kept).any() and not fitted[~kept].any() and not sl[~kept].any() and not sl[fitted == 0].any()
    assert (score[t].astype(np.float64) >= c["score"][t]).all() and np.isfinite(w[t]).all()
    assert np.array_equal(w[~t].view(np.int64), c["w"][~t].view(np.int64)) and np.array_equal(score[~t].view(np.int32), c["score"][~t].view(np.int32))
    r, (h0, w0) = c["r"], c["plane"].shape
    inner = np.zeros((h0, w0), bool)
    if h0 > 2 * r and w0 > 2 * r:
        inner[r:h0 - r, r:w0 - r] = True
    assert not (t & ~inner).any()
    moved = np.abs(w[t] - c["w"][t]) / abs(c["w_step"])
    assert (moved <= c["span"] + 0.5 / c["sub"] + 1e-9).all()                             # the parabola moves by at most half a candidate


SWEPT = ["shape_16x64_r3_R4_span1_sub4", "shape_33x97_r3_R4_span1_sub4", "shape_15x63_r1_R1_span1_sub1", "negative_w_step", "window_leaves_src",
         "constant_patch_in_src"]


@pytest.mark.parametrize("name", list(C.cases()))
def test_candidate_0_of_a_zero_slant_scores_what_the_sweep_scored(name):
    """Consequence (b), on every case's pair and schedule: w = w_first + k w_step as the sweep computes it gives the sweep's own H, so
    candidate 0 under a zero slant has the score of plane k, bit for bit, and is valid exactly where the plane was (nowhere, on the pairs
    where no plane scores: a NaN in A, a ref smaller than the window, one row, one column)."""
    c = C.cases()[name]
    valid, s = O.scores(c["ref"], c["src"], c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"])
    zero = np.zeros(c["plane"].shape + (2,))
    for k in range(c["D"]):
        with np.errstate(all="ignore"):
            w = np.full(c["plane"].shape, np.float64(c["w_first"]) + np.float64(k) * np.float64(c["w_step"]))
        v0, s0 = RO.candidate_scores(c["ref"], c["src"], c["A"], c["B"], w, zero, c["w_step"], c["r"], c["min_var"], 1, 1)
        assert np.array_equal(v0[1], valid[k]) and np.array_equal(s0[1].view(np.int64), s[k].view(np.int64)), (name, k)
    assert valid.any() or name not in SWEPT


def test_the_fit_equals_least_squares_and_recovers_an_affine_map_exactly():
    rng = np.random.default_rng(5)
    h, w, step = 21, 30, 0.01
    # an affine map whose heights are whole 1024ths of a step: recovered exactly wherever it is fitted, at the border too
    gu, gv = 37.0 / 1024.0, -90.0 / 1024.0
    uu, vv = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    plane = np.full((h, w), 2, np.int16)
    wmap = 0.5 + (gu * uu + gv * vv) * 0.5                 # w_step = 0.5: every difference and every quotient is exact
    sl, fitted = RO.slant(plane, wmap, 0.5, R=3, max_diff=2.0, min_count=6)
    assert fitted.all() and (sl[..., 0] == gu).all() and (sl[..., 1] == gv).all()
    sl, fitted = RO.slant(plane, wmap, -0.5, R=3, max_diff=2.0, min_count=6)             # counted from the far end: the slant changes its sign
    assert fitted.all() and (sl[..., 0] == -gu).all() and (sl[..., 1] == -gv).all()
    # a noisy map with dropped pixels against numpy.linalg.lstsq on the same integer heights
    plane = rng.integers(-1, 4, (h, w)).astype(np.int16)
    wmap = np.where(plane >= 0, 0.2 + (0.05 * uu - 0.03 * vv + rng.normal(0.0, 0.7, (h, w))) * step, 0.0)
    R, max_diff = 2, 1.5
    sl, fitted = RO.slant(plane, wmap, step, R=R, max_diff=max_diff, min_count=4)
    checked = 0
    for v in range(h):
        for u in range(w):
            if plane[v, u] < 0:
                assert fitted[v, u] == 0
                continue
            rows, q = [], []
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    y, x = v + dy, u + dx
                    if 0 <= y < h and 0 <= x < w and plane[y, x] >= 0:
                        d = (wmap[y, x] - wmap[v, u]) / step
                        if abs(d) <= max_diff:
                            rows.append((1.0, dx, dy))
                            q.append(float(np.rint(d * 1024.0)))
            M = np.array(rows)
            if len(rows) >= 4 and np.linalg.matrix_rank(M) == 3:
                sol = np.linalg.lstsq(M, np.array(q), rcond=None)[0]
                assert fitted[v, u] == 1 and np.allclose(sl[v, u] * 1024.0, sol[1:], rtol=1e-9, atol=1e-9), (v, u)
                checked += 1
            else:
                assert fitted[v, u] == 0 and not sl[v, u].any()
    assert checked > 300


# ---- the error against the truth of rendered scenes -------------------------------------------------------------------------------------------------
def test_the_error_does_not_rise_on_rendered_scenes():
    """Four rendered 48 x 80 scenes (`refine_cases.SCENES`), swept by the restatement with min_score 0.8 and refined twice with the defaults
    (fit_radius 4, max_diff 2, min_count 6, span 1, sub 4): the RMS of (w - truth) / w_step over the kept pixels does not rise after either
    pass. That is all that is asserted. Measured with this restatement, before -> after pass 1 -> after pass 2, as RMS / worst / 99th
    percentile in plane steps, and the mean score:
      slant 0.06 / 0.05 (seed 1, D 13, r 3)      0.0739 / 0.3159 / 0.1952  ->  0.0124 / 0.1221 / 0.0346  ->  0.0118 / 0.1221 / 0.0331;  0.9587 -> 0.9978 -> 0.9998
      slant 0.15 / 0.10 (seed 2, D 21, r 3)      0.1185 / 0.4708 / 0.3245  ->  0.0166 / 0.1146 / 0.0567  ->  0.0087 / 0.1068 / 0.0235;  0.9278 -> 0.9971 -> 0.9998
      the same, r 5 (seed 4)                     0.1210 / 0.5177 / 0.3168  ->  0.0185 / 0.1493 / 0.0657  ->  0.0049 / 0.0384 / 0.0148;  0.8698 -> 0.9950 -> 0.9997
      the same, r 3, Gaussian noise sigma 4      0.1247 / 0.4606 / 0.3431  ->  0.0341 / 0.1695 / 0.0895  ->  0.0324 / 0.1695 / 0.0848;  0.9148 -> 0.9842 -> 0.9869
    Not asserted (README reports them): under noise of sigma 10 the same slanted scene goes 0.1535 -> 0.0824 -> 0.0821 (mean score 0.8693 ->
    0.9347), and a fronto-parallel one 0.0751 -> 0.0974 -> 0.0872: on a flat surface under heavy noise the quarter-step candidates and a
    noisy slant chase the noise, and the error rises a little."""
    for name in C.ASSERTED:
        e = C.errors(name)
        taken = [int(s[2].sum()) for s in C.scene(name)[2]]
        print(name, [tuple(round(x, 4) for x in s) for s in e], "taken", taken)
        assert (C.scene(name)[1] >= 0).sum() > 2000 and taken[1] > 1000
        assert e[1][0] <= e[0][0] and e[2][0] <= e[1][0], (name, e)
        assert e[2][3] >= e[1][3] >= e[0][3]                                              # consequence (a) again: the mean score cannot fall


def test_a_clean_fronto_parallel_scene_is_left_alone():
    """The clean fronto-parallel scene (seed 1, D 13, k_true 6): every kept pixel already scores what its best candidate scores, `taken` is
    empty after both passes and the map keeps its bits. Measured: RMS 0.0447, worst 0.2004, 99th percentile 0.1216 plane steps, mean score
    1.0000, before and after."""
    p, plane, states = C.scene("fronto_parallel")
    assert (plane >= 0).sum() > 2000
    for w, score, taken in states[1:]:
        assert not taken.any() and np.array_equal(w, states[0][0]) and np.array_equal(score, states[0][1])
    print([tuple(round(x, 4) for x in s) for s in C.errors("fronto_parallel")])


# ---- (b) the host build of the kernels' rules ---------------------------------------------------------------------------------------------------
def write_records(path):
    with open(path, "wb") as f:
        for name, c in C.cases().items():
            out = C.expected(name)
            label = "refine " + name
            f.write(struct.pack("<qq", 1, len(label)) + label.encode())
            f.write(np.asarray([*c["ref"].shape, *c["src"].shape, c["r"], c["min_var"], c["span"], c["sub"], c["R"], c["min_count"]], np.int64).tobytes())
            f.write(np.concatenate([np.asarray(c["A"], np.float64).reshape(9), np.asarray(c["B"], np.float64).reshape(9),
                                    [c["w_step"], c["max_diff"]]]).astype(np.float64).tobytes())
            for k, t in (("ref", np.uint8), ("src", np.uint8), ("plane", np.int16), ("w", np.float64), ("score", np.float32)):
                assert c[k].dtype == t
                f.write(np.ascontiguousarray(c[k]).tobytes())
            for a, t in zip(out, (np.float64, np.uint8, np.float64, np.float32, np.uint8)):
                assert a.dtype == t
                f.write(np.ascontiguousarray(a).tobytes())
    return len(C.cases())


@pytest.fixture(scope="module")
def harness_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("refine_host"))
    return d, write_records(os.path.join(d, "records.bin"))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_equals_the_restatement_bit_for_bit(harness_dir, sanitize):
    d, n = harness_dir
    exe = toolchain.host_program(d, "refine_host_harness.cpp", sanitize)
    r = subprocess.run([exe, os.path.join(d, "records.bin")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout[-3000:] + r.stderr[-3000:]
    assert n == len(C.cases()) and r.stdout.count("\nok ") + r.stdout.startswith("ok ") == n
    assert "DIFFERENT" not in r.stdout and "MISSING" not in r.stdout
    with open(os.path.join(ROOT, "tests", "refine_host_harness.cpp")) as f:
        text = f.read()
    assert '#include "refine_pixel.h"' in text and "#include <hip/" not in text and "int main(" in text      # the stub stands in for the runtime


# ---- (c) the ABI, the kernels' resources, the options ---------------------------------------------------------------------------------------------
def test_abi_is_declared_bound_and_exported():
    from icepy4d_amd import _lib
    with open(os.path.join(ROOT, "include", "icematch.h")) as f:
        header = f.read()
    for n in NAMES:
        m = re.search(r"\nint " + n + r"\(([^;]*)\);", header)
        assert m and n in _lib.SIGNATURES, n
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[n]), (n, len(args), len(_lib.SIGNATURES[n]))
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES)
    assert (D.MAX_FIT_RADIUS, D.MAX_SLANT_DIFF, D.MAX_SPAN, D.MAX_SUB) == (RO.MAX_FIT_RADIUS, RO.MAX_DIFF, RO.MAX_SPAN, RO.MAX_SUB) == (7, 64.0, 4, 8)
    with open(os.path.join(toolchain.CSRC, "refine_pixel.h")) as f:
        text = f.read()
    assert "REFINE_MAX_FIT_RADIUS = 7, REFINE_MIN_COUNT = 3, REFINE_MAX_COUNT = 225, REFINE_MAX_SPAN = 4, REFINE_MAX_SUB = 8" in text
    # every function of this header that computes in float64 switches contraction off: slant_height, slant_fit and refine_pixel, three.
    # (refine_best_step only compares; the score, the parabola and the sample carry their own pragma in dense_pixel.h.) And the int64 headroom
    assert text.count("#pragma clang fp contract(off)") == 3 and "static_assert" in text
    for fn in ("slant_height", "slant_fit", "refine_pixel"):
        assert re.search(r"bool " + fn + r"\([^{]*\{\n#pragma clang fp contract\(off\)", text), fn
    assert "sqrt" not in text and "fma" not in text and "atomic" not in text                  # + - * /; the one sqrt is dense_score's
    with open(os.path.join(toolchain.CSRC, "dense_pixel.h")) as f:
        dense = f.read()
    assert "dense_plane_at(A, B, w_first + (double)k * w_step, H)" in dense                   # one definition of H = A + w B
    with open(os.path.join(toolchain.CSRC, "dense_refine.hip")) as f:
        assert "atomic" not in f.read().split("#include", 1)[1]


def test_the_kernels_use_no_scratch_memory(tmp_path):
    """Two kernels of 256 threads per 64 x 16 tile: no scratch, no spills; the LDS of the slant kernel is the tile and its largest halo in
    float64 with the kept flags (78 x 30 x 9 bytes), that of the refinement the ref bytes and the two matrices."""
    res = toolchain.kernel_resources(toolchain.device_listing("dense_refine.hip", str(tmp_path)))
    assert len(res) == 2 and all(any(k in name for name in res) for k in ("dense_slant_kernel", "dense_refine_kernel")), sorted(res)
    for k, f in res.items():
        print(k, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "lds", f["group_segment_fixed_size"])
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (k, dict(f))
        assert f["max_flat_workgroup_size"] == 256 and f["vgpr_count"] <= 128 and f["group_segment_fixed_size"] <= 78 * 30 * 9 + 64


def cameras():
    K = np.array([[1200.0, 0.0, 400.0], [0.0, 1200.0, 300.0], [0.0, 0.0, 1.0]])
    return [Camera(800, 600, K=K, R=np.eye(3), t=np.zeros(3)), Camera(800, 600, K=K, R=np.eye(3), t=np.array([-1.0, 0.02, 0.05]))]


REFUSALS = [
    ("a refine that is no pair", dict(refine=2), "refine is None"),
    ("a refine of three", dict(refine=(2, 4, 1)), "refine is None"),
    ("an unknown option", dict(refine=dict(passes=1, radius=3)), "unknown options"),
    ("passes 0", dict(refine=(0, 4)), "passes"),
    ("passes 17", dict(refine=(17, 4)), "passes"),
    ("passes True", dict(refine=(True, 4)), "passes"),
    ("passes 1.5", dict(refine=(1.5, 4)), "passes"),
    ("fit_radius 0", dict(refine=(2, 0)), "fit_radius"),
    ("fit_radius 8", dict(refine=(2, 8)), "fit_radius"),
    ("max_diff 0", dict(refine=dict(max_diff=0.0)), "max_diff"),
    ("max_diff above 64", dict(refine=dict(max_diff=64.5)), "max_diff"),
    ("max_diff that is no number", dict(refine=dict(max_diff=float("nan"))), "max_diff"),
    ("min_count 2", dict(refine=dict(min_count=2)), "min_count"),
    ("min_count 226", dict(refine=dict(min_count=226)), "min_count"),
    ("span 0", dict(refine=dict(span=0)), "span"),
    ("span 5", dict(refine=dict(span=5)), "span"),
    ("sub 0", dict(refine=dict(sub=0)), "sub"),
    ("sub 9", dict(refine=dict(sub=9)), "sub"),
    ("a one-plane schedule", dict(refine=(2, 4), depth_range=(30.0, 30.0)), "w_step"),
]


@pytest.mark.parametrize("what,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_python_layer_refuses_before_any_device_work(what, change, text, monkeypatch):
    from icepy4d_amd import engine
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    monkeypatch.setattr(D, "default_engine", lambda e: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    args = dict(images=[np.zeros((600, 800), np.uint8), np.zeros((600, 800), np.uint8)], cameras=cameras(), depth_range=(20.0, 60.0))
    args.update(change)
    with pytest.raises(ValueError, match=text):
        D.build_dense_cloud(**args)
    with pytest.raises(ValueError, match=text):
        D.build_depth_maps(**args)


def a_map(h, w, step=0.01):
    import torch
    return D.DepthMap(torch.zeros((h, w), dtype=torch.int16), torch.zeros((h, w), dtype=torch.float64), torch.zeros((h, w)), None,
                      torch.zeros((h, w), dtype=torch.uint8), np.eye(3), np.eye(3), np.zeros(3), (0.1, step, 5))


def test_the_two_functions_refuse_before_any_device_work(monkeypatch):
    import torch
    monkeypatch.setattr(D, "default_engine", lambda e: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    m, o = a_map(20, 30), a_map(22, 36)
    for bad, text in ((dict(fit_radius=0), "fit_radius"), (dict(fit_radius=8), "fit_radius"), (dict(max_diff=0.0), "max_diff"), (dict(max_diff=65.0), "max_diff"),
                      (dict(max_diff="2"), "max_diff"), (dict(min_count=2), "min_count"), (dict(min_count=226), "min_count")):
        with pytest.raises(ValueError, match=text):
            D.slant_map(m, **bad)
        with pytest.raises(ValueError, match=text):
            D.refine_slanted(m, o, **bad)
    for bad, text in ((dict(passes=0), "passes"), (dict(span=0), "span"), (dict(span=5), "span"), (dict(sub=0), "sub"), (dict(sub=9), "sub"),
                      (dict(radius=0), "radius"), (dict(radius=8), "radius"), (dict(min_var=-1), "min_var"), (dict(min_var=(1 << 26) + 1), "min_var")):
        with pytest.raises(ValueError, match=text):
            D.refine_slanted(m, o, **bad)
    for step in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="w_step"):
            D.slant_map(a_map(20, 30, step))
        with pytest.raises(ValueError, match="w_step"):
            D.refine_slanted(a_map(20, 30, step), o)
    with pytest.raises(ValueError, match="float64"):
        D.slant_map(m._replace(w=m.w.to(torch.float32)))
    with pytest.raises(ValueError, match="float32"):
        D.refine_slanted(m._replace(score=m.score.to(torch.float64)), o)
    with pytest.raises(ValueError, match="int16"):
        D.slant_map(m._replace(plane=m.plane.to(torch.int32)))
    with pytest.raises(ValueError, match="grey"):
        D.refine_slanted(m, o._replace(grey=None))
    with pytest.raises(ValueError, match="grey"):
        D.refine_slanted(m._replace(grey=o.grey), o)


class FakeContext:
    def __init__(self):
        self.names, self.args = [], []

    def call(self, name, *args):
        self.names.append(name)
        self.args.append(args)
        if name == "im_dense_refine":                                                     # h_A and h_B live as long as the call
            self.matrices = [np.array((ctypes.c_double * 9).from_address(args[i])) for i in (6, 7)]


class FakeEngine:
    def __init__(self):
        import torch
        self.device, self.ctx = torch.device("cpu"), FakeContext()

    def stream_ptr(self):
        return None


def small_pair():
    images = [np.zeros((60, 80), np.uint8), np.zeros((60, 80), np.uint8)]
    K = np.array([[120.0, 0.0, 40.0], [0.0, 120.0, 30.0], [0.0, 0.0, 1.0]])
    return images, [Camera(80, 60, K=K, R=np.eye(3), t=np.zeros(3)), Camera(80, 60, K=K, R=np.eye(3), t=np.array([-1.0, 0.0, 0.0]))]


def test_without_the_option_no_new_call_is_made(monkeypatch):
    """`refine=None` is today's path: the engine's `call` sees the names it saw before. The option adds, per view and pass, the slant and
    the refinement, behind the clean-up and before the consistency check, with the call's radius and min_var and the sweep's own A and B."""
    import torch
    images, cams = small_pair()
    eng = FakeEngine()
    monkeypatch.setattr(D, "default_engine", lambda e: eng)
    monkeypatch.setattr(torch, "empty", torch.zeros)
    per_view = ["im_dense_consistency", "im_dense_cloud"]
    for extra in (dict(), dict(refine=None)):
        eng.ctx.names.clear()
        D.build_dense_cloud(images, cams, depth_range=(8.0, 12.0), views=(0, 1), engine=eng, **extra)
        assert eng.ctx.names == ["im_dense_sweep"] * 2 + per_view * 2
        eng.ctx.names.clear()
        D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng, **extra)
        assert eng.ctx.names == ["im_dense_sweep"] * 2
    pass_ = ["im_dense_slant", "im_dense_refine"]
    eng.ctx.names.clear()
    eng.ctx.args.clear()
    D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng, radius=2, min_var=9, refine=(2, 3))
    assert eng.ctx.names == ["im_dense_sweep"] * 2 + pass_ * 4
    sweep0, slant0, refine0 = eng.ctx.args[0], eng.ctx.args[2], eng.ctx.args[3]
    assert slant0[4:8] == (sweep0[9], 3, 2.0, 6)                                          # w_step, fit_radius, max_diff, min_count
    assert refine0[12:17] == (sweep0[9], 2, 9, 1, 4)                                      # w_step, r, min_var, span, sub
    want = D.sweep_matrices(cams[1].K, cams[0].K, *D.relative_pose(cams[1], cams[0]))     # the last call refined view 1
    assert np.array_equal(eng.ctx.matrices[0], want[0]) and np.array_equal(eng.ctx.matrices[1], want[1])
    eng.ctx.names.clear()
    D.build_dense_cloud(images, cams, depth_range=(8.0, 12.0), views=(0,), engine=eng, speckle=(4, 1), holes=(16, 2), refine=dict(passes=1, sub=2, span=2))
    clean = ["im_depth_components", "im_depth_drop_small", "im_depth_components", "im_depth_fill_holes"]
    assert eng.ctx.names == (["im_dense_sweep"] + clean) * 2 + pass_ * 2 + per_view


def test_dense_series_hands_refine_down(monkeypatch):
    calls = []
    monkeypatch.setattr(D, "build_dense_cloud", lambda images, cameras, **kw: calls.append(kw) or len(calls))
    D.dense_series([["a0", "a1"]], cameras(), refine=(1, 5))
    assert calls[0]["refine"] == (1, 5)
    calls.clear()
    D.dense_series([["a0", "a1"]], cameras())
    assert "refine" not in calls[0]
