"""Dense surface displacement without a device: (a) the cases reach what they are named for; the consequences of the definition on shifted
textures, on rendered two-epoch scenes and under the forward-backward check, all in the restatement (tests/flow_oracle.py), (b) a host
build of the kernels' own rules (csrc/flow_pixel.h behind the stub <hip/hip_runtime.h>, in tests/flow_host_harness.cpp, a stand-alone
program built plain and with the address and undefined-behaviour sanitizers) against the restatement bit for bit, (c) the ABI, the compiled
resources of the kernels and the arguments that `icepy4d_amd.dense_flow` refuses. The device run is tests/test_gpu_flow.py."""
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
import dense_cases as DC  # noqa: E402
import dense_oracle as O  # noqa: E402
import flow_cases as C  # noqa: E402
import flow_oracle as FO  # noqa: E402

from icepy4d_amd import dense_flow as DF  # noqa: E402  (the feature under test: without it nothing here can pass)

NAMES = ["im_flow_match", "im_flow_check", "im_flow_lift"]


# ---- (a) the cases and the restatement ------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_what_they_are_named_for():
    m, E = C.matches(), C.match_expected
    assert {(15, 63), (16, 64), (17, 65), (33, 97), (1, 70), (70, 1), (5, 9)} <= {c["a"].shape for c in m.values()}
    assert {c["r"] for c in m.values()} >= {1, 3, 7, 15} and {c["S"] for c in m.values()} >= {0, 1, 4, 16}
    assert [n for n, c in m.items() if (c["r"], c["S"]) == (15, 16)] == ["largest_r15_S16_40x80"] and E("largest_r15_S16_40x80")[3].sum() > 100
    for name, c in m.items():
        assert c["a"].dtype == c["b"].dtype == np.uint8 and c["a"].shape == c["b"].shape, name
        if name.startswith("shape_") and "x70" not in name and "70x" not in name:
            assert E(name)[3].sum() > 100, name
    for name in ("shape_1x70", "shape_70x1", "image_smaller_than_window", "prior_pushes_every_window_out", "mask_asks_for_nothing"):
        assert not any(a.any() for a in E(name)), name
    assert not C.candidates("prior_pushes_every_window_out")[0].any() and C.candidates("mask_asks_for_nothing")[0].any()
    c, e = m["prior_4_-2_shift_5_-3"], E("prior_4_-2_shift_5_-3")
    assert c["prior"] == (4, -2) and (np.rint(e[0][e[3] != 0]) == 5).mean() > 0.95 and (np.rint(e[1][e[3] != 0]) == -3).mean() > 0.95
    e = E("prior_-12_9_shift_-13_10")
    assert e[3].sum() > 300 and (e[0][e[3] != 0] == -13.0).all() and (e[1][e[3] != 0] == 10.0).all()      # the best on the rim of S = 1: whole pixels
    v = C.candidates("prior_leaves_a_strip")[0].any((0, 1))
    assert v[:, :8].any() and not v[:, 12:].any() and 0 < E("prior_leaves_a_strip")[3].sum() < 200
    # constant patches: pixels whose window lies in the patch never score, whatever min_var is (a zero variance is invalid); at the patch's
    # edge a window holds a little texture, which min_var = 4 refuses and min_var = 0 takes
    for name, img in (("constant_patch_in_a", "a"), ("constant_patch_in_b", "b")):
        assert m[name]["min_var"] == 4 and m[name + "_min_var_0"]["min_var"] == 0
        flat = (O.box(m[name][img].astype(np.int64) ** 2, 2) * 25 - O.box(m[name][img].astype(np.int64), 2) ** 2) == 0
        assert flat.sum() > 100
        if img == "a":
            assert not E(name)[3][2:-2, 2:-2][flat].any() and not E(name + "_min_var_0")[3][2:-2, 2:-2][flat].any()
        assert (C.candidates(name + "_min_var_0")[0].sum() >= C.candidates(name)[0].sum())
    one = m["mask_one_pixel_per_tile"]["ask"]
    assert one.sum() == 6 and all(one[y0:y0 + 16, x0:x0 + 64].sum() == 1 for y0 in (0, 16, 32) for x0 in (0, 64))
    e, full = E("mask_one_pixel_per_tile"), FO.match(m["mask_one_pixel_per_tile"]["a"], m["mask_one_pixel_per_tile"]["b"], None, 3, 4, (0, 0), 4, 0.5)
    assert 0 < e[3].sum() <= 6 and not e[3][one == 0].any() and all(np.array_equal(np.where(one != 0, f, 0), g) for f, g in zip(full, e))
    ask = m["mask_random_and_one_empty_tile"]["ask"]
    assert not ask[:, 64:].any() and 500 < ask.sum() < 1500
    # the periodic texture: dx = -3, 0, +3 score the same bits and nothing scores more; the smallest displacement wins
    valid, s = C.candidates("periodic_tie")
    inner = (slice(2, -2), slice(5, -5))
    assert valid[4, 1][inner].all() and np.array_equal(s[4, 1][inner], s[4, 4][inner]) and np.array_equal(s[4, 7][inner], s[4, 4][inner])
    assert (s[4, 4][inner] == s.max((0, 1))[inner]).all()
    e = E("periodic_tie")
    assert e[3][inner].all() and (np.rint(e[0][inner]) == 0).all() and (np.abs(e[0][inner]) <= 0.5).all()
    for name, axis, rim in (("best_on_the_rim_along_x", 0, 4.0), ("best_on_the_rim_along_y", 1, -4.0)):
        e = E(name)
        k = e[3] != 0
        c = m[name]                                                                       # of the pixels whose true window lies inside b, every one
        uu, vv = np.meshgrid(np.arange(70), np.arange(20))
        sx, sy = (4, 1) if axis == 0 else (-1, -4)
        true_inside = k & (uu + sx >= 2) & (uu + sx < 68) & (vv + sy >= 2) & (vv + sy < 18)
        assert c["S"] == 4 and true_inside.sum() > 500 and (e[axis][true_inside] == rim).all(), name
        assert (e[1 - axis][true_inside] != np.rint(e[1 - axis][true_inside])).mean() > 0.9, name      # the other axis does take its offset
    assert E("every_score_kept")[3].sum() == 15 * 63 and (E("every_score_kept")[2] < 0.5).sum() > 10
    # checks
    k, E = C.checks(), C.check_expected
    c = k["backward_hit_on_an_invalid_pixel"]
    assert not E("backward_hit_on_an_invalid_pixel")[:, 18:38].any() and E("backward_hit_on_an_invalid_pixel")[:, :18].all() and c["valid"].all()
    e = E("hit_outside_the_image")
    assert not e[:, :8].any() and not e[:, -8:].any() and not e[:3].any() and not e[-3:].any() and e[3:-3, 8:-8].all()
    e = E("sum_exactly_at_tol")
    assert e[:, 1:62:2].all() and not e[:, 0::2].any()                                      # pixel u lands on column u + 3: an even one for an odd u
    assert E("sum_exactly_at_tol_3_4_5")[:13, :62].all()
    c, e = k["nan_fails"], E("nan_fails")
    assert np.isnan(c["du"]).sum() > 20 and np.isnan(c["du_b"]).sum() > 20 and not e[np.isnan(c["du"])].any() and e.sum() > 100
    assert 0 < E("from_match_shape_33x97_r3_S4").sum() < (k["from_match_shape_33x97_r3_S4"]["valid"] != 0).sum()
    # lifts
    L, E = C.lifts(), C.lift_expected
    assert {(15, 63), (16, 64), (17, 65), (33, 97), (1, 70), (70, 1)} <= {c["du"].shape for c in L.values()}
    for name in L:
        P, D, ok = E(name)
        assert not P[ok == 0].any() and not D[ok == 0].any() and np.isfinite(P).all() and np.isfinite(D).all(), name
        c = L[name]
        assert not ok[(c["keep"] == 0) | (c["plane_a"] < 0) | (c["valid"] == 0)].any(), name
    assert not E("shape_1x70")[2].any() and not E("shape_70x1")[2].any()                    # a map of one row holds no four taps
    ok = E("a_tap_outside_and_an_integer_x_in_the_last_column")[2]
    assert not ok[:, -3:].any() and not ok[:, :2].any() and not ok[:, -6].any() and ok[:-1, -7].all() and ok[:-1, 2:-7].all() and not ok[-1].any()
    ok = E("a_tap_dropped_and_a_tap_not_kept")[2]
    assert not ok[4:8, 19:30].any() and not ok[9:13, 39:50].any() and ok[:3, :-1].all() and ok[13:-1, :-1].all()
    for name in ("span_exactly_at_and_just_above_max_diff", "span_exactly_at_and_just_above_max_diff_negative_step"):
        ok = E(name)[2]
        assert ok[3:5, 9:30].all() and not ok[11:13, 9:27:4].any() and not ok[11:13, 10:27:4].any() and ok[11:13, 11:27:4].all(), name
    assert L["negative_w_step_b"]["w_step_b"] < 0 and E("negative_w_step_b")[2].sum() > 200
    assert 0 < E("rough_map_b_gated_by_max_diff")[2].sum() < E("shape_33x97")[2].sum() / 2
    assert L["map_b_of_another_shape"]["plane_b"].shape == (20, 50)


@pytest.mark.parametrize("r,S,shift", [(2, 3, (2, -3)), (3, 4, (-4, 1)), (7, 2, (1, 2))])
def test_a_shifted_texture_is_found_where_its_windows_lie_inside(r, S, shift):
    """`dense_cases.texture` cut twice at an integer offset inside the search range: every pixel whose template and whose window at the true
    shift lie inside the images is valid, with rint(du) == sx, rint(dv) == sy, score == 1.0 and |du - sx| <= 0.5. Pixels whose true window
    leaves b do go wrong: that is the condition's reason. Measured: the RMS of du - sx and dv - sy (the parabola's bias) is printed."""
    sx, sy = shift
    h, w = 40, 70
    a, b = C.shifted(600 + r, h, w, sx, sy)
    du, dv, score, valid = FO.match(a, b, None, r, S)
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    inside = (uu >= r) & (uu < w - r) & (vv >= r) & (vv < h - r) & (uu + sx >= r) & (uu + sx < w - r) & (vv + sy >= r) & (vv + sy < h - r)
    assert inside.sum() > 500 and valid[inside].all()
    assert (np.rint(du[inside]) == sx).all() and (np.rint(dv[inside]) == sy).all() and (score[inside] == 1.0).all()
    assert (np.abs(du[inside] - sx) <= 0.5).all() and (np.abs(dv[inside] - sy) <= 0.5).all()
    e = np.concatenate([du[inside] - sx, dv[inside] - sy])
    print(f"r {r} S {S}: sub-pixel bias RMS {np.sqrt((e * e).mean()):.4f} px, worst {np.abs(e).max():.4f} px")


def test_the_forward_backward_check_drops_an_overwritten_region_and_keeps_the_rest():
    """On a shifted texture the check keeps every pixel that is valid in both directions and whose windows stay inside. With a region of b
    overwritten by another texture, every pixel of a whose true window lies wholly in that region is dropped. The radius is 7 for a reason:
    the score is symmetric, so a false match that passes min_score is usually confirmed by the backward field, and only min_score stands
    against it. The texture is white noise under two 2 x 2 box filters, so a window of 15 x 15 holds about 225 / 4 independent samples and
    the score of two unrelated windows has a standard deviation near 0.13: min_score = 0.8 is six of them away. At radius 3 (about 12
    samples, 0.29) it is fewer than three, and some of the 81 candidates of some pixel do pass."""
    r, S, (sx, sy) = 7, 4, (2, -1)
    h, w = 56, 100
    a, b = C.shifted(610, h, w, sx, sy)
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    inside = (uu >= r) & (uu < w - r) & (vv >= r) & (vv < h - r) & (uu + sx >= r) & (uu + sx < w - r) & (vv + sy >= r) & (vv + sy < h - r)
    fwd, bwd = FO.match(a, b, None, r, S), FO.match(b, a, None, r, S)
    keep = FO.check(fwd[0], fwd[1], fwd[3], bwd[0], bwd[1], bwd[3], 1.0)
    both = inside & (fwd[3] != 0)
    both[both] &= bwd[3][vv[both] + sy, uu[both] + sx] != 0
    assert both.sum() > 2000 and keep[both].all()
    # a region of b overwritten with another texture: a pixel of a whose true window lies wholly in it has lost its partner
    b2 = b.copy()
    y0, y1, x0, x1 = 8, 48, 25, 85
    b2[y0:y1, x0:x1] = DC.texture(611, y1 - y0, x1 - x0)
    lost = (uu + sx - r >= x0) & (uu + sx + r < x1) & (vv + sy - r >= y0) & (vv + sy + r < y1)
    fwd, bwd = FO.match(a, b2, None, r, S), FO.match(b2, a, None, r, S)
    keep = FO.check(fwd[0], fwd[1], fwd[3], bwd[0], bwd[1], bwd[3], 1.0)
    print("lost", int(lost.sum()), "forward matches among them", int(fwd[3][lost].sum()), "kept", int(keep[lost].sum()))
    assert lost.sum() > 500 and not keep[lost].any()
    far = inside & ((uu + sx + r + S < x0) | (uu + sx - r - S >= x1) | (vv + sy + r + S < y0) | (vv + sy - r - S >= y1))
    assert far.sum() > 100 and keep[far].all()


# ---- rendered scenes: two epochs of a plane --------------------------------------------------------------------------------------------------------
H0, W0, PLANES, K_TRUE, SHIFT = 40, 80, 7, 2, (3, -2)


def epoch(tex, cut, k_true, R0, t0):
    """One epoch of a fronto-parallel plane on plane k_true of `dense_cases.pair`'s schedule (baseline 1 along x, f = 120 px, plane k at a
    disparity of 10 + k px), seen by a stereo pair whose view 0 has the world pose (R0, t0): view 1 is the texture cut at `cut`, view 0 is
    rendered from it; swept by the restatement. A map as `flow_oracle.surface_displacement` takes it, with its keep mask."""
    p = DC.pair(0, H0, W0, PLANES, 3, k_true=k_true)
    h1, w1 = p["src"].shape
    src = np.ascontiguousarray(tex[C.M - cut[1]:C.M - cut[1] + h1, C.M - cut[0]:C.M - cut[0] + w1])
    ref = DC.render(src, p["A"], p["B"], np.full((H0, W0), p["w_first"] + k_true * p["w_step"]))
    plane, w, score = O.sweep(ref, src, p["A"], p["B"], p["w_first"], p["w_step"], PLANES, 3, 4, 0.8)
    return dict(grey=ref, plane=plane, w=w, K=p["K0"], R=np.asarray(R0, np.float64), t=np.asarray(t0, np.float64), w_step=p["w_step"],
                w_true=p["w_first"] + k_true * p["w_step"]), (plane >= 0).astype(np.uint8)


def scenes():
    """name -> (map A, keep A, map B, keep B, the analytic D [h, w, 3] in world coordinates)."""
    sx, sy = SHIFT
    tex = DC.texture(620, H0 + 2 * C.M + 8, W0 + 2 * C.M + 40)
    R0, t0 = DC.R_WORLD, DC.T_WORLD
    a, keep_a = epoch(tex, (0, 0), K_TRUE, R0, t0)
    Ki = O.W.inv3(a["K"])
    uu, vv = np.meshgrid(np.arange(W0, dtype=np.float64), np.arange(H0, dtype=np.float64))
    ray = lambda x, y: np.stack([Ki[i, 0] * x + Ki[i, 1] * y + Ki[i, 2] for i in range(3)], -1)      # noqa: E731
    out = {}
    # the plane moved parallel to the image by a whole-pixel shift: both views see the texture moved by (sx, sy)
    b, keep_b = epoch(tex, (sx, sy), K_TRUE, R0, t0)
    D_cam = ray(uu + sx, vv + sy) / b["w_true"] - ray(uu, vv) / a["w_true"]
    out["shifted"] = (a, keep_a, b, keep_b, D_cam @ R0)
    # the same shift and two planes nearer: two more pixels of disparity, so view 1 sees the texture moved by (sx - 2, sy)
    b, keep_b = epoch(tex, (sx - 2, sy), K_TRUE + 2, R0, t0)
    D_cam = ray(uu + sx, vv + sy) / b["w_true"] - ray(uu, vv) / a["w_true"]
    out["shifted_and_two_planes_nearer"] = (a, keep_a, b, keep_b, D_cam @ R0)
    # the surface has not moved, epoch B's cameras have: their centre moved by c in camera axes, which shifts both images by (sx, sy)
    c = np.array([-sx / (DC.F * a["w_true"]), -sy / (DC.F * a["w_true"]), 0.0])
    b, keep_b = epoch(tex, (sx, sy), K_TRUE, R0, t0 - c)
    out["camera_moved_surface_still"] = (a, keep_a, b, keep_b, np.zeros((H0, W0, 3)))
    return out


def test_rendered_scenes_give_the_analytic_displacement():
    """Two epochs of a rendered plane, swept by the restatement and run through the restatement's chain with radius 3, search 4. The median
    error of D against the analytic truth stays below half a pixel of flow and half a plane step of depth at each end:
    0.5 Z / f + 2 * 0.5 Z^2 w_step with Z the farther of the two depths, w_step = 1 / (f * baseline). In the scene whose camera moved and
    whose surface did not, the median |D| stays below the same bound. Measured with this restatement (RMS error of D / median error /
    bound, in world units; a pixel's footprint Z / f is 0.0833 there):
      shifted                          0.0067 / 0.0048 / 0.8750
      shifted and two planes nearer    0.0126 / 0.0078 / 0.8750
      camera moved, surface still      0.0067 / 0.0048 / 0.8750"""
    for name, (a, keep_a, b, keep_b, truth) in scenes().items():
        (P, D, V, score, px), fwd, keep, (Pm, Dm, ok) = FO.surface_displacement(a, keep_a, b, keep_b, 2.0, True, radius=3, search=4)
        Z = 1.0 / min(a["w_true"], b["w_true"])
        bound = 0.5 * Z / DC.F + 2.0 * 0.5 * Z * Z * abs(a["w_step"])
        err = np.linalg.norm(D - truth[px[:, 1], px[:, 0]], axis=1)
        print(f"{name}: lifted {len(D)} of {int(keep_a.sum())} kept, RMS error {np.sqrt((err * err).mean()):.4f}, median {np.median(err):.4f}, bound {bound:.4f}, "
              f"pixel footprint {Z / DC.F:.4f}, median |D| {np.median(np.linalg.norm(D, axis=1)):.4f}")
        assert len(D) > 1000 and np.array_equal(V, D / 2.0)
        assert np.median(err) < bound, (name, float(np.median(err)), bound)
        assert (np.rint(fwd[0][ok != 0]) == SHIFT[0]).all() and (np.rint(fwd[1][ok != 0]) == SHIFT[1]).all()


# ---- (b) the host build of the kernels' rules -----------------------------------------------------------------------------------------------------
def write_records(path):
    n = 0
    with open(path, "wb") as f:
        def head(kind, label):
            f.write(struct.pack("<qq", kind, len(label)) + label.encode())

        def arrays(pairs):
            for a, t in pairs:
                assert a.dtype == t, (a.dtype, t)
                f.write(np.ascontiguousarray(a).tobytes())

        for name, c in C.matches().items():
            head(1, "match " + name)
            f.write(np.asarray([*c["a"].shape, c["r"], c["S"], *c["prior"], c["min_var"], c["ask"] is not None], np.int64).tobytes())
            f.write(np.float64(c["min_score"]).tobytes())
            arrays([(c["a"], np.uint8), (c["b"], np.uint8)] + ([(c["ask"], np.uint8)] if c["ask"] is not None else []))
            arrays(zip(C.match_expected(name), (np.float64, np.float64, np.float32, np.uint8)))
            n += 1
        for name, c in C.checks().items():
            head(2, "check " + name)
            f.write(np.asarray(c["du"].shape, np.int64).tobytes())
            f.write(np.float64(c["tol"]).tobytes())
            arrays([(c[k], t) for k, t in (("du", np.float64), ("dv", np.float64), ("valid", np.uint8), ("du_b", np.float64), ("dv_b", np.float64),
                                           ("valid_b", np.uint8))] + [(C.check_expected(name), np.uint8)])
            n += 1
        for name, c in C.lifts().items():
            head(3, "lift " + name)
            f.write(np.asarray([*c["du"].shape, *c["plane_b"].shape], np.int64).tobytes())
            f.write(np.concatenate([c["cam_a"], c["cam_b"], [c["w_step_b"], c["max_diff"]]]).astype(np.float64).tobytes())
            arrays([(c[k], t) for k, t in (("du", np.float64), ("dv", np.float64), ("valid", np.uint8), ("keep", np.uint8), ("plane_a", np.int16),
                                           ("w_a", np.float64), ("plane_b", np.int16), ("w_b", np.float64), ("keep_b", np.uint8))])
            arrays(zip(C.lift_expected(name), (np.float64, np.float64, np.uint8)))
            n += 1
    return n


@pytest.fixture(scope="module")
def harness_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("flow_host"))
    return d, write_records(os.path.join(d, "records.bin"))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_equals_the_restatement_bit_for_bit(harness_dir, sanitize):
    d, n = harness_dir
    exe = toolchain.host_program(d, "flow_host_harness.cpp", sanitize)
    r = subprocess.run([exe, os.path.join(d, "records.bin")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout[-3000:] + r.stderr[-3000:]
    assert n == len(C.matches()) + len(C.checks()) + len(C.lifts()) and r.stdout.count("\nok ") + r.stdout.startswith("ok ") == n
    assert "DIFFERENT" not in r.stdout and "MISSING" not in r.stdout
    with open(os.path.join(ROOT, "tests", "flow_host_harness.cpp")) as f:
        text = f.read()
    assert '#include "flow_pixel.h"' in text and "#include <hip/" not in text and "int main(" in text      # the stub stands in for the runtime


# ---- (c) the ABI, the kernels' resources, the arguments ---------------------------------------------------------------------------------------------
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
    assert (DF.MAX_RADIUS, DF.MAX_SEARCH, DF.MAX_PRIOR, DF.MAX_MIN_VAR) == (FO.MAX_RADIUS, FO.MAX_SEARCH, FO.MAX_PRIOR, FO.MAX_MIN_VAR) == (15, 16, 4096, 1 << 26)
    with open(os.path.join(toolchain.CSRC, "flow_pixel.h")) as f:
        text = f.read()
    assert "FLOW_MAX_RADIUS = 15, FLOW_MAX_SEARCH = 16, FLOW_MAX_PRIOR = 4096" in text and "static_assert" in text
    assert "fma" not in text and "atomic" not in text and "hipLaunch" not in text and "<<<" not in text      # the arithmetic alone, no launch code
    with open(os.path.join(toolchain.CSRC, "dense_flow.hip")) as f:
        assert "atomic" not in f.read().split("#include", 1)[1]
    for n in ("FlowField", "DisplacementField", "match_flow", "flow_consistency", "lift_flow", "surface_displacement", "displacement_series"):
        assert hasattr(DF, n), n
    assert DF.TABLE_COLS[:13] == DF.F64_COLS and DF.TABLE_COLS[13:] == ("dt", "ep_ini", "ep_fin")


def test_the_kernels_use_no_scratch_memory(tmp_path):
    """Three kernels: no scratch memory. The match kernel sizes its LDS per launch (at most 62800 bytes at r = 15, S = 16: two blocks per
    compute unit; 34832 bytes at r = 7, S = 8: four); its static share is what the block-wide vote takes. At most 128 VGPRs: four waves per
    SIMD, so the registers allow the four blocks that LDS allows at the defaults. Arithmetic on the listing; occupancy was not measured."""
    res = toolchain.kernel_resources(toolchain.device_listing("dense_flow.hip", str(tmp_path)))
    assert len(res) == 3 and all(any(k in name for name in res) for k in ("flow_match_kernel", "flow_check_kernel", "flow_lift_kernel")), sorted(res)
    for k, f in res.items():
        print(k, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "sgpr spills", f["sgpr_spill_count"], "lds", f["group_segment_fixed_size"])
        assert f["vgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (k, dict(f))
        assert f["max_flat_workgroup_size"] == 256 and f["vgpr_count"] <= 128 and f["group_segment_fixed_size"] <= 1024


def lds_bytes(r, S):
    up8 = lambda v: (v + 7) & ~7      # noqa: E731
    return up8((64 + 2 * r) * (16 + 2 * r)) + up8((64 + 2 * (r + S)) * (16 + 2 * (r + S))) + (64 + 2 * S) * (16 + 2 * S) * 8 + (16 + 2 * r) * 64 * 4


def test_the_match_kernels_lds_fits_a_launch_and_a_compute_unit():
    assert lds_bytes(15, 16) == 62800 and lds_bytes(15, 16) + 1024 <= 64 * 1024 and 160 * 1024 // (lds_bytes(15, 16) + 256) == 2
    assert lds_bytes(7, 8) == 34832 and 160 * 1024 // (lds_bytes(7, 8) + 256) == 4
    with open(os.path.join(toolchain.CSRC, "dense_flow.hip")) as f:
        text = f.read()
    assert "62800" in text and "34.8 KB" in text


def grey(h, w):
    import torch
    return torch.zeros((h, w), dtype=torch.uint8)


def a_map(h, w, step=0.01):
    import torch
    from icepy4d_amd.dense import DepthMap
    return DepthMap(torch.zeros((h, w), dtype=torch.int16), torch.zeros((h, w), dtype=torch.float64), torch.zeros((h, w)), None, grey(h, w), np.eye(3),
                    np.eye(3), np.zeros(3), (0.1, step, 5))


def a_field(h, w):
    import torch
    return DF.FlowField(torch.zeros((h, w), dtype=torch.float64), torch.zeros((h, w), dtype=torch.float64), torch.zeros((h, w)), grey(h, w))


MATCH_REFUSALS = [(dict(radius=0), "radius"), (dict(radius=16), "radius"), (dict(radius=1.5), "radius"), (dict(radius=True), "radius"), (dict(search=-1), "search"),
                  (dict(search=17), "search"), (dict(prior=3), "prior"), (dict(prior=(1, 2, 3)), "prior"), (dict(prior=(4097, 0)), "prior"),
                  (dict(prior=(0, -4097)), "prior"), (dict(prior=(0.5, 0)), "prior"), (dict(min_var=-1), "min_var"), (dict(min_var=(1 << 26) + 1), "min_var"),
                  (dict(min_score=float("nan")), "min_score"), (dict(min_score=float("inf")), "min_score"), (dict(min_score="0.8"), "min_score")]
PAIR_REFUSALS = MATCH_REFUSALS + [(dict(tol=0.0), "tol"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(tol=float("inf")), "tol"),
                                  (dict(max_diff=0.0), "max_diff"), (dict(max_diff=float("inf")), "max_diff"), (dict(max_diff="2"), "max_diff"),
                                  (dict(window=3), "unknown options")]


def test_python_layer_refuses_before_any_device_work(monkeypatch):
    import torch
    from icepy4d_amd import engine
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    monkeypatch.setattr(DF, "default_engine", lambda e: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    g = grey(20, 30)
    for bad, text in MATCH_REFUSALS:
        with pytest.raises(ValueError, match=text):
            DF.match_flow(g, g, **bad)
    for args, text in (((g.to(torch.int32), g), "uint8"), ((g, grey(20, 31)), "one shape"), ((g, np.zeros((20, 30), np.uint8)), "uint8"), ((g[0], g[0]), "uint8")):
        with pytest.raises(ValueError, match=text):
            DF.match_flow(*args)
    with pytest.raises(ValueError, match="ask"):
        DF.match_flow(g, g, ask=grey(20, 31))
    with pytest.raises(ValueError, match="ask"):
        DF.match_flow(g, g, ask=g.to(torch.bool))
    f = a_field(20, 30)
    for tol in (0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="tol"):
            DF.flow_consistency(f, f, tol)
    with pytest.raises(ValueError, match="bwd"):
        DF.flow_consistency(f, a_field(20, 31))
    with pytest.raises(ValueError, match="fwd.du"):
        DF.flow_consistency(f._replace(du=f.du.to(torch.float32)), f)
    with pytest.raises(ValueError, match="FlowField"):
        DF.flow_consistency((f.du, f.dv, f.score, f.valid), f)
    m = a_map(20, 30)
    for max_diff in (0.0, -2.0, float("nan"), float("inf"), "2"):
        with pytest.raises(ValueError, match="max_diff"):
            DF.lift_flow(f, g, m, m, g, max_diff)
    for step in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="w_step"):
            DF.lift_flow(f, g, m, a_map(20, 30, step), g)
    with pytest.raises(ValueError, match="field"):
        DF.lift_flow(a_field(20, 31), g, m, m, g)
    with pytest.raises(ValueError, match="keep_b"):
        DF.lift_flow(f, g, m, a_map(22, 30), g)
    with pytest.raises(ValueError, match="keep "):
        DF.lift_flow(f, g.to(torch.int16), m, m, g)
    with pytest.raises(ValueError, match="map_a.w"):
        DF.lift_flow(f, g, m._replace(w=m.w.to(torch.float32)), m, g)
    with pytest.raises(ValueError, match="map_b.K"):
        DF.lift_flow(f, g, m, m._replace(K=np.full((3, 3), np.nan)), g)
    for schedule in (None, (0.1, 0.01), (0.1, "0.01", 5), 3.0):
        with pytest.raises(ValueError, match="map_b.schedule"):
            DF.lift_flow(f, g, m, m._replace(schedule=schedule), g)
        with pytest.raises(ValueError, match="map_a.schedule"):
            DF.surface_displacement(m._replace(schedule=schedule), g, m, g, 1.0)
    for bad, text in PAIR_REFUSALS:
        with pytest.raises(ValueError, match=text):
            DF.surface_displacement(m, g, m, g, 1.0, **bad)
        with pytest.raises(ValueError, match=text):
            DF.displacement_series([[m, m], [m, m]], [[g, g], [g, g]], [0, 1], **bad)
    for dt in (0, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="dt_days"):
            DF.surface_displacement(m, g, m, g, dt)
    with pytest.raises(ValueError, match="one shape"):
        DF.surface_displacement(m, g, a_map(20, 31), grey(20, 31), 1.0)
    with pytest.raises(ValueError, match="grey"):
        DF.surface_displacement(m._replace(grey=None), g, m, g, 1.0)
    with pytest.raises(ValueError, match="keep_a"):
        DF.surface_displacement(m, grey(20, 31), m, g, 1.0)
    pair, keeps = [[m, m], [m, m], [m, m]], [[g, g]] * 3
    for bad, text in ((dict(lag=0), "lag"), (dict(lag=3), "lag"), (dict(camera=2), "camera"), (dict(dates=[0, 1]), "epochs"), (dict(dates=[0, 0, 1]), "dt_days"),
                      (dict(dates=[0, "tomorrow", 2]), "does not match format"), (dict(dates=[0, None, 2]), "a date")):
        args = dict(maps=pair, keeps=keeps, dates=[0, 1, 2])
        args.update(bad)
        with pytest.raises(ValueError, match=text):
            DF.displacement_series(**args)
    with pytest.raises(ValueError, match="epochs"):
        DF.displacement_series([[m, m]], [[g, g]], [0])


def test_day_numbers():
    import datetime
    assert DF.day_number(3) == 3.0 and DF.day_number(2.5) == 2.5
    assert DF.day_number("2022_05_02") - DF.day_number("2022_05_01") == 1.0
    assert DF.day_number(datetime.date(2022, 5, 3)) - DF.day_number("2022_05_01") == 2.0
    assert DF.day_number(datetime.datetime(2022, 5, 1, 12)) - DF.day_number(datetime.date(2022, 5, 1)) == 0.5
