"""Coarse-to-fine dense displacement without a device: (a) the cases reach what they are named for, the tiles' paths included, and the
consequences of the definition on scenes whose truth is known, all in the restatement (tests/pyrflow_oracle.py); (b) a host build of the
kernels' own rules (csrc/flow_field_pixel.h and csrc/flow_pixel.h behind the stub <hip/hip_runtime.h>, in
tests/flow_field_host_harness.cpp, a stand-alone program built plain and with the address and undefined-behaviour sanitizers) against the
restatement bit for bit; (c) the ABI, the compiled resources of the kernels and the arguments that `icepy4d_amd.dense_flow` refuses. The
device run is tests/test_gpu_pyrflow.py."""
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
import flow_oracle as FO  # noqa: E402
import pyrflow_cases as C  # noqa: E402
import pyrflow_oracle as PO  # noqa: E402
from test_flow_cpu import PAIR_REFUSALS, a_field, a_map, grey  # noqa: E402

from icepy4d_amd import dense_flow as DF  # noqa: E402
from icepy4d_amd.dense_flow import PriorField, match_flow_field, match_flow_pyramid, prior_field_up  # noqa: E402,F401  (the feature under test)

NAMES = ["im_flow_prior_up", "im_flow_match_field"]


# ---- (a) the cases and the restatement ------------------------------------------------------------------------------------------------------------
def test_the_prior_cases_reach_what_they_are_named_for():
    u, E = C.ups(), C.up_expected
    assert {(c["du"].shape, c["shape"]) for c in u.values()} >= set(C.SHAPES_UP)
    assert {c["m"] for c in u.values()} == {0, 1, 2} and {(c["m"], c["min_count"]) for c in u.values()} >= {(0, 1), (1, 1), (1, 9), (2, 1), (2, 25)}
    for name, c in u.items():
        pu, pv, have = E(name)
        assert pu.shape == pv.shape == have.shape == c["shape"] and pu.dtype == pv.dtype == np.int16 and have.dtype == np.uint8, name
        assert not pu[have == 0].any() and not pv[have == 0].any() and np.abs(pu).max(initial=0) <= 4096 and np.abs(pv).max(initial=0) <= 4096, name
    name = "up_17x49_to_33x97_m1_count1"
    assert 0.9 < E(name)[2].mean() <= 1.0 and 0 < E("up_17x49_to_33x97_m2_count25")[2].mean() < 0.2 < E("up_17x49_to_33x97_m0_count1")[2].mean() < 0.95
    assert not any(a.any() for a in E("no_valid_pixel"))
    for m in (0, 1, 2):                                   # the fine pixels whose parent lies within m of coarse pixel (20, 4): a square of 2 (2 m + 1)
        pu, pv, have = E(f"one_valid_pixel_m{m}")
        at = (slice(2 * (4 - m), 2 * (4 + m) + 2), slice(2 * (20 - m), 2 * (20 + m) + 2))
        assert have.sum() == (2 * (2 * m + 1)) ** 2 and have[at].all() and (pu[at] == 6).all() and (pv[at] == -6).all()      # 6.5 -> 6, -5.5 -> -6: ties to even
    c = u["nan_and_infinity_under_valid"]
    assert np.isnan(c["du"]).sum() > 20 and np.isinf(c["dv"]).sum() > 20 and c["valid"].all()
    bad = ~(np.isfinite(c["du"]) & np.isfinite(c["dv"]))
    have0 = E("nan_and_infinity_under_valid_m0")[2]
    assert np.array_equal(have0[::2, ::2][:9, :33] != 0, ~bad) and E("nan_and_infinity_under_valid")[2].all()
    assert 0 < E("nan_and_infinity_under_valid_m2_count20")[2].mean() < 1
    pu, pv, have = E("medians_at_half")
    assert have.all() and pu[0, 0:12:2].tolist() == [2, 4, 0, -6, 0, 4] and pv[0, 0:12:2].tolist() == [-2, -4, 0, 6, 0, -4]
    for axis, name in enumerate(("twice_the_median_at_4096_and_beyond_along_u", "twice_the_median_at_4096_and_beyond_along_v")):
        out = E(name)
        assert out[2][0, 0:20:2].tolist() == [1, 1, 0, 1, 1, 0, 0, 0, 0, 1] and out[axis][0, 0:20:2].tolist() == [4096, 4096, 0, -4096, -4096, 0, 0, 0, 0, 10]
        assert out[1 - axis][0, 0:20:2].tolist() == [v * (2 if axis == 0 else -2) for v in out[2][0, 0:20:2].tolist()]      # no prior: both are zero
    pu, pv, have = E("an_even_count_takes_the_lower_median")
    assert pu[8, 21] == 6 and pv[8, 21] == -14 and pu[5, 50] == -18 and pv[5, 50] == 10 and have[8, 21] and have[5, 50]      # the lower of (3, 7), (-7, -3), ...
    assert not have[8, 26] and have.sum() > 0                                      # a single neighbour is fewer than min_count = 2


def test_the_field_cases_reach_what_they_are_named_for():
    f, E, P = C.fields(), C.field_expected, C.field_paths
    assert {(15, 63), (16, 64), (17, 65), (33, 97), (1, 70), (70, 1), (5, 9), (40, 80)} <= {c["a"].shape for c in f.values()}
    assert {c["r"] for c in f.values()} >= {1, 3, 7, 15} and {c["S"] for c in f.values()} >= {0, 1, 2, 16}
    assert [n for n, c in f.items() if (c["r"], c["S"]) == (15, 16)] == ["constant_largest_r15_S16_40x80"]
    for name, c in f.items():
        assert c["pu"].dtype == c["pv"].dtype == np.int16 and c["have"].dtype == np.uint8 and c["pu"].shape == c["a"].shape == c["b"].shape, name
        e = E(name)
        assert not e[3][~PO.wanted(c["pu"], c["pv"], c["have"], c["ask"])].any(), name
        if C.is_constant(c):                              # a constant field is the single-level match with that prior
            want = FO.match(c["a"], c["b"], None, c["r"], c["S"], (int(c["pu"][0, 0]), int(c["pv"][0, 0])), c["min_var"], c["min_score"])
            assert all(np.array_equal(g, x) for g, x in zip(e, want)) and set(P(name).ravel().tolist()) <= {0, 1}, name
    assert sum(C.is_constant(c) for c in f.values()) == 11
    for name in ("constant_15x63_r1_S0", "constant_16x64_r3_S1", "constant_33x97_r3_S2", "constant_17x65_r1_S16", "constant_33x97_r15_S1"):
        assert E(name)[3].sum() > 150, name
    for name in ("constant_1x70", "constant_70x1", "constant_5x9_smaller_than_the_window", "have_all_zero", "priors_push_every_window_out"):
        assert not any(a.any() for a in E(name)), name
    assert not P("have_all_zero").any() and not P("constant_1x70").any() and (P("priors_push_every_window_out") == 1).all()
    # two priors in one tile: tiled, and each side finds its own shift
    for name, axis, sides in (("two_priors_split_along_x", 0, ((slice(3, 30), slice(4, 24), 6), (slice(3, 30), slice(42, 90), 2))),
                              ("two_priors_split_along_y", 1, ((slice(3, 5), slice(3, 94), 3), (slice(12, 30), slice(3, 94), -1)))):
        e, c = E(name), f[name]
        assert (P(name)[:2] == 1).all() and len(np.unique(c["pu" if axis == 0 else "pv"][:16, :64])) == 2, name
        for ys, xs, shift in sides:
            k = e[3][ys, xs] != 0
            assert k.mean() > 0.8 and (np.rint(e[axis][ys, xs][k]) == shift).mean() > 0.95, (name, shift)
    E_ = PO.spread(3, 2)
    assert E_ == 8 and PO.spread(15, 8) == 8 and PO.spread(15, 16) == 1 and PO.spread(14, 16) == 2 and PO.spread(7, 2) == 8
    for axis in ("x", "y"):
        at, beyond = f[f"spread_at_the_limit_along_{axis}"], f[f"spread_one_beyond_the_limit_along_{axis}"]
        k = "pu" if axis == "x" else "pv"
        assert int(at[k][:16, :64].max()) - int(at[k][:16, :64].min()) == E_ and int(beyond[k][:16, :64].max()) - int(beyond[k][:16, :64].min()) == E_ + 1
        assert (P(f"spread_at_the_limit_along_{axis}")[:2] == 1).all() and (P(f"spread_one_beyond_the_limit_along_{axis}")[:2] == 2).all()
        assert E(f"spread_at_the_limit_along_{axis}")[3].sum() > 1500
    assert (P("spread_at_the_limit_8_of_r15_S8") == 1).all() and (P("spread_one_beyond_the_limit_8_of_r15_S8")[:, 0] == 2).all()
    for name in ("random_field_of_wide_spread", "random_field_of_wide_spread_r1_S16"):
        assert (P(name)[:2] == 2).all() and E(name)[3].sum() > 1000, name
    c = f["have_one_pixel_per_tile"]
    assert c["have"].sum() == 6 and all(c["have"][y0:y0 + 16, x0:x0 + 64].sum() == 1 for y0 in (0, 16, 32) for x0 in (0, 64))
    assert P("have_one_pixel_per_tile").tolist() == [[1, 1], [1, 1], [0, 0]] and 0 < E("have_one_pixel_per_tile")[3].sum() <= 4
    c, e = f["ask_crossed_with_have"], E("ask_crossed_with_have")
    assert not c["ask"][:, 64:].any() and (P("ask_crossed_with_have")[:, 1] == 0).all() and 200 < e[3].sum() and ((c["have"] > 1) & (c["ask"] > 1)).sum() > 100
    assert not e[3][(c["have"] == 0) | (c["ask"] == 0)].any()
    c, e = f["priors_at_4096_and_beyond"], E("priors_at_4096_and_beyond")
    assert {4096, -4096, 4097, -4097, 32767, -32768, 0} == set(c["pu"].ravel().tolist()) == set(c["pv"].ravel().tolist())
    assert (P("priors_at_4096_and_beyond")[0] == 2).all() and e[3].sum() > 10 and not e[3][(c["pu"] != 0) | (c["pv"] != 0)].any()
    c, e = f["priors_beyond_4096_only_and_zero"], E("priors_beyond_4096_only_and_zero")
    assert (P("priors_beyond_4096_only_and_zero") == 1).all() and e[3].sum() > 100 and not e[3][(c["pu"] != 0) | (c["pv"] != 0)].any()
    e = E("priors_leave_a_strip")
    assert 0 < e[3].sum() < 250 and not e[3][:, 12:].any()
    # the periodic texture: each pixel's tie goes to the displacement nearest its own prior, which is the prior itself
    c, e = f["periodic_tie_under_priors_-3_0_3"], E("periodic_tie_under_priors_-3_0_3")
    inner = (slice(2, -2), slice(9, -9))
    assert set(c["pu"].ravel().tolist()) == {-3, 0, 3} and e[3][inner].all() and np.array_equal(np.rint(e[0][inner]), c["pu"][inner].astype(np.float64))
    c, e = f["best_on_the_rim_of_the_own_range"], E("best_on_the_rim_of_the_own_range")
    k = np.zeros((20, 70), bool)
    k[4:16, 8:60] = True
    k &= e[3] != 0
    assert k.sum() > 400 and (e[0][k] == 4.0).all() and (e[1][k & (c["pu"] == 6)] == 1.0).all()      # whole pixels: no offset on the rim
    assert (e[1][k & (c["pu"] == 2)] != 1.0).mean() > 0.9                          # the axis that is not on the rim does take its offset


def inner_of(shape, r, shift):
    h, w = shape
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    sx, sy = shift
    return (uu >= r) & (uu < w - r) & (vv >= r) & (vv < h - r) & (uu + sx >= r) & (uu + sx < w - r) & (vv + sy >= r) & (vv + sy < h - r)


def share_at(field, inner, shift):
    return float(((field[3] != 0) & (np.rint(field[0]) == shift[0]) & (np.rint(field[1]) == shift[1]))[inner].mean())


def test_whole_image_shifts_beyond_the_single_levels_reach_are_found():
    """Whole-image shifts of the octave texture on 65 x 193 with noise of sigma 2 on b and min_score 0.5. Every shift lies beyond `search`,
    so the single-level match with the same radius and search finds none of the inner pixels (those whose window and whose true partner's
    window lie inside the images); the pyramid finds more than half. A shift of exactly the reach 2^(L-1) search + (2^(L-1) - 1) fine_search
    is found and one pixel farther is not. Measured in this restatement (share of inner pixels valid at the true shift; levels, radius,
    search, fine_search):
      (21, -11)  3, 3, 4, 2   0.700      (13, -9)  3, 2, 3, 1   0.940      (6, -5)  2, 3, 4, 1   0.963
      (19, -11)  3, 3, 4, 1   0.915  (the reach is 19)          (20, -11)  3, 3, 4, 1   0.000
    About one tile in two of level 0 takes the direct path at this size: the rim of a 65 x 193 image is most of it."""
    seen = set()
    for name, (shift, levels, r, S, fine) in C.SHIFTS.items():
        c, (field, trace) = C.pyramids()[name], C.pyramid_expected(name)
        inner = inner_of(c["a"].shape, r, shift)
        single = FO.match(c["a"], c["b"], None, r, S, (0, 0), c["min_var"], c["min_score"])
        found = share_at(field, inner, shift)
        print(f"{name}: reach {PO.reach(levels, S, fine)}, inner {int(inner.sum())}, pyramid {found:.3f}, single level {share_at(single, inner, shift):.3f}; tiles of "
              f"level 0 on paths 0/1/2: {[int((trace[-1][2] == k).sum()) for k in (0, 1, 2)]}")
        assert max(abs(shift[0]), abs(shift[1])) > S and inner.sum() > 5000 and share_at(single, inner, shift) == 0.0, name
        assert [t[0] for t in trace] == list(range(levels - 2, -1, -1)) and 2 in trace[-1][2], name
        seen |= set(trace[-1][2].ravel().tolist())
        if name == "shift_20_-11_beyond_the_reach":
            assert PO.reach(levels, S, fine) == 19 and found == 0.0
        else:
            assert max(abs(shift[0]), abs(shift[1])) <= PO.reach(levels, S, fine) and found > 0.5, (name, found)
    assert seen == {0, 1, 2}
    assert PO.reach(3, 4, 1) == 19 == max(C.SHIFTS["shift_19_-11_at_the_reach"][0])
    assert [PO.coarse_prior(p, 3) for p in (0, 1, 2, 3, 5, 6, 7, 10, -2, -6, -10, -11)] == [0, 0, 0, 1, 1, 2, 2, 2, 0, -2, -2, -3]      # ties to even
    assert [DF.coarse_prior(p, L) for p in range(-40, 41) for L in (1, 2, 3, 6)] == [PO.coarse_prior(p, L) for p in range(-40, 41) for L in (1, 2, 3, 6)]
    assert all(PO.coarse_prior(p, L) == int(np.rint(p / 2.0 ** (L - 1))) for p in range(-4096, 4097, 7) for L in range(1, 7))


def test_a_shear_gives_each_side_its_own_shift():
    """64 x 256, 3 levels, radius 3, search 4, fine_search 2: the left half moves by 20 or 16 px, the right half by 2 px; no single prior
    serves both at search 4. Of the valid pixels of either side (away from the seam and from what the fast side covers) the share at the
    side's own shift, measured in this restatement: 20 against 2: 0.908 fast, 0.998 slow; 16 against 2: 1.000 fast, 0.998 slow. Over eight
    texture seeds the fast side at 20 px gave 0.896 to 0.982: 20 px is 5 px on the coarsest level, one beyond its search of 4, so that
    level finds the rim of its range at best and the finer levels make up the rest. 16 px is 4 px there and lies inside. The fast side at
    20 px is therefore asserted at 0.8 and everything else at 0.9."""
    for name, fast, floor in (("shear_20_against_2", 20, 0.8), ("shear_16_against_2", 16, 0.9)):
        c, (field, trace) = C.pyramids()[name], C.pyramid_expected(name)
        h, w = c["a"].shape
        r = c["r"]
        uu, vv = np.meshgrid(np.arange(w), np.arange(h))
        rows = (vv >= r) & (vv < h - r)
        got = []
        for side, shift in (((uu >= r) & (uu < w // 2 - r), fast), ((uu >= w // 2 + r + fast) & (uu < w - r - 2), 2)):
            k = side & rows
            v = k & (field[3] != 0)
            got += [v.sum() / k.sum(), float(((np.rint(field[0]) == shift) & (np.rint(field[1]) == 0))[v].mean())]
        print(f"{name}: fast side valid {got[0]:.3f}, at its shift {got[1]:.3f}; slow side valid {got[2]:.3f}, at its shift {got[3]:.3f}")
        single = FO.match(c["a"], c["b"], None, r, c["S"], (0, 0), c["min_var"], c["min_score"])
        assert not ((single[3] != 0) & (np.rint(single[0]) == fast))[rows & (uu < w // 2 - r)].any()      # the single level cannot reach the fast side
        assert got[0] > 0.7 and got[2] > 0.7 and got[1] > floor and got[3] > 0.9, (name, got)


def test_a_gradient_is_followed_within_a_pixel():
    """A displacement growing linearly from 0 to 24 px across 64 x 256 (3 levels, radius 3, search 4, fine_search 2). Measured in this
    restatement: 0.985 of the valid inner pixels within 1 px of the truth, median error 0.093 px; the single-level match at search 8
    reaches 0.426 and a median error of 9.0 px. The tiles of level 0 span up to 6 px of priors: 12 of 16 take the tiled path."""
    c, (field, trace) = C.pyramids()["gradient_0_to_24"], C.pyramid_expected("gradient_0_to_24")
    _, _, d = C.stretched(912, 64, 256, 24.0)
    h, w = c["a"].shape
    r = c["r"]
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    inner = (uu >= r) & (uu < w - r - 24) & (vv >= r) & (vv < h - r)
    v = inner & (field[3] != 0)
    err = np.hypot(field[0] - d[None, :], field[1])
    single = FO.match(c["a"], c["b"], None, r, 8, (0, 0), c["min_var"], c["min_score"])
    v1 = inner & (single[3] != 0)
    e1 = np.hypot(single[0] - d[None, :], single[1])
    print(f"pyramid: valid {v.sum() / inner.sum():.3f}, within 1 px {(err[v] <= 1.0).mean():.3f}, median {np.median(err[v]):.3f} px; single level at search 8: "
          f"within 1 px {(e1[v1] <= 1.0).mean():.3f}, median {np.median(e1[v1]):.3f} px; level 0 tiles on paths 0/1/2 {[int((trace[-1][2] == k).sum()) for k in (0, 1, 2)]}")
    assert v.sum() > 0.7 * inner.sum() and (err[v] <= 1.0).mean() > 0.9 and np.median(err[v]) < 0.25
    assert (e1[v1] <= 1.0).mean() < 0.6 and (trace[-1][2] == 1).sum() >= 8


def test_the_octave_texture_survives_the_pyramid_and_the_sweeps_texture_does_not():
    import dense_cases as DC
    from oracle.pyramid_cpu import pyr_down
    flat, rich = DC.texture(5, 64, 192), C.octaves(5, 64, 192)
    std = lambda a: a.astype(np.float64).std()      # noqa: E731
    before = std(flat), std(rich)
    for _ in range(2):
        flat, rich = pyr_down(flat), pyr_down(rich)
    print(f"contrast left on level 2: the sweep's texture {std(flat) / before[0]:.2f}, the octave texture {std(rich) / before[1]:.2f}")      # 0.32 and 0.66
    assert std(flat) < 0.4 * before[0] and std(rich) > 0.6 * before[1]
    assert PO.levels_of(C.octaves(6, 65, 193), 3)[2].shape == (17, 49) and DF.level_shapes((65, 193), 3) == [(65, 193), (33, 97), (17, 49)]


# ---- (b) the host build of the kernels' rules -----------------------------------------------------------------------------------------------------
SPREADS = [(r, S) for r in range(1, 16) for S in range(0, 17)]


def write_records(path):
    n = 0
    with open(path, "wb") as f:
        def head(kind, label):
            f.write(struct.pack("<qq", kind, len(label)) + label.encode())

        def arrays(pairs):
            for a, t in pairs:
                assert a.dtype == t, (a.dtype, t)
                f.write(np.ascontiguousarray(a).tobytes())

        for name, c in C.ups().items():
            head(1, "prior_up " + name)
            f.write(np.asarray([*c["du"].shape, *c["shape"], c["m"], c["min_count"]], np.int64).tobytes())
            arrays([(c["du"], np.float64), (c["dv"], np.float64), (c["valid"], np.uint8)])
            arrays(zip(C.up_expected(name), (np.int16, np.int16, np.uint8)))
            n += 1
        for name, c in C.fields().items():
            head(2, "field " + name)
            f.write(np.asarray([*c["a"].shape, c["r"], c["S"], c["min_var"], c["ask"] is not None], np.int64).tobytes())
            f.write(np.float64(c["min_score"]).tobytes())
            arrays([(c["a"], np.uint8), (c["b"], np.uint8), (c["pu"], np.int16), (c["pv"], np.int16), (c["have"], np.uint8)]
                   + ([(c["ask"], np.uint8)] if c["ask"] is not None else []))
            arrays(zip(C.field_expected(name), (np.float64, np.float64, np.float32, np.uint8)))
            n += 1
        head(3, "spread of every r and S")
        f.write(np.asarray([len(SPREADS)] + [v for r, S in SPREADS for v in (r, S, PO.spread(r, S), PO.lds_bytes(r, S, PO.spread(r, S), PO.spread(r, S)))],
                           np.int64).tobytes())
        n += 1
    return n


@pytest.fixture(scope="module")
def harness_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("flow_field_host"))
    return d, write_records(os.path.join(d, "records.bin"))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_equals_the_restatement_bit_for_bit(harness_dir, sanitize):
    d, n = harness_dir
    exe = toolchain.host_program(d, "flow_field_host_harness.cpp", sanitize)
    r = subprocess.run([exe, os.path.join(d, "records.bin")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout[-3000:] + r.stderr[-3000:]
    assert n == len(C.ups()) + len(C.fields()) + 1 and r.stdout.count("\nok ") + r.stdout.startswith("ok ") == n
    assert "DIFFERENT" not in r.stdout and "MISSING" not in r.stdout
    with open(os.path.join(ROOT, "tests", "flow_field_host_harness.cpp")) as f:
        text = f.read()
    assert '#include "flow_field_pixel.h"' in text and "#include <hip/" not in text and "int main(" in text      # the stub stands in for the runtime


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
    assert (DF.MAX_LEVELS, DF.MAX_MEDIAN_RADIUS) == (PO.MAX_LEVELS, PO.MAX_MEDIAN_RADIUS) == (6, 2)
    with open(os.path.join(toolchain.CSRC, "flow_field_pixel.h")) as f:
        text = f.read()
    assert "FLOW_FIELD_MAX_SPREAD = 8" in text and "FLOW_FIELD_LDS_BUDGET = 64 * 1024 - 1024" in text and "FLOW_MAX_MEDIAN_RADIUS = 2" in text
    assert (PO.MAX_SPREAD, PO.LDS_BUDGET) == (8, 64512)
    assert "fma" not in text and "atomic" not in text and "hipLaunch" not in text and "<<<" not in text and "threadIdx" not in text      # no launch code
    with open(os.path.join(toolchain.CSRC, "dense_flow_field.hip")) as f:
        code = f.read().split("#include", 1)[1]
    assert "atomic" not in code and '#include "dense_tile.h"' in "#include" + code and "DENSE_REFUSED" in code and "flow_match_pixel(" in code
    for n in ("PriorField", "prior_field_up", "match_flow_field", "match_flow_pyramid", "level_shapes", "coarse_prior"):
        assert hasattr(DF, n), n
    assert DF.OPTIONS[:7] == ("radius", "search", "prior", "min_var", "min_score", "tol", "max_diff") and set(DF.OPTIONS[7:]) == {"levels", "fine_search", "median_radius", "min_count"}


def test_the_kernels_use_no_scratch_memory(tmp_path):
    """The match kernel and the three forms of the prior kernel (median_radius 0, 1, 2): no scratch memory and no spilled VGPR - the median
    of 25 values per axis is taken by ranks in registers. The match kernel sizes its LDS per launch; its static share is the fold of the
    box of priors over the block's four waves. At most 168 VGPRs: three waves per SIMD, so three blocks per compute unit by registers,
    where LDS allows five at radius 7, fine_search 2. Arithmetic on the listing; occupancy was not measured."""
    res = toolchain.kernel_resources(toolchain.device_listing("dense_flow_field.hip", str(tmp_path)))
    assert len(res) == 4 and sum("flow_match_field_kernel" in k for k in res) == 1 and sum("flow_prior_up_kernel" in k for k in res) == 3, sorted(res)
    for k, f in res.items():
        print(k, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "sgpr spills", f["sgpr_spill_count"], "lds", f["group_segment_fixed_size"])
        assert f["vgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (k, dict(f))
        assert f["max_flat_workgroup_size"] == 256 and f["vgpr_count"] <= 168 and f["group_segment_fixed_size"] <= 1024


def test_the_match_kernels_lds_fits_a_launch_and_a_compute_unit():
    sizes = {(r, S): PO.lds_bytes(r, S, PO.spread(r, S), PO.spread(r, S)) for r, S in SPREADS}
    worst = max(sizes.values())
    assert worst == 64344 == sizes[(14, 16)] == sizes[(14, 13)] and worst + 1024 <= 64 * 1024 and PO.lds_bytes(15, 16, 0, 0) == 62800 and sizes[(15, 16)] == 64168
    assert PO.lds_bytes(7, 2, 8, 8) == 30832 and PO.spread(7, 2) == 8 and 160 * 1024 // (30832 + 256) == 5
    assert all(PO.spread(r, S) == 8 for r in range(1, 16) for S in range(0, 9))      # every fine_search up to 8 keeps the whole spread
    # a box of zero spread is flow_match_kernel's own layout
    from test_flow_cpu import lds_bytes
    assert all(PO.lds_bytes(r, S, 0, 0) == lds_bytes(r, S) for r, S in SPREADS)
    with open(os.path.join(toolchain.CSRC, "dense_flow_field.hip")) as f:
        text = f.read()
    assert "64344" in text and "30.8 KB" in text and "62800" in text


PYRAMID_REFUSALS = [(dict(levels=0), "levels"), (dict(levels=7), "levels"), (dict(levels=2.5), "levels"), (dict(levels=True), "levels"), (dict(levels=None), "levels"),
                    (dict(fine_search=-1), "fine_search"), (dict(fine_search=17), "fine_search"), (dict(fine_search=1.5), "fine_search"),
                    (dict(median_radius=-1), "median_radius"), (dict(median_radius=3), "median_radius"), (dict(min_count=0), "min_count"),
                    (dict(min_count=10), "min_count"), (dict(median_radius=0, min_count=2), "min_count"), (dict(median_radius=2, min_count=26), "min_count"),
                    (dict(levels=2, radius=7), "levels = 2"), (dict(levels=3, radius=3), "levels = 3"), (dict(levels=6, radius=1), "levels = 6")]


def a_prior(h, w):
    import torch
    return PriorField(torch.zeros((h, w), dtype=torch.int16), torch.zeros((h, w), dtype=torch.int16), grey(h, w))


def test_python_layer_refuses_before_any_device_work(monkeypatch):
    import torch
    from icepy4d_amd import engine
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    monkeypatch.setattr(DF, "default_engine", lambda e: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    g, m = grey(20, 30), a_map(20, 30)                     # the coarsest of two levels is 10 x 15: too small for radius 7, enough for radius 4
    for bad, text in PYRAMID_REFUSALS:
        with pytest.raises(ValueError, match=text):
            DF.match_flow_pyramid(g, g, **bad)
        with pytest.raises(ValueError, match=text):
            DF.surface_displacement(m, g, m, g, 1.0, **bad)
        with pytest.raises(ValueError, match=text):
            DF.displacement_series([[m, m], [m, m]], [[g, g], [g, g]], [0, 1], **bad)
    for bad, text in PAIR_REFUSALS:                        # what was refused is refused with the new options beside it
        with pytest.raises(ValueError, match=text):
            DF.surface_displacement(m, g, m, g, 1.0, levels=2, radius=bad.get("radius", 3), **{k: v for k, v in bad.items() if k != "radius"})
    with pytest.raises(ValueError, match="unknown options"):
        DF.surface_displacement(m, g, m, g, 1.0, window=3)
    for bad, text in ((dict(radius=0), "radius"), (dict(search=17), "search"), (dict(prior=(4097, 0)), "prior"), (dict(min_var=-1), "min_var"),
                      (dict(min_score=float("nan")), "min_score"), (dict(ask=grey(20, 31)), "ask")):
        with pytest.raises(ValueError, match=text):
            DF.match_flow_pyramid(g, g, **bad)
    for args, text in (((g.to(torch.int32), g), "uint8"), ((g, grey(20, 31)), "one shape")):
        with pytest.raises(ValueError, match=text):
            DF.match_flow_pyramid(*args)
        with pytest.raises(ValueError, match=text):
            DF.match_flow_field(*args, a_prior(20, 30))
    # the field match
    pf = a_prior(20, 30)
    for bad, text in ((dict(radius=0), "radius"), (dict(radius=16), "radius"), (dict(search=-1), "search"), (dict(search=17), "search"), (dict(min_var=-1), "min_var"),
                      (dict(min_score=float("inf")), "min_score"), (dict(ask=grey(20, 31)), "ask"), (dict(tile_path=grey(2, 2)), "tile_path")):
        with pytest.raises(ValueError, match=text):
            DF.match_flow_field(g, g, pf, **bad)
    for bad, text in ((a_prior(20, 31), "prior_field.pu"), (pf._replace(pv=pf.pv.to(torch.int32)), "prior_field.pv"), (pf._replace(have=pf.have.to(torch.bool)), "prior_field.have"),
                      ((pf.pu, pf.pv, pf.have), "PriorField"), (None, "PriorField")):
        with pytest.raises(ValueError, match=text):
            DF.match_flow_field(g, g, bad)
    # the prior of a level
    f = a_field(10, 15)
    for args, text in (((f, (20, 31)), "10 x 16"), ((f, (21, 30)), "11 x 15"), ((f, (20, 30), 3), "median_radius"), ((f, (20, 30), -1), "median_radius"),
                       ((f, (20, 30), 1, 0), "min_count"), ((f, (20, 30), 1, 10), "min_count"), ((f, (20, 30), 0, 2), "min_count"), ((f, 20), "shape"),
                       ((f, (0, 30)), "sides"), (((f.du, f.dv, f.score, f.valid), (20, 30)), "FlowField"), ((f._replace(du=f.du.to(torch.float32)), (20, 30)), "field.du")):
        with pytest.raises(ValueError, match=text):
            DF.prior_field_up(*args)


def test_one_level_makes_todays_calls_and_never_reaches_the_new_names(monkeypatch):
    """`levels=1`, given or left out, calls `match_flow` with exactly the arguments of before and none of the new functions."""
    import torch
    calls = []

    def fake_match(a, b, **k):
        calls.append(k)
        h, w = a.shape
        return DF.FlowField(torch.zeros((h, w), dtype=torch.float64), torch.zeros((h, w), dtype=torch.float64), torch.zeros((h, w)), torch.zeros((h, w), dtype=torch.uint8))

    def never(*a, **k):
        raise AssertionError("a new entry point was reached")

    monkeypatch.setattr(DF, "default_engine", lambda e: "the engine")
    monkeypatch.setattr(DF, "match_flow", fake_match)
    monkeypatch.setattr(DF, "flow_consistency", lambda fwd, bwd, tol, engine=None: fwd.valid)
    monkeypatch.setattr(DF, "lift_flow", lambda field, keep, ma, mb, kb, max_diff, engine=None: (torch.zeros((*keep.shape, 3), dtype=torch.float64),
                                                                                                 torch.zeros((*keep.shape, 3), dtype=torch.float64), keep))
    for name in ("match_flow_pyramid", "match_flow_field", "prior_field_up", "_pyr_down"):
        monkeypatch.setattr(DF, name, never)
    g, m = grey(20, 30), a_map(20, 30)
    for options in (dict(), dict(levels=1), dict(levels=1, fine_search=5, median_radius=2, min_count=7)):
        calls.clear()
        out = DF.surface_displacement(m, g, m, g, 1.0, prior=(3, -2), search=5, **options)
        assert len(out.points) == 0 and len(calls) == 2
        assert calls[0].pop("ask") is g and calls[0] == dict(prior=(3, -2), radius=7, search=5, min_var=4, min_score=0.8, engine="the engine")
        assert calls[1] == dict(prior=(-3, 2), radius=7, search=5, min_var=4, min_score=0.8, engine="the engine")
    small = a_map(5, 9)                                    # smaller than the window: one level takes it as ever
    assert len(DF.surface_displacement(small, grey(5, 9), small, grey(5, 9), 1.0).points) == 0
