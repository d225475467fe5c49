"""Template matching without a device: (a) the numpy restatement (tests/tm_oracle.py) against independent arithmetic: its emulated fused
multiply-add against the C library's, its C against the float64 sum of the plain definition within the derived rounding bound, its sums
against numpy's own, its argmax against np.argmax; (b) the case list (tests/tm_cases.py) reaches what it names; (c) a host build of the
kernels' own arithmetic (csrc/tm_pair.h behind the stub <hip/hip_runtime.h>, in tests/tm_host_harness.cpp, a stand-alone program built
plain and with the address and undefined-behaviour sanitizers) against the restatement bit for bit: the plan for every 1 <= T <= 300 and
T < S <= T + 300 and a sparse set up to (2048, 4096), the window rule, forient, every element of C, the wave's reduction and the peak
tail on every case. The device run is tests/test_gpu_templatematch_edges.py."""
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
import oc_oracle  # noqa: E402
import tm_cases as TC  # noqa: E402
import tm_oracle as O  # noqa: E402

F32 = np.float32
NONFINITE = [n for n in TC.cases() if n.startswith("nonfinite_") and n not in ("nonfinite_none", "nonfinite_nan_just_outside_both_windows")]


def window_of(c, i, w):
    T, S = c["T"], c["S"]
    return (c["A"][w["arow"]:w["arow"] + T, w["acol"]:w["acol"] + T],
            c["B"][int(c["bidx"][i])][w["brow"]:w["brow"] + S, w["bcol"]:w["bcol"] + S])


# ---- (a) the restatement against independent arithmetic --------------------------------------------------------------------------------------
def fma_triples():
    """About 10^5 triples: random values over many binades, raw bit patterns (NaN, infinities, subnormals), and the hard cases: a product
    exactly half way between two float32 values with a sticky accumulator far below it (the sum is inexact in float64 too: this is what
    rounding to odd is for), cancellation against the rounded product, and operands 2^30 apart."""
    rng = np.random.default_rng(11)
    n = 30000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-30, 31, n)).astype(F32)
    bits = [rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(F32) for _ in range(3)]
    # ties: (1 + k 2^-12)^2 = 1 + k 2^-11 + k^2 2^-24 lies half way for odd k; the accumulator is the sticky bit
    k = (2 * rng.integers(0, 2048, 10000) + 1).astype(np.float64)
    ta = (1 + k * 2.0 ** -12).astype(F32)
    sticky = np.array([2.0 ** -60, -2.0 ** -60, 2.0 ** -149, -2.0 ** -149, 2.0 ** -40, -2.0 ** -40, 0.0, 2.0 ** -126], F32)[rng.integers(0, 8, 10000)]
    # cancellation: c = -fl(a b), and the same one ulp off
    ca, cb = a[:10000], b[:10000]
    cc = -(ca.astype(np.float64) * cb.astype(np.float64)).astype(F32)
    cc2 = np.nextafter(cc, F32(0))
    # 2^30 apart
    fa, fb = (1 + rng.random(10000)).astype(F32), ((1 + rng.random(10000)) * 2.0 ** 30).astype(F32)
    fc = (rng.standard_normal(10000)).astype(F32)
    A = np.concatenate([a, bits[0], ta, ca, ca, fa, fc])
    B = np.concatenate([b, bits[1], ta, cb, cb, fb, fa])
    C = np.concatenate([c, bits[2], sticky, cc, cc2, fc, fb])
    assert len(A) == len(B) == len(C) == 100000
    return A, B, C


def test_the_hard_fma_cases_are_hard():
    """The tie with a sticky bit: rounding the float64 sum to float32 (double rounding) gets it wrong, the emulation does not."""
    a = F32(1 + 2.0 ** -12)                                                      # a^2 = 1 + 2^-11 + 2^-24: half way at float32
    up, down = O.fma32(a, a, F32(2.0 ** -60)), O.fma32(a, a, F32(-2.0 ** -60))
    assert float(up) == 1 + 2.0 ** -11 + 2.0 ** -23 and float(down) == 1 + 2.0 ** -11
    naive = F32(np.float64(a) * np.float64(a) + np.float64(F32(-2.0 ** -60)))
    assert float(naive) != float(down) or float(F32(np.float64(a) * np.float64(a) + 2.0 ** -60)) != float(up)
    assert float(O.fma32(a, a, F32(0))) == 1 + 2.0 ** -11                        # the exact tie goes to even
    assert float(O.fma32(F32(3), F32(5), F32(-15))) == 0.0 and not np.signbit(O.fma32(F32(3), F32(5), F32(-15)))
    assert np.isnan(O.fma32(F32(0), F32(np.inf), F32(1))) and float(O.fma32(F32(2), F32(np.inf), F32(1))) == np.inf


def test_np_sum_small_is_numpys_sum():
    rng = np.random.default_rng(2)
    for n in (1, 7, 8, 9, 15, 16, 17, 25, 49, 81, 128):
        for dt in (np.float32, np.float64):
            v = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(dt)
            got = O.np_sum_small(list(v), dt)
            assert got.dtype == dt and got == np.sum(v) == np.add.reduce(v), (n, dt)


def finite_pairs():
    for name, c in TC.cases().items():
        for i, w in enumerate(O.windows(c)):
            if w["valid"] and O.window_finite(c, i, w):
                yield name, c, i, w


def test_restated_c_is_within_the_rounding_bound_of_the_plain_definition():
    """A chain of 2 T^2 fused multiply-adds and ks - 1 additions commits at most 2 T^2 + ks roundings on any path from a term to the
    result, so |C - exact| <= gamma * sum |a| |b| with gamma = n u / (1 - n u), n = 2 T^2 + ks, u = 2^-24 (Higham, Accuracy and Stability
    of Numerical Algorithms, section 3.1). oc_oracle.corr_block's float64 sum of the same terms errs by 2 T^2 * 2^-53 of the same sum at
    most, which the comparison adds."""
    worst, count = 0.0, 0
    for name, c, i, w in finite_pairs():
        Aw, Bw = window_of(c, i, w)
        ks, T = O.plan(c["T"], c["S"])["ks"], c["T"]
        n = 2 * T * T + ks
        gamma = n * 2.0 ** -24 / (1 - n * 2.0 ** -24) + 2 * T * T * 2.0 ** -53
        ref = oc_oracle.corr_block(Aw, Bw, bool(c["conj_b"]))
        mag = oc_oracle.corr_block(np.abs(Aw.real) + 1j * np.abs(Aw.imag), np.abs(Bw.real) + 1j * np.abs(Bw.imag), True)
        err = np.abs(TC.expected_corr(name)[i].astype(np.float64) - ref)
        assert (err <= gamma * mag).all(), (name, i, float((err / np.maximum(gamma * mag, 1e-300)).max()))
        if mag.max() > 0:
            worst = max(worst, float((err[mag > 0] / (gamma * mag[mag > 0])).max()))
        count += 1
    print(f"{count} pairs, largest error / bound {worst:.3g}")
    assert count > 200 and 0 < worst <= 1


def test_wave_argmax_is_np_argmax_and_the_sum_is_near_numpys():
    for name, c, i, w in finite_pairs():
        C = TC.expected_corr(name)[i]
        best, bi, sabs = O.wave_reduce(C)
        assert bi == int(np.argmax(C)) and best == C.ravel()[bi], (name, i)
        exact = np.abs(C.astype(np.float64)).sum()
        assert abs(sabs - exact) <= C.size * 2.0 ** -53 * exact, (name, i)            # any order of n float64 additions


def test_the_restated_window_is_the_references_rule():
    """pu, pv and the set of correlated pairs against a direct statement of `templatematch.py:264-294` with numpy's own round and trunc."""
    for name, c in TC.cases().items():
        ha, wa = c["A"].shape
        hb, wb = c["B"].shape[1:]
        T, S = c["T"], c["S"]
        for i, w in enumerate(O.windows(c)):
            u, v, idu, idv = c["pairs"][i]
            if np.isnan(u):
                assert not w["valid"] and np.isnan(w["pu"])
                continue
            with np.errstate(all="ignore"):
                ac = np.round(np.array([u, v])) - (T / 2 % 1)
                bc = np.round(np.array([u, v]) + np.array([idu, idv])) - (S / 2 % 1)
                assert np.array_equal([w["pu"], w["pv"]], ac, equal_nan=True)
                ok = bool(np.isfinite(ac).all() and np.isfinite(bc).all())
                if ok:
                    lo = [bc[1] - S / 2, ac[1] - T / 2, bc[0] - S / 2, ac[0] - T / 2]
                    hi = [(bc[1] + S / 2, hb), (ac[1] + T / 2, ha), (bc[0] + S / 2, wb), (ac[0] + T / 2, wa)]
                    ok = all(np.trunc(x) >= 0 for x in lo) and all(np.trunc(x) < m for x, m in hi)
            assert w["valid"] == (ok and 0 <= c["bidx"][i] < len(c["B"])), (name, i)


# ---- (b) the cases reach what they are named for -----------------------------------------------------------------------------------------------
def test_the_path_cases_reach_their_paths():
    plans = TC.check_claims()
    assert {p["ks"] > 1 for p in plans.values()} == {True, False} and {p["gy"] for p in plans.values()} >= {1, 3, 16, 32}
    assert any(p["nx"] > 1 for p in plans.values()) and any(p["ny"] > 1 for p in plans.values())
    assert any(p["ks"] & (p["ks"] - 1) for p in plans.values())                   # a ks that is no power of two
    cs = TC.cases()
    assert {cs[n]["conj_b"] for n in cs} == {0, 1}
    assert cs["float32_images"]["img_a"].dtype == np.float32 and cs["gy16"]["img_a"].dtype == np.uint8
    c = cs["B_larger_than_A_three_B_images"]
    assert c["A"].shape != c["B"].shape[1:] and set(c["bidx"]) == {0, 1, 2}
    assert cs["B_narrower_than_A"]["B"].shape[2] < cs["B_narrower_than_A"]["A"].shape[1]
    for n in TC.PATHS:
        assert all(w["valid"] for w in O.windows(cs[n])), n
        assert len(cs[n]["pairs"]) == TC.PATHS[n][2] <= 4 and max(cs[n]["A"].shape) <= cs[n]["S"] + 8


def test_the_window_cases_cross_every_edge():
    for T, S in ((4, 8), (5, 8), (4, 9), (5, 9)):
        c = TC.cases()[f"windows_T{T}_S{S}"]
        ha, wa = c["A"].shape
        hb, wb = c["B"].shape[1:]
        ws = O.windows(c)
        valid = [w for w in ws if w["valid"]]
        assert 40 <= len(valid) <= len(ws) - 40
        for key, first, last in (("brow", 0, hb - 1 - S), ("bcol", 0, wb - 1 - S), ("arow", 0, ha - 1 - T), ("acol", 0, wa - 1 - T)):
            got = {w[key] for w in valid}
            assert first in got and last in got and min(got) == first and max(got) == last, (T, S, key, sorted(got))
        # the sweeps step over the edge: each has valid and invalid points
        sweeps = np.arange(13, 13 + 13 * 8).reshape(13, 8)
        for col in range(8):
            flags = [ws[k]["valid"] for k in sweeps[:, col]]
            assert True in flags and False in flags, (T, S, col)
        assert [w["valid"] for w in ws[:9]] == [False] * 9 and all(w["valid"] for w in ws[9:13])
        assert np.isnan(ws[0]["pu"]) and ws[1]["pu"] == 40 - T / 2 % 1 and np.isnan(ws[1]["pv"]) and np.isnan(ws[2]["initdu"])
        assert (ws[9]["pu"], ws[9]["pv"]) == (100 - T / 2 % 1, 102 - T / 2 % 1)   # 100.5 -> 100 and 101.5 -> 102: half to even
        assert [w["valid"] for w in ws[-4:]] == [False, False, True, False]


def test_the_peak_tie_flat_and_nonfinite_cases_are_what_they_claim():
    cs = TC.cases()
    # peaks: where they were put; NaN du on the border with the mean kept; window sides 3 ... 9
    out, spots = TC.expected_oc("peaks_border_and_distance_1_to_5"), TC.peak_spots()
    C = TC.expected_corr("peaks_border_and_distance_1_to_5")
    for i, (mi, mj) in enumerate(spots):
        assert divmod(int(np.argmax(C[i])), 12) == (mi, mj) and C[i].max() > 60
        edge = min(mi, mj, 11 - mi, 11 - mj)
        assert np.isnan(out[2, i]) == (edge == 0) and np.isfinite(out[5, i])
        if edge:
            assert abs(out[2, i]) < 0.5 and abs(out[3, i] - (mi - 6)) < 0.5 and out[4, i] == C[i].max()
    assert sorted(min(mi, mj, 11 - mi, 11 - mj) for mi, mj in spots) == [0, 0, 0, 0, 1, 2, 3, 4, 5]
    # ties: the maximum occurs more than once, exactly; first and later maxima in the same lane, or in other lanes
    lanes = {}
    for n in ("ties_same_lane", "ties_other_lanes", "ties_both"):
        for i, Ci in TC.expected_corr(n).items():
            at = np.nonzero(Ci.ravel() == Ci.max())[0]
            assert len(at) >= 2, (n, i)
            lanes.setdefault(n, []).append((at % 64).tolist())
            assert O.wave_reduce(Ci)[1] == at[0]
    assert all(len(set(l)) == 1 for l in lanes["ties_same_lane"]) and all(len(set(l)) == len(l) for l in lanes["ties_other_lanes"])
    assert all(len(set(l)) < len(l) and len(set(l)) > 1 for l in lanes["ties_both"])
    assert np.isfinite(TC.expected_oc("ties_both")[2]).all()                      # interior first maxima: the centroid runs on a tie
    # flat: C = 0, the argmax 0, the mean 0.0
    for Ci in TC.expected_corr("flat_image").values():
        assert not Ci.any()
    out = TC.expected_oc("flat_image")
    assert np.isnan(out[2:5]).all() and (out[5] == 0.0).all() and not np.signbit(out[5]).any()
    # non-finite: NaN in the four outputs, pu / pv written; raw C only partly NaN; outside the windows nothing changes
    clean = TC.expected_oc("nonfinite_none")
    assert np.isfinite(clean).all()
    for n in NONFINITE:
        out, Craw = TC.expected_oc(n), TC.expected_corr(n)[0]
        assert np.isnan(out[2:]).all() and np.array_equal(out[:2], clean[:2]), n
        if n == "nonfinite_nan_in_last_row_of_the_window":                          # kt = T: no padded row, nothing multiplies row S - 1
            assert np.array_equal(Craw, TC.expected_corr("nonfinite_none")[0]), n
        else:
            assert not np.isfinite(Craw).all() and (np.isfinite(Craw).any() or "template" in n), n     # raw sums: only what the terms reach
    assert len(NONFINITE) == 5
    last = cs["nonfinite_nan_in_last_column_of_the_window"]
    w = O.windows(last)[0]
    assert (w["brow"], w["bcol"], w["arow"], w["acol"]) == (4, 4, 7, 7) and np.isnan(last["B"][0][9, 4 + 12 - 1])
    # the definition's own terms never reach column S - 1: the float64 sum of the plain definition is finite
    assert np.isfinite(oc_oracle.corr_block(*window_of(last, 0, w), True)).all()
    assert np.array_equal(TC.expected_oc("nonfinite_nan_just_outside_both_windows"), clean)
    assert np.isnan(cs["nonfinite_nan_just_outside_both_windows"]["A"]).sum() == 4


# ---- (c) the host build of the kernels' arithmetic ---------------------------------------------------------------------------------------------
def record(f, kind, name, ints, arrays):
    f.write(struct.pack("<qq", kind, len(name)) + name.encode())
    f.write(np.asarray(ints, np.int64).tobytes())
    for a, t in arrays:
        f.write(np.ascontiguousarray(a, t).tobytes())


def plan_table():
    ts = [(T, S) for T in range(1, 301) for S in range(T + 1, T + 301)]
    sparse_t = [1, 2, 15, 16, 17, 255, 256, 257, 301, 500, 511, 512, 513, 777, 1000, 1023, 1024, 1025, 1500, 2047, 2048]
    ts += [(T, S) for T in sparse_t for S in sorted({T + 1, T + 2, T + 15, T + 16, T + 17, T + 145, T + 301, T + 1000, 2 * T, 4096}) if T < S <= 4096]
    return ts


def interleaved(m):
    return np.stack([m.real, m.imag], -1).astype(F32)


FORIENT_SHAPES = [(3, 1, 1), (2, 1, 9), (2, 9, 1), (2, 255, 3), (2, 257, 3), (1, 2, 2), (1, 3, 3)]


def synthetic_peaks():
    """C blocks given directly, for the tail alone: R = 1, 2, 3; a NaN-free block whose window sums cancel; equal values everywhere."""
    rng = np.random.default_rng(9)
    out = [("R1", np.array([[2.5]], F32)), ("R2", rng.standard_normal((2, 2)).astype(F32)), ("R3_centre", np.array([[0, 1, 0], [1, 5, 1], [0, 1, 0]], F32)),
           ("all_equal", np.full((9, 9), 3.0, F32)), ("all_negative", -np.abs(rng.standard_normal((13, 13))).astype(F32) - 1)]
    flat_peak = np.full((11, 11), 1.0, F32)                        # the window minus its mean |c| is 0 everywhere: 0 / 0
    flat_peak[5, 5] = np.nextafter(F32(1), F32(2))
    out.append(("window_sums_to_zero", flat_peak))
    for R in (5, 12, 17, 64, 100):
        out.append((f"random_R{R}", rng.standard_normal((R, R)).astype(F32)))
    return out


def write_records(path):
    n = 0
    with open(path, "wb") as f:
        A, B, C = fma_triples()
        record(f, 1, "fma 100000 triples", [len(A)], [(A, F32), (B, F32), (C, F32), (O.fma32(A, B, C), F32)])
        ts = np.array(plan_table(), np.int32)
        table = np.array([[O.plan(int(T), int(S))[k] for k in O.PLAN_FIELDS] for T, S in ts], np.int32)
        record(f, 2, f"plans {len(ts)}", [len(ts)], [(ts[:, 0], np.int32), (ts[:, 1], np.int32), (table, np.int32)])
        n += 2
        for name, c in TC.cases().items():
            ws = O.windows(c)
            record(f, 3, "window " + name, [len(ws), len(c["B"]), c["T"], c["S"], *c["A"].shape, *c["B"].shape[1:]],
                   [(c["pairs"], np.float64), (c["bidx"], np.int32), ([w["valid"] for w in ws], np.uint8),
                    ([[w["arow"], w["acol"], w["brow"], w["bcol"]] for w in ws], np.int64),
                    ([[w["pu"], w["pv"], w["initdu"], w["initdv"]] for w in ws], np.float64)])
            n += 1
            if "img_a" in c:
                for what, img in (("a", c["img_a"][None]), ("b", c["img_b"])):
                    maps = np.stack([O.forient(i) for i in img])
                    record(f, 4, f"forient {name} {what}", [0 if img.dtype == np.uint8 else 1, *img.shape], [(img, img.dtype), (interleaved(maps), F32)])
                    n += 1
            out = TC.expected_oc(name)
            for i, Ci in TC.expected_corr(name).items():
                Aw, Bw = window_of(c, i, ws[i])
                record(f, 5, f"corr {name} {i}", [c["T"], c["S"], c["conj_b"]], [(interleaved(Aw), F32), (interleaved(Bw), F32), (Ci, F32)])
                finite = O.window_finite(c, i, ws[i])
                h, w_ = c["A"].shape
                record(f, 7, f"finite {name} {i} a", [c["T"], h, w_, ws[i]["arow"], ws[i]["acol"]], [(interleaved(c["A"]), F32), ([not np.isfinite(interleaved(Aw)).all()], np.uint8)])
                Bi = c["B"][int(c["bidx"][i])]
                record(f, 7, f"finite {name} {i} b", [c["S"], *Bi.shape, ws[i]["brow"], ws[i]["bcol"]], [(interleaved(Bi), F32), ([not np.isfinite(interleaved(Bw)).all()], np.uint8)])
                n += 3
                if finite:
                    best, bi, sabs = O.wave_reduce(Ci)
                    record(f, 6, f"peak {name} {i}", [c["S"] - c["T"]], [([ws[i]["initdu"], ws[i]["initdv"]], np.float64), (Ci, F32), ([bi], np.int64),
                                                                        ([best], F32), ([sabs], np.float64), (out[2:, i], np.float64)])
                    n += 1
        rng = np.random.default_rng(4)
        for k, (cnt, h, w_) in enumerate(FORIENT_SHAPES):
            for dt in (np.uint8, np.float32):
                img = rng.integers(0, 256, (cnt, h, w_), dtype=np.uint8) if dt == np.uint8 else rng.standard_normal((cnt, h, w_)).astype(F32)
                maps = np.stack([O.forient(i) for i in img])
                record(f, 4, f"forient {cnt}x{h}x{w_} {np.dtype(dt).name}", [0 if dt == np.uint8 else 1, cnt, h, w_], [(img, dt), (interleaved(maps), F32)])
                n += 1
        for name, Ci in synthetic_peaks():
            best, bi, sabs = O.wave_reduce(Ci)
            record(f, 6, "peak synthetic " + name, [Ci.shape[0]], [([0.5, -1.5], np.float64), (Ci, F32), ([bi], np.int64), ([best], F32), ([sabs], np.float64),
                                                                   (O.peak_tail(Ci, bi, best, sabs, 0.5, -1.5), np.float64)])
            n += 1
    return n


def test_the_lds_bound_holds_for_every_plan():
    """The staged planes, and the reduction buffer when ks > 1, fit the 16384 floats the kernel may use."""
    for T, S in plan_table():
        p = O.plan(T, S)
        assert p["stage"] <= O.TM_LDS_FLOATS and p["reduce"] <= O.TM_LDS_FLOATS and p["lds_floats"] <= O.TM_LDS_FLOATS, (T, S, p)
        assert p["threads"] <= 256 and p["threads"] % 64 == 0 and p["kt"] % p["ks"] == 0 and p["kx"] % 16 == 0 and p["pitch"] % 16 == 4
        assert p["gy"] * p["gx"] * p["ks"] <= p["threads"] and p["gy"] * p["ny"] >= p["R"] and 16 * p["gx"] * p["nx"] >= p["R"]


@pytest.fixture(scope="module")
def harness_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tm_host"))
    n = write_records(os.path.join(d, "records.bin"))
    return d, n


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_equals_the_restatement_bit_for_bit(harness_dir, sanitize):
    d, n = harness_dir
    exe = toolchain.host_program(d, "tm_host_harness.cpp", sanitize)
    r = subprocess.run([exe, os.path.join(d, "records.bin")], capture_output=True, text=True)
    bad = [ln for ln in r.stdout.split("\n") if not ln.startswith("ok ")]
    print("\n".join(bad))
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), "\n".join(bad)[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == n and "DIFFERENT" not in r.stdout and "MISSING" not in r.stdout
    assert n > 600


def test_the_new_entry_point_is_declared_bound_and_exported():
    from icepy4d_amd import _lib
    with open(os.path.join(ROOT, "include", "icematch.h")) as f:
        header = f.read()
    for name in ("im_forient", "im_template_match_oc", "im_template_match_corr"):
        m = re.search(r"\nint " + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.SIGNATURES["im_template_match_corr"] == _lib.SIGNATURES["im_template_match_oc"]
    assert hasattr(_lib.load(), "im_template_match_corr")
