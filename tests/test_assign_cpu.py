"""The assignment stage's oracles and cases held against each other without a GPU (tests/assign_oracle.py, tests/assign_cases.py):
what test_gpu_assign.py leans on must itself be right.

* the float32 restatement, fed the float64 normalisers rounded once, gives the matches of oracle/ref_cpu.mutual_nn_filter on float64
  scores, except where `explain` explains a difference by its float64 margin;
* the planted ties are exact ties of the restated float32 matrix and win their rows and columns; the planted one-step ties are one
  float32 step;
* the 1 % cap on explained differences is held by the reference alone: with tol = 4 x (float32 oracle - float64), at most 1 % of
  the rows, columns and threshold decisions of any case lie inside tol, the plants (known, exempted by index) apart;
* `f2ord` and the key decode round-trip, and key order is (score descending, row ascending).
"""
import numpy as np
import pytest
import torch

import assign_cases as ac
import assign_oracle as ao
from oracle import ref_cpu

IDS = [ac.case_id(c) for c in ac.CASES]
_RS = {}


def prepared(c):
    """The shared case data plus the restatement from the float64 normalisers rounded once."""
    d, r64, y = ac.prepared(c)
    if c not in _RS:
        _RS.clear()
        _RS[c] = ao.restate(d["sim"], ao.normalisers_from_ref64(r64), 0)
    return d, r64, y, _RS[c]


def top2(v):
    o = np.argsort(-v, kind="stable")[:2]
    return tuple(int(k) for k in o)


@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_case_selects_its_form(c):
    assert ac.selected_form(c)[0] == c.form
    d = ac.make_case(c) if c.m * c.n < 5000 else prepared(c)[0]
    buf = d["buf"]
    live = np.zeros(buf.shape, dtype=bool)
    live[c.off:c.off + c.m * c.ld].reshape(c.m, c.ld)[:, :c.n] = True
    assert np.isnan(buf[~live]).all() and np.isfinite(buf[live]).all()          # NaN wherever a clamped load may land
    assert np.array_equal(buf[c.off:c.off + c.m * c.ld].reshape(c.m, c.ld)[:, :c.n], d["sim"])


@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_restatement_matches_float64_reference(c):
    d, r64, y, rs = prepared(c)
    t = torch.from_numpy(r64["scores"])
    full = torch.full((1, c.m + 1, c.n + 1), -1e300, dtype=torch.float64)
    full[0, :c.m, :c.n] = t
    q0, q1, s0, s1 = ref_cpu.mutual_nn_filter(full, ac.THRESHOLD)
    f = ao.filter_matches(rs["ridx"], rs["rval"], rs["cidx"], ac.THRESHOLD)
    e = ao.explain(rs["ridx"], rs["cidx"], f["m0"], f["m1"], r64, ac.THRESHOLD, y["tol"])
    assert np.array_equal(e["ref_m0"], q0[0].numpy()) and np.array_equal(e["ref_m1"], q1[0].numpy())       # explain's filter = the oracle's
    assert e["unexplained"] == [], e["unexplained"][:5]
    if not (e["rows"] or e["cols"] or e["thr"]):
        assert np.array_equal(f["m0"], q0[0].numpy()) and np.array_equal(f["m1"], q1[0].numpy())
    # the restated scores are float32 roundings of the float64 ones: within the yardstick itself
    assert np.abs(rs["scores"].astype(np.float64) - r64["scores"]).max() <= y["tol"]
    # keys decode to the column arg-max
    val, row = ao.decode_keys(rs["keys"])
    assert np.array_equal(row, rs["cidx"]) and np.array_equal(val.view(np.uint32), rs["cval"].view(np.uint32))


@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_planted_ties_are_exact_and_win(c):
    d, r64, y, rs = prepared(c)
    s, p = rs["scores"], d["plants"]
    if c.m >= 15 and c.n >= 40:
        assert p["cols"] and p["rows"] and p["near_row"] and p["near_col"]
    for j, j2, rows in p["cols"]:
        assert np.array_equal(s[:, j].view(np.uint32), s[:, j2].view(np.uint32))        # the whole column, bit for bit
        for i in rows:
            assert s[i, j] == s[i].max() and rs["ridx"][i] == j                           # the winners, and the first of the two
    for i, i2, cols in p["rows"]:
        assert np.array_equal(s[i].view(np.uint32), s[i2].view(np.uint32))
        for j in cols:
            assert s[i, j] == s[:, j].max() and rs["cidx"][j] == i
            f = ao.filter_matches(rs["ridx"], rs["rval"], rs["cidx"], ac.THRESHOLD)
            if rs["ridx"][i] == j:      # the mutual check follows the lower row; its duplicate stays unmatched
                assert f["mutual0"][i] and not f["mutual0"][i2] and f["m0"][i2] == -1
    dup_r, dup_c = {v for t in p["rows"] for v in t[:2]}, {v for t in p["cols"] for v in t[:2]}
    if c.m >= 15 and c.n >= 40:
        assert (p["last_row"] is not None) == (c.m - 1 not in dup_r) and (p["last_col"] is not None) == (c.n - 1 not in dup_c)
    if p["last_row"]:
        i, j = p["last_row"]
        assert i == c.m - 1 and rs["cidx"][j] == i and rs["ridx"][i] == j
    if p["last_col"]:
        r, k = p["last_col"]
        assert k == c.n - 1 and rs["ridx"][r] == k and rs["cidx"][k] == r
    if p["near_row"]:
        r, a, b = p["near_row"]
        assert top2(s[r]) == (b, a) and s[r, b] == np.nextafter(s[r, a], np.float32(np.inf)) and rs["ridx"][r] == b
    if p["near_col"]:
        cc, q0, q1 = p["near_col"]
        assert top2(s[:, cc]) == (q1, q0) and s[q1, cc] == np.nextafter(s[q0, cc], np.float32(np.inf)) and rs["cidx"][cc] == q1


@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_one_percent_cap_is_held_by_the_reference(c):
    """On these cases tol is 2.1e-5 .. 5.3e-5 at scale 3 and 3.4e-4 .. 3.7e-4 at scale 30 (the planted winners sit near 12 x scale, where
    a float32 step of 2 x - lse is 4e-6 / 3e-5), and 0 to 1 decision per case lies inside it, the plants apart."""
    d, r64, y, rs = prepared(c)
    rows, cols, thr = ao.decisions_within(r64, ac.THRESHOLD, y["tol"])
    s = r64["scores"]
    rows = [i for i in rows if not ac.planted_tie(d["plants"], "row", int(i), top2(s[i]))]
    cols = [j for j in cols if not ac.planted_tie(d["plants"], "col", int(j), top2(s[:, j]))]
    print(f"{ac.case_id(c)}: tol {y['tol']:.3g} tol_lse {y['tol_lse']:.3g}; inside tol: {len(rows)} rows, {len(cols)} columns, {len(thr)} thresholds")
    assert 0 < y["tol"] < 1e-3 or c.m * c.n == 1
    assert len(rows) <= 0.01 * c.m and len(cols) <= 0.01 * c.n
    assert len(thr) <= 0.01 * c.m


def test_f2ord_and_keys():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.normal(0, 50, 4000), [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.0e38, -3.0e38]]).astype(np.float32)
    o = ao.f2ord(v)
    assert np.array_equal(ao.ord2f(o).view(np.uint32), v.view(np.uint32))                 # round trip, bit for bit (signed zeros too)
    idx = np.argsort(o, kind="stable")
    assert (np.diff(v[idx].astype(np.float64)) >= 0).all()                                # monotone
    assert ao.f2ord(np.float32(-0.0)) + 1 == ao.f2ord(np.float32(0.0))                     # -0 sits one step below +0, nothing between
    # keys: (score descending, row ascending), with many equal scores
    val = rng.integers(-3, 4, 5000).astype(np.float32) * np.float32(0.5)
    row = rng.permutation(5000)
    keys = ao.make_keys(val, row)
    dv, dr = ao.decode_keys(keys)
    assert np.array_equal(dv.view(np.uint32), val.view(np.uint32)) and np.array_equal(dr, row)
    by_key = np.argsort(keys)[::-1]
    by_rule = np.lexsort((row, -val.astype(np.float64)))
    assert np.array_equal(by_key, by_rule)
    # signed zeros: the key compares bit patterns, so +0 ranks above -0 before the row is looked at. `assign_score` cannot return -0
    # (a sum is -0 only if both terms are, and x - max and l0 + l1 are +0 when they vanish), so on scores the stage produces the key
    # order IS (score descending, row ascending); with the zeros canonical that holds here as well.
    z = np.array([0.0, -0.0, 0.0, -0.0], dtype=np.float32)
    rz = np.array([3, 0, 1, 2])
    assert list(np.argsort(ao.make_keys(z, rz))[::-1]) == [2, 0, 1, 3]
    assert list(np.argsort(ao.make_keys(z + np.float32(0.0), rz))[::-1]) == [1, 2, 3, 0]


def test_explain_rejects_what_it_should():
    """A wrong arg-max with a real margin, a dropped match and an invented one are all unexplained."""
    c = ac.CASES[12]
    d, r64, y, rs = prepared(c)
    f = ao.filter_matches(rs["ridx"], rs["rval"], rs["cidx"], ac.THRESHOLD)
    good = ao.explain(rs["ridx"], rs["cidx"], f["m0"], f["m1"], r64, ac.THRESHOLD, y["tol"])
    assert good["unexplained"] == []
    bad = rs["ridx"].copy()
    bad[5] = (bad[5] + 1) % c.n
    assert ao.explain(bad, rs["cidx"], f["m0"], f["m1"], r64, ac.THRESHOLD, y["tol"])["unexplained"]
    i = int(np.nonzero(f["m0"] > -1)[0][0])
    m0 = f["m0"].copy()
    m0[i] = -1
    assert ao.explain(rs["ridx"], rs["cidx"], m0, f["m1"], r64, ac.THRESHOLD, y["tol"])["unexplained"]
    k = int(np.nonzero(f["m1"] == -1)[0][0])
    m1 = f["m1"].copy()
    m1[k] = 0
    assert ao.explain(rs["ridx"], rs["cidx"], f["m0"], m1, r64, ac.THRESHOLD, y["tol"])["unexplained"]
