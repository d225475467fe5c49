"""The assignment sweeps (csrc/lg_misc.hip, csrc/lg_assign_pipe.hip, csrc/assign_sweep.h) pinned to exact restatements at every path
boundary: each case of tests/assign_cases.py through `im_assign_from_sim`, by the kernel form its table names.

Per case:
  * `rmax` / `cmax` bit-exact against the float32 row / column maxima (`max` is exact);
  * `rmax + rlog`, `cmax + clog` within tol_lse of the float64 logsumexp;
  * with the device's own normalisers read back, the float32 restatement of `assign_score` reproduces the score matrix, so `ridx`,
    `rval`, every `cbest` key, `m0`, `m1` and the zero / non-zero pattern of `s0` / `s1` are bit-identical to it (no tolerance); the
    matching score is within 2 ulp of exp(rval), and `ms > th` is decided on the device's own value;
  * `explain` against the float64 reference leaves nothing unexplained, and explains at most 1 % of the rows and of the columns (the
    planted one-step ties apart: they are inside any tolerance on purpose);
  * the duplicated columns / rows resolve to the first column / the lowest row; NaN padding never leaks; the sentinels behind the
    live part of the four outputs survive; a second run through the same workspace is bit-identical.
Tolerances come from the reference alone (assign_oracle.yardsticks): tol = 4 x max |float32 oracle scores - float64|, tol_lse =
4 x max |torch float32 logsumexp - float64|. Each test prints the device's errors beside them.

Then SuperGlue's MODE 1 sweep (`((x + u) + v) - norm` restated from the tapped `sim`, `u`, `v`, `norm`) in all three forms, and the
LightGlue goldens on engines whose grid is larger than the live counts.

Measured on an MI355X, largest over the cases of a scale (each case prints its own):

    scale   |lse - float64|   tol_lse             |restated device scores - float64|   tol                 expf
    3       4.3e-7            5.7e-6 .. 7.4e-6    1.3e-5                               2.1e-5 .. 5.3e-5    <= 1 ulp
    30      2.7e-7            5.2e-5 .. 5.3e-5    9.1e-5                               3.4e-4 .. 3.7e-4    <= 1 ulp

The normalisers are 13 to 200 times inside their yardstick; the score error equals what the float32 oracle itself loses (the
rounding of 2 x - lse at |x| near 12 x scale, not the normalisers). `explain` had at most one row and one column per case to
explain, each a planted one-step tie; no threshold decision differed. logsigmoid is within 2.4e-7 of float64.
"""
import numpy as np
import pytest
import torch

import assign_cases as ac
import assign_oracle as ao
from conftest import load_golden
from icepy4d_amd import synthetic

pytestmark = pytest.mark.gpu

IDS = [ac.case_id(c) for c in ac.CASES]
SENT_I, SENT_F = -7, -5.0

def make_engine(kpts):
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    e.reserve(64, 64, 2, kpts)
    return e


@pytest.fixture(scope="module")
def eng6160():
    e = make_engine(ac.MAX_KPTS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng1040():
    e = make_engine(1040)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng1041():
    e = make_engine(1041)       # an odd reservation: ld = K = 1041 puts the matcher's own sweeps on the scalar-load form
    yield e
    e.close()


def tap(e, name, count, dtype=np.float32):
    """`count` 32-bit words of the internal buffer `name`, reinterpreted as dtype."""
    buf = torch.empty(count, dtype=torch.float32, device=e.device)
    e.ctx.call("im_debug_read", name.encode(), buf.data_ptr(), count, e.stream_ptr())
    return buf.cpu().numpy().view(dtype)


def run_assign(e, d):
    """One `im_assign_from_sim` call on case data d: every output and every tapped buffer, as host arrays."""
    c = d["case"]
    K = e.max_kpts
    dbuf = torch.from_numpy(d["buf"]).to(e.device)
    sim_ptr = dbuf.data_ptr() + 4 * c.off
    vec = c.ld % 4 == 0 and sim_ptr % 16 == 0                    # launch_assign's condition on the real pointer
    form = "pipe" if vec and (c.m + 15) // 16 <= 384 else "vec" if vec else "scalar"
    assert form == c.form, (form, c)
    dz0, dz1 = torch.from_numpy(d["z0"]).to(e.device), torch.from_numpy(d["z1"]).to(e.device)
    m0 = torch.full((c.m + 8,), SENT_I, dtype=torch.int32, device=e.device)
    m1 = torch.full((c.n + 8,), SENT_I, dtype=torch.int32, device=e.device)
    s0 = torch.full((c.m + 8,), SENT_F, device=e.device)
    s1 = torch.full((c.n + 8,), SENT_F, device=e.device)
    e.ctx.call("im_assign_from_sim", sim_ptr, c.m, c.n, c.ld, dz0.data_ptr(), dz1.data_ptr(), ac.THRESHOLD,
               m0.data_ptr(), m1.data_ptr(), s0.data_ptr(), s1.data_ptr(), e.stream_ptr())
    e.synchronize()
    lz = tap(e, "lz", 2 * K)
    out = dict(m0=m0.cpu().numpy(), m1=m1.cpu().numpy(), s0=s0.cpu().numpy(), s1=s1.cpu().numpy(),
               rmax=tap(e, "rmax", c.m), rlog=tap(e, "rlog", c.m), cmax=tap(e, "cmax", c.n), clog=tap(e, "clog", c.n),
               ridx=tap(e, "ridx", c.m, np.int32), rval=tap(e, "rval", c.m), cbest=tap(e, "cbest", 2 * c.n, np.uint64),
               lz0=lz[:c.m].copy(), lz1=lz[K:K + c.n].copy())
    assert np.array_equal(dbuf.cpu().numpy().view(np.uint32), d["buf"].view(np.uint32))        # the input is read-only
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def check_against_restatement(out, rs, m, n, th):
    """ridx, rval, keys, matches and the score pattern bit-identical to the restatement rs; returns the device's column arg-max."""
    assert np.array_equal(out["ridx"], rs["ridx"])
    assert np.array_equal(bits(out["rval"]), bits(rs["rval"]))
    assert np.array_equal(out["cbest"], rs["keys"])
    cval, cidx = ao.decode_keys(out["cbest"])
    assert np.array_equal(cidx, rs["cidx"]) and np.array_equal(bits(cval), bits(rs["cval"]))
    s0, s1 = out["s0"][:m], out["s1"][:n]
    f = ao.filter_matches(rs["ridx"], rs["rval"], rs["cidx"], th, ms_dev=s0)
    assert np.array_equal(out["m0"][:m], f["m0"]) and np.array_equal(out["m1"][:n], f["m1"])
    assert np.array_equal(s0 != 0, f["mutual0"]) and np.array_equal(s1 != 0, f["mutual1"])
    ms_ref = f["ms0"].astype(np.float32)
    ulps = int(ao.ulp_distance(s0, ms_ref).max())
    assert ulps <= 2, ulps                                                    # expf against the correctly rounded exp(rval)
    assert np.array_equal(bits(s1), bits(np.where(f["mutual1"], s0[rs["cidx"]], np.float32(0))))
    return f, ulps


@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_assign_case(eng6160, c):
    d, r64, y = ac.prepared(c)
    m, n, th = c.m, c.n, ac.THRESHOLD
    out = run_assign(eng6160, d)
    again = run_assign(eng6160, d)
    for k in out:                                                             # repeatable through the same workspace, bit for bit
        assert out[k].tobytes() == again[k].tobytes(), k
    for k, live in (("m0", m), ("m1", n)):
        assert (out[k][live:] == SENT_I).all(), k
    for k, live in (("s0", m), ("s1", n)):
        assert (out[k][live:] == np.float32(SENT_F)).all(), k
    for k in ("rmax", "rlog", "cmax", "clog", "rval", "lz0", "lz1"):
        assert np.isfinite(out[k]).all(), k                                   # no NaN from the padding
    # normalisers: the maxima exactly, the log-sum-exp within the float32 yardstick
    assert np.array_equal(bits(out["rmax"]), bits(d["sim"].max(1))) and np.array_equal(bits(out["cmax"]), bits(d["sim"].max(0)))
    err_r = float(np.abs(out["rmax"].astype(np.float64) + out["rlog"].astype(np.float64) - r64["rlse"]).max())
    err_c = float(np.abs(out["cmax"].astype(np.float64) + out["clog"].astype(np.float64) - r64["clse"]).max())
    err_z = float(max(np.abs(out["lz0"] - r64["lz0"]).max(), np.abs(out["lz1"] - r64["lz1"]).max()))
    nz = {k: out[k] for k in ("rmax", "rlog", "cmax", "clog", "lz0", "lz1")}
    rs = ao.restate(d["sim"], nz, 0)
    err_s = float(np.abs(rs["scores"].astype(np.float64) - r64["scores"]).max())
    print(f"\n{ac.case_id(c)}: row lse err {err_r:.3g} col lse err {err_c:.3g} (tol_lse {y['tol_lse']:.3g}, float32 torch {y['err32_lse']:.3g}); "
          f"score err {err_s:.3g} (tol {y['tol']:.3g}, float32 oracle {y['err32']:.3g}); logsigmoid err {err_z:.3g}")
    if m * n > 1:
        assert err_r <= y["tol_lse"] and err_c <= y["tol_lse"], (err_r, err_c, y)
    else:
        assert err_r == 0 and err_c == 0       # one entry: log(1) = 0 exactly (the yardstick itself is 0 there)
    # everything behind the normalisers: identity
    f, ulps = check_against_restatement(out, rs, m, n, th)
    # the plants
    p = d["plants"]
    for j, j2, rows in p["cols"]:
        assert bits(out["cmax"])[j] == bits(out["cmax"])[j2] and bits(out["clog"])[j] == bits(out["clog"])[j2]
        assert np.array_equal(bits(rs["scores"][:, j]), bits(rs["scores"][:, j2]))
        for i in rows:
            assert out["ridx"][i] == j, (i, j, j2, out["ridx"][i])
    for i, i2, cols in p["rows"]:
        assert bits(out["rmax"])[i] == bits(out["rmax"])[i2] and bits(out["rlog"])[i] == bits(out["rlog"])[i2]
        for j in cols:
            assert rs["cidx"][j] == i, (j, i, i2, rs["cidx"][j])
            if out["ridx"][i] == j:
                assert out["s0"][i] != 0 and out["s0"][i2] == 0 and out["m0"][i2] == -1
    if p["last_row"]:
        i, j = p["last_row"]
        assert rs["cidx"][j] == i and out["ridx"][i] == j and out["s0"][i] != 0 and out["s1"][j] != 0      # the last strip's own winner, mutual
    if p["last_col"]:
        r, k = p["last_col"]
        assert out["ridx"][r] == k and rs["cidx"][k] == r and out["s0"][r] != 0 and out["s1"][k] != 0      # the last column's
    # end to end against float64
    e = ao.explain(out["ridx"], rs["cidx"], out["m0"][:m], out["m1"][:n], r64, th, y["tol"])
    assert e["unexplained"] == [], e["unexplained"][:5]
    rows = [t for t in e["rows"] if not ac.planted_tie(p, "row", t[1], (t[2], t[3]))]
    cols = [t for t in e["cols"] if not ac.planted_tie(p, "col", t[1], (t[2], t[3]))]
    print(f"    explained: {len(e['rows'])} rows ({len(rows)} not planted), {len(e['cols'])} columns ({len(cols)} not planted), "
          f"{len(e['thr'])} thresholds; matches {int((out['m0'][:m] > -1).sum())}; expf within {ulps} ulp")
    assert len(rows) + len(e["thr"]) <= 0.01 * m and len(cols) <= 0.01 * n


# ------------------------------------------------------------------------------------------------ SuperGlue: MODE 1
def superglue_case(e, m, n, form):
    K = e.max_kpts
    vec = K % 4 == 0                                # ld = K, the workspace's own score matrix (16-byte aligned)
    got = "pipe" if vec and (K + 15) // 16 <= 384 else "vec" if vec else "scalar"          # m_max = K: the grid is the reservation's
    assert got == form
    e.load_state_dict("superglue", synthetic.superglue_state_dict(0, "passthrough"))
    f = synthetic.synthetic_features(11, m, n)
    e.kpts.zero_(); e.desc.zero_(); e.scores.zero_()
    e.kpts[0, :m] = torch.from_numpy(f["kpts0"]).cuda(); e.kpts[1, :n] = torch.from_numpy(f["kpts1"]).cuda()
    e.desc[0, :m] = torch.from_numpy(f["desc0"]).cuda(); e.desc[1, :n] = torch.from_numpy(f["desc1"]).cuda()
    e.scores[0, :m] = torch.from_numpy(f["scores0"]).cuda(); e.scores[1, :n] = torch.from_numpy(f["scores1"]).cuda()
    e.n[:] = torch.tensor([m, n], dtype=torch.int32)
    th = 0.3                                        # these weights put mutual pairs on both sides of it
    runs = []
    for _ in range(2):
        e.matches.fill_(SENT_I); e.mscores.fill_(SENT_F)
        e.superglue((480, 640), (480, 640), sinkhorn_iterations=20, match_threshold=th)
        e.synchronize()
        runs.append(dict(m0=e.matches[0].cpu().numpy(), m1=e.matches[1].cpu().numpy(), s0=e.mscores[0].cpu().numpy(), s1=e.mscores[1].cpu().numpy(),
                         ridx=tap(e, "ridx", m, np.int32), rval=tap(e, "rval", m), cbest=tap(e, "cbest", 2 * n, np.uint64),
                         u=tap(e, "u", m + 1), v=tap(e, "v", n + 1), norm=tap(e, "norm", 1)))
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    out = runs[0]
    sim = tap(e, "sim", m * K).reshape(m, K)[:, :n]
    assert np.isfinite(sim).all() and np.isfinite(out["u"]).all() and np.isfinite(out["v"]).all()
    rs = ao.restate(sim, dict(u=out["u"][:m], v=out["v"][:n], norm=out["norm"][0]), 1)
    fm, ulps = check_against_restatement(out, rs, m, n, th)
    # behind the live counts the forward's own initialisation (-1 / 0) stands
    assert (out["m0"][m:] == -1).all() and (out["m1"][n:] == -1).all() and (out["s0"][m:] == 0).all() and (out["s1"][n:] == 0).all()
    print(f"\nsuperglue {m} x {n} on {K} ({form}): mutual {int(fm['mutual0'].sum())}, matches {int((out['m0'][:m] > -1).sum())}, expf within {ulps} ulp")
    matched = out["m0"][:m] > -1
    assert matched.sum() > 20 and (fm["mutual0"] & ~matched).sum() > 5


def test_superglue_sweep_pipelined(eng1040):
    superglue_case(eng1040, 1030, 517, "pipe")


def test_superglue_sweep_plain_vectorised(eng6160):
    superglue_case(eng6160, 200, 150, "vec")


# ------------------------------------------------------------------------------------------------ LightGlue: grid larger than the live counts
@pytest.mark.parametrize("ci", [2, 5])
@pytest.mark.parametrize("kpts", [1040, 6160])
def test_lightglue_golden_on_a_larger_grid(eng1040, eng6160, kpts, ci):
    """The product path (ld = K, m_max = n_max = K) with far fewer live keypoints than the reservation: 1040 -> pipelined form with
    65 strips of which most are empty, 6160 -> plain vectorised form. Matches equal the golden, scores within the goldens' 1e-4."""
    e = eng1040 if kpts == 1040 else eng6160
    g = load_golden(f"g2_lightglue_{ci}")
    e.load_state_dict("lightglue", synthetic.lightglue_state_dict(0, str(g["variant"])))
    f = synthetic.synthetic_features(int(g["seed"]), int(g["m"]), int(g["n"]))
    m, n = f["kpts0"].shape[0], f["kpts1"].shape[0]
    e.kpts.zero_(); e.desc.zero_()
    e.kpts[0, :m] = torch.from_numpy(f["kpts0"]).cuda(); e.kpts[1, :n] = torch.from_numpy(f["kpts1"]).cuda()
    e.desc[0, :m] = torch.from_numpy(f["desc0"]).cuda(); e.desc[1, :n] = torch.from_numpy(f["desc1"]).cuda()
    e.n[:2] = torch.tensor([m, n], dtype=torch.int32)
    e.lightglue(tuple(f["size0"]), tuple(f["size1"]), depth_confidence=float(g["depth_confidence"]), width_confidence=float(g["width_confidence"]))
    e.synchronize()
    out = e.matches_to_host(m, n)
    assert out["stop"] == int(g["stop"])
    assert np.array_equal(out["matches0"], g["matches0"]) and np.array_equal(out["matches1"], g["matches1"])
    assert np.abs(out["matching_scores0"] - g["matching_scores0"]).max() < 1e-4
    assert np.abs(out["matching_scores1"] - g["matching_scores1"]).max() < 1e-4
    assert int((g["matches0"] > -1).sum()) > 0


def test_superglue_sweep_scalar_load(eng1041):
    superglue_case(eng1041, 1030, 517, "scalar")
