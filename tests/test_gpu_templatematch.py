"""Template matching on the device (csrc/templatematch.hip) against the reference's outputs (tests/golden/g11_templatematch.npz) and
against the numpy oracle (tests/oc_oracle.py) on random synthetic pairs.

Bounds: NaN pattern and pu / pv identical; forient maps within 4e-7 per component of the reference's with identical zeros, and equal
bit for bit to the oracle's; |du|, |dv| within 1e-3 px;
peakCorr and meanAbsCorr within 1e-5 T^2. A point whose du / dv differ by more is EXPLAINED only when its argmax moved and the
oracle's two largest C values lie within 1e-5 T^2 of each other (a float-level tie the device may break the other way)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oc_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {"grid": ("img0", "img1"), "grid_s": ("img1", "img2"), "grid_p": ("img2", "img3"), "odd": ("img0", "img3"),
         "float": ("float_a", "float_b"), "synth": ("synth_a", "synth_b")}


@pytest.fixture(scope="module")
def g11():
    return oc_oracle.load_g11(os.path.join(ROOT, "tests", "golden", "g11_templatematch.npz"))


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def compare(got, ref, T, A=None, B=None, pu_in=None, pv_in=None, S=None, idu=0, idv=0):
    """Asserts the bounds of the module docstring; returns the list of explained points."""
    for k in ("pu", "pv", "du", "dv", "peakCorr", "meanAbsCorr"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), f"NaN pattern of {k}"
    assert np.array_equal(got["pu"], ref["pu"], equal_nan=True) and np.array_equal(got["pv"], ref["pv"], equal_nan=True)
    tol = 1e-5 * T * T
    for k in ("peakCorr", "meanAbsCorr"):
        assert np.nanmax(np.abs(got[k] - ref[k]), initial=0) <= tol, k
    bad = np.argwhere((np.abs(got["du"] - ref["du"]) > 1e-3) | (np.abs(got["dv"] - ref["dv"]) > 1e-3))
    explained = []
    for ii in map(tuple, bad):
        assert A is not None, f"du / dv differ at {ii}"
        o = oc_oracle.oc(A, B, np.array([pu_in[ii]]), np.array([pv_in[ii]]), T, S, np.array([np.broadcast_to(idu, pu_in.shape)[ii]]),
                         np.array([np.broadcast_to(idv, pu_in.shape)[ii]]), return_c=True)
        margin = oc_oracle.top_two_margin(o["C"][(0,)])
        assert margin <= tol, f"du / dv differ at {ii} and the argmax margin {margin} exceeds {tol}"
        explained.append((ii, margin))
    if explained:
        print(f"explained by an argmax margin below {tol:.3g}: {explained}")
    return explained


def test_forient_golden(eng, g11):
    from icepy4d_amd.matching.templatematch import forient
    for name in ("forient_u8", "forient_f32"):
        got, ref = forient(g11[name + "_in"], engine=eng), g11[name]
        assert got.dtype == np.complex64 and got.shape == ref.shape
        assert np.abs(got.real - ref.real).max() <= 4e-7 and np.abs(got.imag - ref.imag).max() <= 4e-7, name
        assert np.array_equal(got == 0, ref == 0) and np.array_equal(np.sign(got.real), np.sign(ref.real))
        assert np.array_equal(np.sign(got.imag), np.sign(ref.imag))
        # the oracle performs the kernel's own three roundings (tests/test_gpu_templatematch_edges.py): the same bits
        assert got.tobytes() == oc_oracle.forient(g11[name + "_in"]).tobytes()


@pytest.mark.parametrize("case", sorted(CASES))
def test_golden_cases(eng, g11, case):
    from icepy4d_amd.matching.templatematch import OC
    T, S = (int(v) for v in g11[case + "_TS"])
    A, B = (g11[k] for k in CASES[case])
    pu, pv = g11[case + "_pu_in"].copy(), g11[case + "_pv_in"].copy()
    r = OC(A, B, pu, pv, T, S, g11[case + "_initdu"], g11[case + "_initdv"], engine=eng)
    assert r.pu is pu and r.pv is pv      # written back in place, as the reference does
    got = {k: getattr(r, k) for k in ("pu", "pv", "du", "dv", "peakCorr", "meanAbsCorr")}
    ref = {k: g11[f"{case}_{k}"] for k in got}
    compare(got, ref, T, A, B, g11[case + "_pu_in"], g11[case + "_pv_in"], S, g11[case + "_initdu"], g11[case + "_initdv"])
    assert np.array_equal(np.isnan(r.snr), np.isnan(g11[case + "_snr"]))


def test_template_match_defaults(eng, g11):
    from icepy4d_amd.matching.templatematch import TemplateMatch
    tm = TemplateMatch(g11["img0"], g11["img1"], g11["grid_xy"], engine=eng)
    r = tm.match()
    assert np.array_equal(r.pu, g11["grid_pu"]) and np.nanmax(np.abs(r.du - g11["grid_du"])) <= 1e-3


def smooth_pair(rng, h, w, shift, noise, dtype):
    from scipy import ndimage
    a = ndimage.gaussian_filter(rng.normal(0, 1, (h + 40, w + 40)), rng.uniform(1.5, 4))
    b = np.roll(a, shift, axis=(0, 1)) + rng.normal(0, noise, a.shape)
    a, b = a[20:-20, 20:-20], b[20:-20, 20:-20]
    lo, hi = a.min(), a.max()
    if dtype == np.uint8:
        return (np.clip((a - lo) / (hi - lo) * 255, 0, 255).astype(np.uint8), np.clip((b - lo) / (hi - lo) * 255, 0, 255).astype(np.uint8))
    return ((a - lo) / (hi - lo)).astype(np.float32), ((b - lo) / (hi - lo)).astype(np.float32)


@pytest.mark.parametrize("T,S,dtype", [(32, 128, np.uint8), (128, 144, np.uint8), (31, 100, np.uint8), (17, 40, np.float32),
                                       (64, 81, np.float32), (5, 6, np.uint8), (9, 30, np.uint8), (40, 120, np.uint8)])
def test_random_pairs_vs_oracle(eng, T, S, dtype):
    from icepy4d_amd.matching.templatematch import OC
    rng = np.random.default_rng(T * 1000 + S)
    h, w = 2 * S + 40, 2 * S + 80
    A, B = smooth_pair(rng, h, w, (int(rng.integers(-6, 7)), int(rng.integers(-6, 7))), 0.05, dtype)
    n = 7
    pu = rng.uniform(0, w, n).round(1)
    pv = rng.uniform(0, h, n).round(1)
    pu[0], pv[1] = 100.5, 120.5
    pu[2] = np.nan
    pu, pv = np.meshgrid(pu, pv)
    idu = rng.integers(-3, 4, pu.shape).astype(np.float64)
    idv = 1.5
    ref = oc_oracle.oc(A, B, pu, pv, T, S, idu, idv)
    pu_in, pv_in = pu.copy(), pv.copy()
    r = OC(A, B, pu, pv, T, S, idu, idv, engine=eng)
    got = {k: getattr(r, k) for k in ("pu", "pv", "du", "dv", "peakCorr", "meanAbsCorr")}
    assert np.isfinite(got["meanAbsCorr"]).sum() >= 3 and (S - T < 3 or np.isfinite(got["du"]).sum() >= 3)
    compare(got, ref, T, A, B, pu_in, pv_in, S, idu, idv)


def test_many_pairs_several_images_deterministic(eng):
    from icepy4d_amd.matching.templatematch import match_many
    rng = np.random.default_rng(5)
    T, S = 32, 128
    A, B0 = smooth_pair(rng, 700, 900, (3, -4), 0.05, np.uint8)
    Bs = [B0, np.roll(B0, (2, 5), axis=(0, 1)), np.roll(B0, (-7, 1), axis=(0, 1))]
    pu, pv = np.meshgrid(np.arange(40.0, 860, 12.5), np.arange(40.0, 660, 14))
    r1 = match_many(A, Bs, pu, pv, T, S, engine=eng)
    r2 = match_many(A, Bs, pu, pv, T, S, engine=eng)
    assert r1["du"].shape == (3,) + pu.shape and pu.size * 3 > 6000
    for k in r1:
        assert np.array_equal(r1[k], r2[k], equal_nan=True), f"{k} differs between two runs"
    idx = np.argwhere(np.isfinite(r1["du"]))
    sample = idx[rng.choice(len(idx), 24, replace=False)]
    for b, i, j in sample:
        o = oc_oracle.oc(A, Bs[b], pu[i:i + 1, j:j + 1], pv[i:i + 1, j:j + 1], T, S)
        got = {k: r1[k][b, i:i + 1, j:j + 1] for k in r1}
        compare(got, o, T, A, Bs[b], pu[i:i + 1, j:j + 1], pv[i:i + 1, j:j + 1], S)


def test_track_targets_csv(eng, g11, tmp_path):
    from icepy4d_amd.utils.track_targets import TrackTargets
    targets = g11["track_targets"]
    names = [f"T{i}" for i in range(len(targets))]
    slaves = [g11["img1"], g11["img2"], g11["img3"]]
    tr = TrackTargets(g11["img0"], slaves, targets.copy(), out_dir=str(tmp_path), target_names=names, engine=eng, parallel=True)
    tr.track()
    assert isinstance(tr.results, list) and len(tr.results) == 3
    for k, res in enumerate(tr.results):
        # the reference's own outputs
        ref = {q: g11[f"track{k}_{q}"] for q in ("pu", "pv", "du", "dv", "snr", "meanAbsCorr")}
        assert np.array_equal(res["pu"], ref["pu"], equal_nan=True) and np.array_equal(np.isnan(res["du"]), np.isnan(ref["du"]))
        assert np.nanmax(np.abs(res["du"] - ref["du"])) <= 1e-3 and np.nanmax(np.abs(res["dv"] - ref["dv"])) <= 1e-3
        # the CSV driven by the oracle's numbers, formatted as the reference does
        o = oc_oracle.oc(g11["img0"], slaves[k], targets[:, 0], targets[:, 1], 32, 128)
        snr = o["peakCorr"] / o["meanAbsCorr"]
        lines = ["label,x,y"] + [f"{n},{x:.3f},{y:.3f}" for n, x, y, s in zip(names, targets[:, 0] + o["du"], targets[:, 1] + o["dv"], snr) if s > 7.0]
        want = "\n".join(lines) + "\n"
        got = open(os.path.join(tmp_path, f"{k}.csv")).read()
        assert got == want or _csv_close(got, want), (got, want)
        assert _csv_close(got, bytes(g11[f"track{k}_csv"]).decode())


def _csv_close(a: str, b: str) -> bool:
    """Same labels, coordinates within 1e-3 px (+ the 5e-4 of the printed rounding)."""
    ra = [ln.split(",") for ln in a.strip().split("\n")[1:]]
    rb = [ln.split(",") for ln in b.strip().split("\n")[1:]]
    return [r[0] for r in ra] == [r[0] for r in rb] and all(
        abs(float(x) - float(y)) <= 1.5e-3 for p, q in zip(ra, rb) for x, y in zip(p[1:], q[1:]))


def test_clean_under_debug_guards(g11, tmp_path):
    """IM_DEBUG_GUARDS=1: guard words around every library buffer (the C scratch included) stay intact through forient and a
    correlation launch at both default sizes."""
    np.save(tmp_path / "a.npy", g11["img0"])
    np.save(tmp_path / "b.npy", g11["img1"])
    code = f"""
import numpy as np
from icepy4d_amd import _lib
from icepy4d_amd.engine import Engine
from icepy4d_amd.matching.templatematch import OC, match_many
e = Engine(0)
A, B = np.load(r"{tmp_path / 'a.npy'}"), np.load(r"{tmp_path / 'b.npy'}")
pu, pv = np.meshgrid(np.arange(0.0, 640, 20), np.arange(0.0, 480, 20))
r = OC(A, B, pu.copy(), pv.copy(), 128, 144, engine=e)
m = match_many(A, [B, A], pu, pv, 32, 128, engine=e)
e.synchronize()
assert np.isfinite(r.du).sum() > 10 and np.isfinite(m["du"]).sum() > 10
del e
import gc; gc.collect()
print("guard failures", _lib.load().im_debug_guard_failures())
assert _lib.load().im_debug_guard_failures() == 0
"""
    env = dict(os.environ, IM_DEBUG_GUARDS="1", PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "guard failures 0" in p.stdout
