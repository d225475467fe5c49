"""Template matching without a device: the numpy oracle (tests/oc_oracle.py) against the reference's own outputs
(tests/golden/g11_templatematch.npz, tools/gen_golden_templatematch.py), and the host side of the public API."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oc_oracle  # noqa: E402

CASES = {"grid": ("img0", "img1"), "grid_s": ("img1", "img2"), "grid_p": ("img2", "img3"), "odd": ("img0", "img3"),
         "float": ("float_a", "float_b"), "synth": ("synth_a", "synth_b")}
KEYS = ("pu", "pv", "du", "dv", "peakCorr", "meanAbsCorr")


@pytest.fixture(scope="module")
def g11():
    return oc_oracle.load_g11(os.path.join(ROOT, "tests", "golden", "g11_templatematch.npz"))


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_equals_reference_outputs(g11, case):
    T, S = (int(v) for v in g11[case + "_TS"])
    a, b = CASES[case]
    r = oc_oracle.oc(g11[a], g11[b], g11[case + "_pu_in"], g11[case + "_pv_in"], T, S, g11[case + "_initdu"], g11[case + "_initdv"])
    for k in KEYS:
        assert np.array_equal(np.isnan(r[k]), np.isnan(g11[f"{case}_{k}"])), k
    assert np.array_equal(r["pu"], g11[case + "_pu"], equal_nan=True) and np.array_equal(r["pv"], g11[case + "_pv"], equal_nan=True)
    for k in ("du", "dv"):
        assert np.nanmax(np.abs(r[k] - g11[f"{case}_{k}"]), initial=0) <= 1e-4
    for k in ("peakCorr", "meanAbsCorr"):
        assert np.nanmax(np.abs(r[k] - g11[f"{case}_{k}"]), initial=0) <= 1e-6 * T * T


def test_fixture_covers_nan_paths(g11):
    """Out-of-bounds points (everything NaN), an edge peak (meanAbsCorr kept, du NaN) and a NaN target are all in the fixture."""
    assert np.any(np.isnan(g11["synth_du"]) & ~np.isnan(g11["synth_meanAbsCorr"]))
    assert np.any(np.isnan(g11["grid_p_meanAbsCorr"])) and np.any(np.isnan(g11["odd_meanAbsCorr"]))
    assert np.isnan(g11["track_targets"]).any() and np.isnan(g11["track0_pu"]).any()


@pytest.mark.parametrize("name", ["forient_u8", "forient_f32"])
def test_oracle_forient(g11, name):
    ref = g11[name]
    mine = oc_oracle.forient(g11[name + "_in"])
    assert mine.dtype == np.complex64 and mine.shape == ref.shape
    assert np.abs(mine.real - ref.real).max() <= 4e-7 and np.abs(mine.imag - ref.imag).max() <= 4e-7
    assert np.array_equal(mine == 0, ref == 0)
    if name == "forient_u8":   # the gradient itself is exact: its direction matches the reference's to the rounding of the division
        re, im = oc_oracle.forient_parts(g11[name + "_in"])
        assert np.array_equal(re, np.round(re)) and np.array_equal(im, np.round(im))
        assert np.array_equal(np.sign(re), np.sign(ref.real)) and np.array_equal(np.sign(im), np.sign(ref.imag))


def test_validation_errors_match_reference():
    from icepy4d_amd.matching.templatematch import TemplateMatch
    A = np.zeros((50, 60), np.uint8)
    xy = np.array([[10.0, 20.0], [30.0, 25.0]])
    with pytest.raises(ValueError, match="Provide grayscale images"):
        TemplateMatch(np.zeros((50, 60, 3)), A, xy)
    with pytest.raises(ValueError, match="Invalid xy shape"):
        TemplateMatch(A, A, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="Invalid method"):
        TemplateMatch(A, A, xy, method="NCC")


def test_define_grid_and_single_points():
    from icepy4d_amd.matching.templatematch import TemplateMatch
    A = np.zeros((300, 400), np.uint8)
    xy = np.array([[10.0, 20.0], [30.0, 25.0], [50.5, 70.0]])
    t = TemplateMatch(A, A, xy, template_width=32, search_width=64)
    assert np.array_equal(t.pu, np.tile(xy[:, 0], (3, 1))) and np.array_equal(t.pv, np.tile(xy[:, 1:2], (1, 3)))
    s = TemplateMatch(A, A, xy, single_points=True)
    assert np.array_equal(np.diag(s.pu), xy[:, 0]) and np.isnan(s.pu[~np.eye(3, dtype=bool)]).all()
    # step form: x from S/2 to W - S/2 + T/2 (exclusive), every step_x; y likewise
    gu, gv = t.define_grid(step_x=50, step_y=40)
    assert np.array_equal(gu[0], np.arange(32.0, 400 - 32 + 16, 50)) and np.array_equal(gv[:, 0], np.arange(32.0, 300 - 32 + 16, 40))
    with pytest.raises(ValueError, match="step_x and step_y"):
        t.define_grid(step_x=5)
    mask = np.zeros(gu.shape, bool)
    mask[1, 2] = mask[3, 4] = True
    mu, mv = t.define_grid(step_x=50, step_y=40, mask=mask)
    assert np.array_equal(mu, np.meshgrid([132.0, 232.0], [72.0, 152.0])[0])
    assert np.array_equal(mv, np.meshgrid([132.0, 232.0], [72.0, 152.0])[1])


def test_match_result_snr():
    from icepy4d_amd.matching.templatematch import MatchResult
    pk, mc = np.array([[8.0, np.nan]]), np.array([[2.0, 1.0]])
    r = MatchResult(np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)), pk, mc, method="OC")
    assert r.snr[0, 0] == 4.0 and np.isnan(r.snr[0, 1]) and r.method == "OC"


def test_track_targets_validation(tmp_path):
    from icepy4d_amd.utils.track_targets import TrackTargets
    A = np.zeros((50, 60), np.uint8)
    t = np.array([[10.0, 20.0]])
    with pytest.raises(TypeError):
        TrackTargets(A, A, t, out_dir=str(tmp_path))
    with pytest.raises(TypeError):
        TrackTargets(3, [A], t, out_dir=str(tmp_path))
    with pytest.raises(TypeError):
        TrackTargets(A, [A], np.zeros((2, 3)), out_dir=str(tmp_path))
    with pytest.raises(ValueError, match="currentely not supported"):
        TrackTargets(A, [A], t, method="NCC", out_dir=str(tmp_path))
    with pytest.warns(UserWarning, match="viz_tracked"):
        tr = TrackTargets(A, [A], t, out_dir=str(tmp_path), viz_tracked=True)
    assert tr.cfg["template_width"] == 32 and tr.cfg["search_width"] == 128 and tr.cfg["snr_threshold"] == 7.0


def test_no_cpu_fallback_without_device(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from icepy4d_amd.matching.templatematch import OC, TemplateMatch, forient
    from icepy4d_amd.utils.track_targets import TrackTargets
    A = np.zeros((200, 200), np.uint8)
    with pytest.raises(RuntimeError):
        forient(A)
    with pytest.raises(RuntimeError):
        OC(A, A, np.array([[100.0]]), np.array([[100.0]]), 32, 64)
    with pytest.raises(RuntimeError):
        TemplateMatch(A, A, np.array([[100.0, 100.0]]), template_width=32, search_width=64).match()
    with pytest.raises(RuntimeError):
        TrackTargets(A, [A], np.array([[100.0, 100.0]]), out_dir=str(tmp_path), target_names=["a"]).track()
