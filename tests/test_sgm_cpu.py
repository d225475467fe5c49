"""Semi-global regularisation of dense-stereo depth maps without a device: (a) the numpy restatement (tests/sgm_oracle.py) against a direct
per-path loop, its invariants and the quality condition on three noisy scenes, (b) a host build of the kernels' own arithmetic
(csrc/sgm_pixel.h and csrc/dense_pixel.h behind the stub <hip/hip_runtime.h>, in tests/sgm_host_harness.cpp, a stand-alone program built plain
and with the address and undefined-behaviour sanitizers) against the restatement bit for bit, (c) the ABI, the compiled resources of the
kernels and the option on `icepy4d_amd.dense`. The device run is tests/test_gpu_sgm.py."""
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
import sgm_cases as SC  # noqa: E402
import sgm_oracle as S  # noqa: E402

from icepy4d_amd import dense as D  # noqa: E402
from icepy4d_amd.dense import cost_volume, sgm_aggregate, sgm_choose  # noqa: E402,F401  (the feature under test: without it nothing here can pass)
from icepy4d_amd.core.camera import Camera  # noqa: E402

NAMES = ["im_dense_sgm_max_planes", "im_dense_costs", "im_dense_sgm", "im_dense_sgm_choose"]


# ---- (a) the restatement ------------------------------------------------------------------------------------------------------------------------
def direct_sum(cost, P1, P2, paths):
    """One pixel after another along every line of every direction, in Python integers."""
    h0, w0, Dn = cost.shape
    total = np.zeros((h0, w0, Dn), np.int64)
    for dy, dx in S.DIRECTIONS[:paths]:
        for y0 in range(h0):
            for x0 in range(w0):
                if 0 <= y0 - dy < h0 and 0 <= x0 - dx < w0:
                    continue                                         # not the first pixel of its line
                y, x, Lq = y0, x0, None
                while 0 <= y < h0 and 0 <= x < w0:
                    c = [int(v) for v in cost[y, x]]
                    if Lq is None:
                        L = c
                    else:
                        m = min(Lq)
                        L = []
                        for d in range(Dn):
                            terms = [Lq[d], m + P2]
                            if d - 1 >= 0:
                                terms.append(Lq[d - 1] + P1)
                            if d + 1 < Dn:
                                terms.append(Lq[d + 1] + P1)
                            L.append(c[d] + min(terms) - m)
                    total[y, x] += L
                    Lq, y, x = L, y + dy, x + dx
    return total


@pytest.mark.parametrize("shape,P1,P2,paths", [((7, 11, 5), 16, 128, 8), ((11, 7, 5), 7, 7, 8), ((6, 6, 1), 3, 9, 8), ((1, 9, 4), 0, 4095, 8),
                                               ((9, 1, 3), 4095, 4095, 8), ((5, 8, 6), 16, 128, 4), ((1, 1, 2), 1, 2, 8)])
def test_the_recurrence_equals_a_direct_loop_along_every_path(shape, P1, P2, paths):
    c = SC.random_volume(*shape)
    got = S.aggregate(c, P1, P2, paths)
    assert got.dtype == np.uint16 and np.array_equal(got.astype(np.int64), direct_sum(c, P1, P2, paths))


def test_without_penalties_the_sum_is_the_cost_times_the_paths():
    for name in ("random_17x65x5_p4", "random_17x65x64_p8", "shape_33x97_p8"):
        c, _, _, paths = SC.aggregations()[name]
        assert np.array_equal(S.aggregate(c, 0, 0, paths).astype(np.int64), paths * c.astype(np.int64)), name


def test_the_sum_never_exceeds_its_bound():
    worst = 0.0
    for name, (c, P1, P2, paths) in SC.aggregations().items():
        total = SC.aggregate_oracle(name)
        assert int(total.max()) <= paths * (255 + P2) <= 34800, name
        worst = max(worst, int(total.max()) / (paths * (255 + P2)))
    all_invalid = np.full((4, 6, 3), 255, np.uint8)
    assert int(S.aggregate(all_invalid, 4095, 4095, 8).max()) == 8 * 255          # m cancels what a constant line carries
    print("largest sum / bound:", worst)
    with pytest.raises(ValueError):
        S.aggregate(all_invalid, 5, 4, 8)
    with pytest.raises(ValueError):
        S.aggregate(all_invalid, 0, 4096, 8)
    with pytest.raises(ValueError):
        S.aggregate(all_invalid, 1, 2, 6)


def test_the_dequantised_score_lies_within_one_step_below_the_score():
    """c = floor((1 - s) 127) <= (1 - s) 127 < c + 1, so 1 - c / 127 lies in [s, s + 1 / 127) up to the rounding of three float64
    operations on values of magnitude <= 254 (at most 3 * 2^-53 * 254 / 127 < 1e-15 in the score); the clamp at 254 holds s >= -1."""
    for name in ("shape_33x97", "radius_3", "planes_65", "window_leaves_src"):
        c = SC.costs()[name]
        valid, s = O.scores(c["ref"], c["src"], c["A"], c["B"], c["w_first"], c["w_step"], c["D"], c["r"], c["min_var"])
        cost = np.moveaxis(SC.cost_oracle(name), -1, 0)
        assert ((cost == 255) == ~valid).all() and valid.any(), name
        back = 1.0 - cost[valid].astype(np.float64) / 127.0
        assert (back >= s[valid] - 1e-15).all() and (back < s[valid] + 1.0 / 127.0 + 1e-15).all(), name
    assert list(S.quantise(np.array([[[True]], [[True]], [[True]], [[False]]]), np.array([[[1.0]], [[-1.0]], [[-1.5]], [[1.0]]]))[0, 0]) == [0, 254, 254, 255]


def test_the_cases_reach_what_they_are_named_for():
    C = SC.choices()
    plane, w, _ = SC.choose_oracle("all_planes_tie")
    assert set(np.unique(plane)) == {-1, 0} and (w[plane == 0] == C["all_planes_tie"]["w_first"]).all()
    for name, k in (("best_at_first_plane", 0), ("best_at_last_plane", 4)):
        plane, w, _ = SC.choose_oracle(name)
        kept = plane >= 0
        assert kept.any() and (plane[kept] == k).all() and (w[kept] == C[name]["w_first"] + float(k) * C[name]["w_step"]).all()
    # an invalid neighbour and a flat sum: no offset; the plain volume under them has offsets
    for name in ("invalid_neighbour", "flat_sum"):
        c = C[name]
        plane, w, _ = SC.choose_oracle(name)
        assert (plane >= 0).all() and (w == c["w_first"] + plane.astype(np.float64) * c["w_step"]).all(), name
    c = C["min_score_drops"]
    plane, w, score = SC.choose_oracle("min_score_drops")
    free = S.choose(c["cost"], c["sum"], c["w_first"], c["w_step"], -2.0)
    assert (free[1] != c["w_first"] + free[0].astype(np.float64) * c["w_step"]).any()                    # offsets in use
    assert (free[0] >= 0).all() and 0 < (plane < 0).sum() < plane.size and (free[2][plane < 0] < 0.3).all() and (score[plane >= 0] >= 0.3).all()
    assert (w[plane < 0] == 0).all() and (score[plane < 0] == 0).all()
    c = C["all_invalid_pixels"]
    plane = SC.choose_oracle("all_invalid_pixels")[0]
    dead = (c["cost"] == 255).all(2)
    assert dead.any() and not dead.all() and ((plane < 0) == dead).all()
    c = C["least_sum_is_invalid"]
    plane = SC.choose_oracle("least_sum_is_invalid")[0]
    assert (c["sum"].argmin(2) != plane).all() and (plane >= 0).all()
    plane = SC.choose_oracle("ties_between_neighbours")[0]
    assert (C["ties_between_neighbours"]["sum"].astype(np.int64).argmin(2) == plane).all()                # argmin takes the first of equals
    assert SC.choose_oracle("planes_256")[0].max() > 128
    # costs: the special cases hold what they are named for
    assert (SC.cost_oracle("ref_smaller_than_window") == 255).all() and (SC.cost_oracle("nan_in_A") == 255).all()
    inner = SC.cost_oracle("window_leaves_src")[2:-2, 2:-2]
    assert (inner == 255).any() and (inner != 255).any()
    for name in ("constant_patch_in_ref", "constant_patch_in_src"):
        c, inner = SC.costs()[name], slice(2, -2)                                    # r = 2: planes that do not score inside the border
        dead4 = (SC.cost_oracle(name)[inner, inner] == 255).sum()
        assert dead4 >= (SC.cost_oracle(name + "_min_var_0")[inner, inner] == 255).sum() and dead4 > 0 and c["r"] == 2, name
    assert SC.cost_oracle("planes_256").shape == (9, 20, 256) and (SC.cost_oracle("planes_256")[1:-1, 1:-1] != 255).all()
    # aggregation: volumes with 255s, and pixels that are 255 throughout
    c = SC.random_volume(17, 65, 5)
    assert (c == 255).any() and (c == 255).all(2).any() and not (c == 255).all()


def test_semi_global_aggregation_recovers_what_noise_scatters():
    """The three noisy scenes (contrast 0.25 about grey level 128 on both images, Gaussian noise on ref, min_var 0, min_score -2) at
    P1 = 16, P2 = 128, eight paths: the share of interior pixels within one plane of the truth. Measured with this restatement
    (winner-take-all -> semi-global, gain): seed 200 0.537 -> 0.926 (+0.389), seed 201 0.440 -> 0.803 (+0.363), seed 202 0.560 -> 0.924
    (+0.364); no pixel dropped by either. Asserted: the gain the issue sets (>= 0.25) and that nothing is dropped."""
    for seed in SC.NOISY:
        c = SC.noisy(seed)
        wta, sgm = SC.noisy_oracle(seed)
        before, after = SC.share_within_one_plane(wta[0], c), SC.share_within_one_plane(sgm[0], c)
        print(seed, "winner-take-all", round(before, 4), "semi-global", round(after, 4), "gain", round(after - before, 4))
        assert after - before >= 0.25, (seed, before, after)
        r = c["r"]
        assert (sgm[0][r:-r, r:-r] >= 0).all(), seed


# ---- (b) the host build of the kernels' arithmetic ---------------------------------------------------------------------------------------------
def record(f, kind, name, ints, doubles, arrays):
    f.write(struct.pack("<qq", kind, len(name)) + name.encode())
    f.write(np.asarray(ints, np.int64).tobytes() + np.asarray(doubles, np.float64).tobytes())
    for a, t in arrays:
        f.write(np.ascontiguousarray(a, t).tobytes())


def write_records(path):
    n = 0
    with open(path, "wb") as f:
        for name, c in SC.costs().items():
            record(f, 1, "cost " + name, [*c["ref"].shape, *c["src"].shape, c["D"], c["r"], c["min_var"]], [*c["A"], *c["B"], c["w_first"], c["w_step"]],
                   [(c["ref"], np.uint8), (c["src"], np.uint8), (SC.cost_oracle(name), np.uint8)])
            n += 1
        for name, (c, P1, P2, paths) in SC.aggregations().items():
            record(f, 2, "aggregate " + name, [*c.shape, P1, P2, paths], [], [(c, np.uint8), (SC.aggregate_oracle(name), np.uint16)])
            n += 1
        for name, c in SC.choices().items():
            plane, w, score = SC.choose_oracle(name)
            record(f, 3, "choose " + name, c["cost"].shape, [c["w_first"], c["w_step"], c["min_score"]],
                   [(c["cost"], np.uint8), (c["sum"], np.uint16), (plane, np.int16), (w, np.float64), (score, np.float32)])
            n += 1
        for seed in SC.NOISY:
            c = SC.noisy(seed)
            cost = SC.volume_of(c)
            plane, w, score = SC.noisy_oracle(seed)[1]
            record(f, 1, f"cost noisy {seed}", [*c["ref"].shape, *c["src"].shape, c["D"], c["r"], c["min_var"]], [*c["A"], *c["B"], c["w_first"], c["w_step"]],
                   [(c["ref"], np.uint8), (c["src"], np.uint8), (cost, np.uint8)])
            total = S.aggregate(cost, SC.P1, SC.P2, SC.PATHS)
            record(f, 2, f"aggregate noisy {seed}", [*cost.shape, SC.P1, SC.P2, SC.PATHS], [], [(cost, np.uint8), (total, np.uint16)])
            record(f, 3, f"choose noisy {seed}", cost.shape, [c["w_first"], c["w_step"], c["min_score"]],
                   [(cost, np.uint8), (total, np.uint16), (plane, np.int16), (w, np.float64), (score, np.float32)])
            n += 3
    return n


@pytest.fixture(scope="module")
def harness_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sgm_host"))
    n = write_records(os.path.join(d, "records.bin"))
    return d, n


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_equals_the_restatement_bit_for_bit(harness_dir, sanitize):
    d, n = harness_dir
    exe = toolchain.host_program(d, "sgm_host_harness.cpp", sanitize)
    r = subprocess.run([exe, os.path.join(d, "records.bin")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout[-3000:] + r.stderr[-3000:]
    assert n == len(SC.costs()) + len(SC.aggregations()) + len(SC.choices()) + 3 * len(SC.NOISY)
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == n and "DIFFERENT" not in r.stdout and "MISSING" not in r.stdout


# ---- (c) the ABI, the kernels' resources and the option --------------------------------------------------------------------------------------------
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
    assert lib.im_dense_sgm_max_planes() == D.MAX_SGM_PLANES == S.MAX_PLANES == 256 and D.MAX_PENALTY == S.MAX_PENALTY == 4095
    with open(os.path.join(toolchain.CSRC, "sgm_pixel.h")) as f:
        text = f.read()
    assert "SGM_MAX_PLANES = 256" in text and "SGM_MAX_PENALTY = 4095" in text and "#pragma clang fp contract(off)" in text
    assert "sqrt" not in text and "fma" not in text                              # + - * / and floor only


def test_the_kernels_spill_nothing(tmp_path):
    """Three kernels. The cost kernel holds dense_sweep_kernel's LDS and 16 KiB of staged planes (two blocks fit the 160 KiB of a CU); the
    aggregation holds a line's path costs, four pixels of prefetched costs and sums, and no LDS."""
    res = toolchain.kernel_resources(toolchain.device_listing("dense_sgm.hip", str(tmp_path)))
    assert len(res) == 3 and all(any(k in name for name in res) for k in ("dense_costs_kernel", "dense_sgm_kernel", "dense_sgm_choose_kernel")), sorted(res)
    for k, f in res.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (k, dict(f))
        print(k, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "lds", f["group_segment_fixed_size"])
        assert f["max_flat_workgroup_size"] == 256
    cost = [f for k, f in res.items() if "dense_costs" in k][0]
    lds = 30 * 78 * (1 + 4) + 30 * 64 * (8 + 8) + 20 * 8 + 64 * 16 * 16
    assert lds <= cost["group_segment_fixed_size"] <= lds + 64 and 2 * (lds + 64) <= 160 * 1024 and cost["vgpr_count"] <= 256
    agg = [f for k, f in res.items() if "dense_sgm_kernel" in k][0]
    assert agg["group_segment_fixed_size"] == 0 and agg["vgpr_count"] <= 128           # four waves per SIMD and more


def cameras():
    K = np.array([[1200.0, 0.0, 400.0], [0.0, 1200.0, 300.0], [0.0, 0.0, 1.0]])
    return [Camera(800, 600, K=K, R=np.eye(3), t=np.zeros(3)), Camera(800, 600, K=K, R=np.eye(3), t=np.array([-1.0, 0.02, 0.05]))]


REFUSALS = [
    ("an unknown regularisation", dict(regularisation="tv"), "regularisation"),
    ("a negative p1", dict(p1=-1), "p1 <= p2"),
    ("p1 above p2", dict(p1=200), "p1 <= p2"),
    ("p2 above 4095", dict(p2=4096), "p1 <= p2"),
    ("a fractional penalty", dict(p1=1.5), "p1 <= p2"),
    ("six paths", dict(paths=6), "paths"),
    ("more than 256 planes", dict(depth_range=(4.0, 60.0)), "downscale or max_step_px"),
    ("an unknown filter", dict(depth_filter="Moderate"), "invalid choise of depth filtering"),
    ("radius 8", dict(radius=8), "radius"),
]


@pytest.mark.parametrize("what,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_python_layer_refuses_before_any_device_work(what, change, text, monkeypatch):
    from icepy4d_amd import engine
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    monkeypatch.setattr(D, "default_engine", lambda e: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    args = dict(images=[np.zeros((600, 800), np.uint8), np.zeros((600, 800), np.uint8)], cameras=cameras(), depth_range=(20.0, 60.0), regularisation="sgm")
    args.update(change)
    with pytest.raises(ValueError, match=text):
        D.build_dense_cloud(**args)
    if what == "more than 256 planes":                                            # the plain sweep takes that schedule
        c0, c1 = cameras()
        assert 256 < D.plane_schedule(c0, c1, 4.0, 60.0, 1.0)[2] <= D.MAX_PLANES


def test_the_lower_functions_refuse_before_any_device_work(monkeypatch):
    import torch
    monkeypatch.setattr(D, "default_engine", lambda e: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    img = torch.zeros((20, 30), dtype=torch.uint8)
    A = np.eye(3).reshape(9)
    for change, text in ((dict(D=257), "downscale"), (dict(D=0), "planes"), (dict(radius=0), "radius"), (dict(min_var=-1), "min_var")):
        a = dict(D=5, radius=1, min_var=4)
        a.update(change)
        with pytest.raises(ValueError, match=text):
            D.cost_volume(img, img, A, A, 0.1, 0.01, a["D"], a["radius"], a["min_var"])
    cost = torch.zeros((4, 5, 3), dtype=torch.uint8)
    for bad in (dict(P1=-1), dict(P1=9, P2=8), dict(P2=4096), dict(paths=5)):
        with pytest.raises(ValueError):
            D.sgm_aggregate(cost, **bad)
    for bad in (cost.to(torch.int16), cost[0], torch.zeros((4, 5, 257), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            D.sgm_aggregate(bad)
    with pytest.raises(ValueError, match="uint16"):
        D.sgm_choose(cost, cost, 0.1, 0.01)
    with pytest.raises(ValueError, match="regularisation"):
        D.sweep(img, img, A, A, 0.1, 0.01, 5, regularisation="semi")
    with pytest.raises(ValueError, match="downscale"):
        D.sweep(img, img, A, A, 0.1, 0.01, 300, regularisation="sgm")


class FakeContext:
    def __init__(self):
        self.names = []

    def call(self, name, *args):
        self.names.append(name)


class FakeEngine:
    def __init__(self):
        import torch
        self.device, self.ctx = torch.device("cpu"), FakeContext()

    def stream_ptr(self):
        return None


def test_without_the_option_no_new_call_is_made(monkeypatch):
    """`regularisation=None` is today's path: two im_dense_sweep calls per pair and nothing else; "sgm" makes the three new calls per view
    and no sweep. The context's `call` is replaced, so no device is needed."""
    images = [np.zeros((60, 80), np.uint8), np.zeros((60, 80), np.uint8)]
    K = np.array([[120.0, 0.0, 40.0], [0.0, 120.0, 30.0], [0.0, 0.0, 1.0]])
    cams = [Camera(80, 60, K=K, R=np.eye(3), t=np.zeros(3)), Camera(80, 60, K=K, R=np.eye(3), t=np.array([-1.0, 0.0, 0.0]))]
    eng = FakeEngine()
    monkeypatch.setattr(D, "default_engine", lambda e: eng)
    D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng)
    assert eng.ctx.names == ["im_dense_sweep", "im_dense_sweep"]
    eng.ctx.names.clear()
    D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng, regularisation=None, p1=1, p2=2, paths=4)
    assert eng.ctx.names == ["im_dense_sweep", "im_dense_sweep"]
    eng.ctx.names.clear()
    maps = D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng, regularisation="sgm")
    assert eng.ctx.names == ["im_dense_costs", "im_dense_sgm", "im_dense_sgm_choose"] * 2
    assert maps[0].plane.shape == (60, 80) and maps[0].w.dtype == __import__("torch").float64


def test_dense_series_hands_the_option_down(monkeypatch):
    calls = []
    monkeypatch.setattr(D, "build_dense_cloud", lambda images, cameras, **kw: calls.append(kw) or len(calls))
    D.dense_series([["a0", "a1"]], cameras(), regularisation="sgm", p1=8, p2=64, paths=4)
    assert calls[0]["regularisation"] == "sgm" and (calls[0]["p1"], calls[0]["p2"], calls[0]["paths"]) == (8, 64, 4)
