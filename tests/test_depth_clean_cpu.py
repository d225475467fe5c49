"""Depth-map clean-up without a device: (a) the restatement (tests/depth_oracle.py) against an independent flood fill, its invariants and
the quality condition on three noisy scenes, (b) a host build of the kernels' own rules (csrc/depth_pixel.h behind the stub
<hip/hip_runtime.h>, in tests/depth_host_harness.cpp, a stand-alone program built plain and with the address and undefined-behaviour
sanitizers) against the restatement bit for bit, (c) the ABI, the compiled resources of the kernels and the options on
`icepy4d_amd.dense`. The device run is tests/test_gpu_depth_clean.py."""
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
import depth_cases as C  # noqa: E402
import depth_oracle as DO  # noqa: E402
import sgm_cases as SC  # noqa: E402

from icepy4d_amd import dense as D  # noqa: E402
from icepy4d_amd.dense import depth_components, remove_speckles, fill_holes  # noqa: E402,F401  (the feature under test: without it nothing here can pass)
from icepy4d_amd.core.camera import Camera  # noqa: E402

NAMES = ["im_depth_tile_w", "im_depth_tile_h", "im_depth_components", "im_depth_drop_small", "im_depth_fill_holes"]


# ---- (a) the restatement ------------------------------------------------------------------------------------------------------------------------
def flood_components(plane, mode, max_diff):
    """Labels and sizes by a flood fill from every unvisited member in row-major order: the seed is the least index of its component."""
    h, w = plane.shape
    label, size = np.full((h, w), -1, np.int32), np.zeros((h, w), np.int32)
    member = (plane >= 0) if mode == 0 else (plane < 0)
    for y0 in range(h):
        for x0 in range(w):
            if not member[y0, x0] or label[y0, x0] >= 0:
                continue
            label[y0, x0] = y0 * w + x0
            stack, found = [(y0, x0)], [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for v, u in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                    if 0 <= v < h and 0 <= u < w and member[v, u] and label[v, u] < 0 and (mode == 1 or abs(int(plane[y, x]) - int(plane[v, u])) <= max_diff):
                        label[v, u] = y0 * w + x0
                        stack.append((v, u))
                        found.append((v, u))
            for v, u in found:
                size[v, u] = len(found)
    return label, size


FLOODED = ["shape_1x1_mode0", "shape_1x70_mode1", "shape_70x1_mode0", "shape_2x2_mode1", "shape_17x65_mode0", "shape_17x65_mode1", "checkerboard",
           "serpentine_mode0", "serpentine_transposed_mode1", "spiral_mode0", "spiral_mode1", "tiles_meet_at_a_corner", "chain_345_against_pair_35",
           "difference_of_exactly_max_diff", "random_65x130_density_0.3_mode0", "random_65x130_density_0.6_mode1", "random_65x130_density_0.9_mode0",
           "all_invalid_mode1", "all_valid_mode0"]


@pytest.mark.parametrize("name", FLOODED)
def test_the_union_find_equals_a_flood_fill(name):
    plane, mode, max_diff = C.labellings()[name]
    label, size = C.label_oracle(name)
    want = flood_components(plane, mode, max_diff)
    assert label.dtype == np.int32 and size.dtype == np.int32 and np.array_equal(label, want[0]) and np.array_equal(size, want[1])


@pytest.mark.parametrize("name", list(C.labellings()))
def test_labels_are_least_indices_and_sizes_sum_to_the_members(name):
    plane, mode, max_diff = C.labellings()[name]
    label, size = C.label_oracle(name)
    h, w = plane.shape
    member = (plane >= 0) if mode == 0 else (plane < 0)
    idx = np.arange(h * w).reshape(h, w)
    assert ((label >= 0) == member).all() and ((size > 0) == member).all() and (label[member] <= idx[member]).all()
    roots = np.unique(label[member])
    assert (label.reshape(-1)[roots] == roots).all()                              # a root is labelled with itself: the least index
    assert int(size.reshape(-1)[roots].sum()) == int(member.sum())
    for r in roots[:50]:
        assert int((label == r).sum()) == int(size.reshape(-1)[r])


def test_the_cases_reach_what_they_are_named_for():
    L = C.label_oracle
    assert (L("one_component_3x3_tiles")[0] == 0).all() and (L("one_component_3x3_tiles")[1] == C.H3 * C.W3).all()
    assert (L("one_hole_3x3_tiles")[0] == 0).all()
    assert (L("checkerboard")[1] == 1).all() and (L("checkerboard_joined_at_100")[1] == C.H3 * C.W3).all()
    for name in ("serpentine_mode0", "serpentine_transposed_mode0", "spiral_mode0"):
        plane = C.labellings()[name][0]
        label, size = L(name)
        assert len(np.unique(label[plane >= 0])) == 1 and size.max() == (plane >= 0).sum() > 1000, name       # one long path
    assert len(np.unique(L("spiral_mode1")[0][C.labellings()["spiral_mode1"][0] < 0])) == 1                   # and one long gap beside it
    assert len(np.unique(L("serpentine_mode1")[0])) > 20
    corner = L("tiles_meet_at_a_corner")[0]
    assert corner[C.TILE_H - 1, C.TILE_W - 1] == 0 and corner[C.TILE_H, C.TILE_W] == C.TILE_H * 2 * C.TILE_W + C.TILE_W      # diagonal neighbours stay apart
    assert len(np.unique(L("holes_meet_at_a_corner")[0])) == 3
    for name in ("joined_through_the_last_column", "joined_through_the_last_row"):
        plane = C.labellings()[name][0].copy()
        assert len(np.unique(L(name)[0])) == 2                                    # -1 and one component
        if "column" in name:
            plane[C.TILE_H, -1] = -1
        else:
            plane[-1, C.TILE_W] = -1
        assert len(np.unique(DO.components(plane, 0, 1)[0])) == 3, name           # without the bridge there are two
    chain = L("chain_345_against_pair_35")[1]
    assert list(chain[1, :6]) == [3, 3, 3, 0, 1, 1]
    exact = L("difference_of_exactly_max_diff")[1]
    assert list(exact[1, :5]) == [2, 2, 0, 1, 1] and exact[0, 7] == 1 and L("difference_of_4095")[1][0, 7] == 2
    # speckles
    plane = C.speckle_oracle("sizes_min_size_and_one_less")[1]
    assert (plane[2, 3:8] >= 0).all() and (plane[5, 3:7] < 0).all() and (plane[8:10, 20:23] >= 0).all() and plane[12, 40] < 0
    assert C.speckle_oracle("sizes_min_size_and_one_less")[4] == 5
    assert C.speckle_oracle("all_valid_dropped_whole")[4] == 20 * 70 and C.speckle_oracle("all_valid_one_component")[4] == 0
    assert 0 < C.speckle_oracle("random_65x130")[4] < (C.speckles()["random_65x130"]["plane"] >= 0).sum()
    # holes
    H = C.hole_oracle
    f = H("holes_at_the_four_borders")[5]
    assert f.sum() == 12 and f[25:28, 100:104].all()
    assert H("hole_over_tile_edges")[5].sum() == 16 + 6
    f = H("sizes_max_hole_and_one_more")[5]
    assert f[5:8, 10:14].all() and f.sum() == 12
    f = H("rim_spread_max_diff_and_one_more")[5]
    assert f[10:13, 38:42].all() and not f[10:13, 118:122].any() and f[20:22, 78:82].all()
    assert H("l_shaped_hole")[5].sum() == 15
    assert H("hole_with_an_island")[5].sum() == 30 and H("hole_with_an_island_kept")[5].sum() == 28
    assert H("one_pixel_holes")[5].sum() == 5
    c = C.holes()["plane_beyond_the_schedule"]
    out = H("plane_beyond_the_schedule")
    assert out[5].sum() == 12 and (out[2][25:27, 130:133] == 5).all() and ((out[3][25:27, 130:133] - c["w_first"]) / c["w_step"] > 6.0).all()
    out = H("plane_before_the_schedule")
    assert (out[2][10:12, 10:13] == 0).all() and (out[3][10:12, 10:13] < C.holes()["plane_before_the_schedule"]["w_first"]).all()
    out = H("negative_w_step")
    assert out[5].sum() == 12 and (np.abs(out[2][out[5] == 1] - (out[3][out[5] == 1] - 0.5) / -0.01) <= 0.5).all()
    out = H("ties_round_to_even")
    assert out[3][1, 2] == 2.5 and out[2][1, 2] == 2 and out[3][3, 5] == 3.5 and out[2][3, 5] == 4
    assert H("all_invalid")[6] == 0 and H("all_valid")[6] == 0 and H("random_65x130")[6] > 100 and H("random_3x3_tiles_plus")[6] > 100
    for name in C.holes():
        out = H(name)
        assert (out[4][out[5] == 1] == 0).all() and (out[2][out[5] == 1] >= 0).all() and out[6] == out[5].sum(), name


def test_min_size_1_and_a_max_hole_below_every_hole_are_identities():
    for name, c in C.speckles().items():
        _, size = DO.components(c["plane"], 0, c["max_diff"])
        out = DO.drop_small(c["plane"], c["w"], c["score"], size, 1)
        assert out[3] == 0 and all(np.array_equal(a, b) for a, b in zip(out[:3], (c["plane"], c["w"], c["score"]))), name
    c = C.holes()["sizes_max_hole_and_one_more"]
    out = DO.fill_holes(c["plane"], c["w"], c["score"], 11, 2, c["w_first"], c["w_step"], c["D"])
    assert out[4] == 0 and not out[3].any() and all(np.array_equal(a, b) for a, b in zip(out[:3], (c["plane"], c["w"], c["score"])))
    for bad in (dict(mode=2), dict(max_diff=-1), dict(max_diff=4096)):
        a = dict(mode=0, max_diff=1)
        a.update(bad)
        with pytest.raises(ValueError):
            DO.components(c["plane"], a["mode"], a["max_diff"])
    with pytest.raises(ValueError):
        DO.fill_holes(c["plane"], c["w"], c["score"], 4097, 2, c["w_first"], c["w_step"], c["D"])
    with pytest.raises(ValueError):
        DO.fill_holes(c["plane"], c["w"], c["score"], 64, 2, c["w_first"], 0.0, c["D"])


def test_speckle_removal_drops_the_wrong_and_keeps_the_right():
    """The three noisy scenes of tests/sgm_cases.py, winner-take-all maps, min_size 16, max_diff 1, interior pixels. Asserted, as the issue
    sets them: at least 0.70 of the kept pixels farther than one plane from the truth are dropped, at least 0.80 of those within one plane
    survive, and at least 0.95 of the interior pixels that `fill_holes(max_hole=64, max_diff=2)` then fills lie within one plane of the truth
    (their interpolated w in plane steps; the rounded plane is printed beside it). Measured with this restatement, right / wrong before ->
    after: seed 200 1580 / 1365 -> 1410 / 108, seed 201 1297 / 1648 -> 1085 / 284, seed 202 1330 / 1046 -> 1255 / 262; filled within one
    plane 208 of 209, 83 of 85, 128 of 128."""
    counts = {}
    for seed in SC.NOISY:
        c = SC.noisy(seed)
        wta, _ = SC.noisy_oracle(seed)
        clean, full, filled = C.noisy_chain(seed)
        (r0, w0), (r1, w1) = C.right_and_wrong(wta[0], c), C.right_and_wrong(clean[0], c)
        assert not (r1 & ~r0).any() and not (w1 & ~w0).any()                      # nothing appears
        dropped, surviving = 1.0 - w1.sum() / w0.sum(), r1.sum() / r0.sum()
        r = c["r"]
        inner = filled[r:-r, r:-r] == 1
        k = (full[1][r:-r, r:-r] - c["w_first"]) / c["w_step"]
        near = inner & (np.abs(k - c["k_true"][r:-r, r:-r]) <= 1.0)
        near_plane = inner & (np.abs(full[0][r:-r, r:-r] - c["k_true"][r:-r, r:-r]) <= 1.0)
        counts[seed] = (int(r0.sum()), int(w0.sum()), int(r1.sum()), int(w1.sum()), int(inner.sum()), int(near.sum()))
        print(seed, "right / wrong", counts[seed][:2], "->", counts[seed][2:4], "dropped", round(dropped, 3), "surviving", round(surviving, 3),
              "filled", int(inner.sum()), "within one plane", int(near.sum()), "by the rounded plane", int(near_plane.sum()))
        assert dropped >= 0.70 and surviving >= 0.80, (seed, dropped, surviving)
        assert near.sum() >= 0.95 * inner.sum() and inner.sum() > 50, (seed, int(near.sum()), int(inner.sum()))
        assert (clean[1][clean[0] < 0] == 0).all() and (clean[2][clean[0] < 0] == 0).all()
    assert counts == {200: (1580, 1365, 1410, 108, 209, 208), 201: (1297, 1648, 1085, 284, 85, 83), 202: (1330, 1046, 1255, 262, 128, 128)}


def test_speckle_removal_on_the_regularised_maps_costs_little():
    """On the semi-global maps of the same scenes: a further 101 / 117 / 8 wrong pixels go at a cost of 5 / 3 / 0 right ones."""
    got = []
    for seed in SC.NOISY:
        c = SC.noisy(seed)
        _, sgm = SC.noisy_oracle(seed)
        plane = DO.remove_speckles(*sgm, *C.SPECKLE)[0]
        (r0, w0), (r1, w1) = C.right_and_wrong(sgm[0], c), C.right_and_wrong(plane, c)
        got.append((int(w0.sum() - w1.sum()), int(r0.sum() - r1.sum())))
    print(got)
    assert got == [(101, 5), (117, 3), (8, 0)]


# ---- (b) the host build of the kernels' rules ---------------------------------------------------------------------------------------------------
def record(f, kind, name, ints, doubles, arrays):
    f.write(struct.pack("<qq", kind, len(name)) + name.encode())
    f.write(np.asarray(ints, np.int64).tobytes() + np.asarray(doubles, np.float64).tobytes())
    for a, t in arrays:
        f.write(np.ascontiguousarray(a, t).tobytes())


def write_records(path):
    n = 0
    with open(path, "wb") as f:
        for name, (plane, mode, max_diff) in C.labellings().items():
            label, size = C.label_oracle(name)
            record(f, 1, "label " + name, [*plane.shape, mode, max_diff], [], [(plane, np.int16), (label, np.int32), (size, np.int32)])
            n += 1
        for name, c in C.speckles().items():
            _, plane, w, score, count = C.speckle_oracle(name)
            record(f, 2, "drop " + name, [*c["plane"].shape, c["min_size"], c["max_diff"], count], [],
                   [(c["plane"], np.int16), (c["w"], np.float64), (c["score"], np.float32), (plane, np.int16), (w, np.float64), (score, np.float32)])
            n += 1
        for name, c in C.holes().items():
            src = C.hole_input(name)
            _, _, plane, w, score, filled, count = C.hole_oracle(name)
            record(f, 3, "fill " + name, [*src[0].shape, c["max_hole"], c["max_diff"], c["D"], count], [c["w_first"], c["w_step"]],
                   [(src[0], np.int16), (src[1], np.float64), (src[2], np.float32), (plane, np.int16), (w, np.float64), (score, np.float32), (filled, np.uint8)])
            n += 1
        for seed in SC.NOISY:
            c = SC.noisy(seed)
            wta, _ = SC.noisy_oracle(seed)
            clean, full, filled = C.noisy_chain(seed)
            record(f, 2, f"drop noisy {seed}", [*wta[0].shape, *C.SPECKLE, int((wta[0] >= 0).sum() - (clean[0] >= 0).sum())], [],
                   [(wta[0], np.int16), (wta[1], np.float64), (wta[2], np.float32), (clean[0], np.int16), (clean[1], np.float64), (clean[2], np.float32)])
            record(f, 3, f"fill noisy {seed}", [*wta[0].shape, *C.HOLES, c["D"], int(filled.sum())], [c["w_first"], c["w_step"]],
                   [(clean[0], np.int16), (clean[1], np.float64), (clean[2], np.float32), (full[0], np.int16), (full[1], np.float64), (full[2], np.float32),
                    (filled, np.uint8)])
            n += 2
    return n


@pytest.fixture(scope="module")
def harness_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("depth_host"))
    n = write_records(os.path.join(d, "records.bin"))
    return d, n


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_build_equals_the_restatement_bit_for_bit(harness_dir, sanitize):
    d, n = harness_dir
    exe = toolchain.host_program(d, "depth_host_harness.cpp", sanitize)
    r = subprocess.run([exe, os.path.join(d, "records.bin")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout[-3000:] + r.stderr[-3000:]
    assert n == len(C.labellings()) + len(C.speckles()) + len(C.holes()) + 2 * len(SC.NOISY)
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == n and "DIFFERENT" not in r.stdout and "MISSING" not in r.stdout


# ---- (c) the ABI, the kernels' resources and the options -----------------------------------------------------------------------------------------
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
    assert (lib.im_depth_tile_w(), lib.im_depth_tile_h()) == (C.TILE_W, C.TILE_H)
    assert (D.MAX_PLANE_DIFF, D.MAX_HOLE, D.MAX_PLANES, D.MAX_SIDE) == (DO.MAX_DIFF, DO.MAX_HOLE, DO.MAX_PLANES, DO.MAX_SIDE) == (4095, 4096, 4096, 16384)
    with open(os.path.join(toolchain.CSRC, "depth_pixel.h")) as f:
        text = f.read()
    assert "DEPTH_MAX_DIFF = 4095, DEPTH_MAX_HOLE = 4096, DEPTH_MAX_PLANES = 4096" in text and text.count("#pragma clang fp contract(off)") == 3
    assert "sqrt" not in text and "fma" not in text and "atomicAdd" not in text       # + - * / and rint; the one atomic of the header is atomicMin


def test_the_kernels_spill_nothing(tmp_path):
    """Eight kernels of 256 threads. The tile kernel holds the planes, the parents and the counts of 64 x 16 pixels in LDS (10 KiB); nothing else has LDS;
    the flatten and the decide launches stay within 64 VGPRs."""
    res = toolchain.kernel_resources(toolchain.device_listing("depth_clean.hip", str(tmp_path)))
    kernels = ("depth_tile_kernel", "depth_merge_kernel", "depth_flatten_kernel", "depth_size_kernel", "depth_drop_kernel", "depth_rim_init_kernel",
               "depth_rim_kernel", "depth_fill_kernel")
    assert len(res) == 8 and all(any(k in name for name in res) for k in kernels), sorted(res)
    for k, f in res.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (k, dict(f))
        print(k, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "lds", f["group_segment_fixed_size"])
        assert f["max_flat_workgroup_size"] == 256
        assert f["group_segment_fixed_size"] == (C.TILE_W * C.TILE_H * 10 if "depth_tile_kernel" in k else 0)
        if "depth_tile_kernel" not in k and "depth_merge_kernel" not in k:
            assert f["vgpr_count"] <= 64, (k, f["vgpr_count"])
        assert f["vgpr_count"] <= 128


def cameras():
    K = np.array([[1200.0, 0.0, 400.0], [0.0, 1200.0, 300.0], [0.0, 0.0, 1.0]])
    return [Camera(800, 600, K=K, R=np.eye(3), t=np.zeros(3)), Camera(800, 600, K=K, R=np.eye(3), t=np.array([-1.0, 0.02, 0.05]))]


REFUSALS = [
    ("a speckle that is no pair", dict(speckle=16), "speckle is None or"),
    ("a speckle of three", dict(speckle=(16, 1, 2)), "speckle is None or"),
    ("min_size 0", dict(speckle=(0, 1)), "min_size"),
    ("a fractional min_size", dict(speckle=(2.5, 1)), "min_size"),
    ("min_size 2^31", dict(speckle=(2 ** 31, 1)), "min_size"),
    ("a negative max_diff", dict(speckle=(16, -1)), "max_diff"),
    ("max_diff 4096", dict(speckle=(16, 4096)), "max_diff"),
    ("holes that are no pair", dict(holes="small"), "holes is None or"),
    ("max_hole 0", dict(holes=(0, 2)), "max_hole"),
    ("max_hole 4097", dict(holes=(4097, 2)), "max_hole"),
    ("holes with max_diff 4096", dict(holes=(64, 4096)), "max_diff"),
    ("holes on a schedule of one plane", dict(holes=(64, 2), depth_range=(30.0, 30.0)), "w_step"),
]


@pytest.mark.parametrize("what,change,text", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("regularisation", [None, "sgm"])
def test_python_layer_refuses_before_any_device_work(what, change, text, regularisation, monkeypatch):
    from icepy4d_amd import engine
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    monkeypatch.setattr(D, "default_engine", lambda e: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    args = dict(images=[np.zeros((600, 800), np.uint8), np.zeros((600, 800), np.uint8)], cameras=cameras(), depth_range=(20.0, 60.0),
                regularisation=regularisation)
    args.update(change)
    with pytest.raises(ValueError, match=text):
        D.build_dense_cloud(**args)
    args.pop("regularisation")
    with pytest.raises(ValueError, match=text):
        D.build_depth_maps(**args)


def test_the_lower_functions_refuse_before_any_device_work(monkeypatch):
    import torch
    monkeypatch.setattr(D, "default_engine", lambda e: (_ for _ in ()).throw(AssertionError("an engine was asked for")))
    plane = torch.zeros((20, 30), dtype=torch.int16)
    for bad in (plane.to(torch.int32), plane[0], np.zeros((20, 30), np.int16)):
        with pytest.raises(ValueError, match="int16"):
            D.depth_components(bad)
    for bad in (-1, 4096, 1.5):
        with pytest.raises(ValueError, match="max_diff"):
            D.depth_components(plane, max_diff=bad)
    m = D.DepthMap(plane, torch.zeros((20, 30), dtype=torch.float64), torch.zeros((20, 30)), None, None, np.eye(3), np.eye(3), np.zeros(3), (0.1, 0.01, 5))
    for bad in (dict(min_size=0), dict(min_size=2 ** 31), dict(min_size=1.5), dict(max_diff=-1), dict(max_diff=4096)):
        with pytest.raises(ValueError):
            D.remove_speckles(m, **bad)
    for bad in (dict(max_hole=0), dict(max_hole=4097), dict(max_diff=-1), dict(max_diff=4096)):
        with pytest.raises(ValueError):
            D.fill_holes(m, **bad)
    for schedule in ((0.1, 0.0, 1), (float("inf"), 0.01, 5), (0.1, float("nan"), 5), (0.1, 0.01, 0), (0.1, 0.01, 4097)):
        with pytest.raises(ValueError):
            D.fill_holes(m._replace(schedule=schedule))


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


def test_without_the_options_no_new_call_is_made(monkeypatch):
    """`speckle=None, holes=None` is today's path under either regularisation; the options add their calls per view behind the sweep,
    speckles first. The context's `call` is replaced, so no device is needed."""
    images = [np.zeros((60, 80), np.uint8), np.zeros((60, 80), np.uint8)]
    K = np.array([[120.0, 0.0, 40.0], [0.0, 120.0, 30.0], [0.0, 0.0, 1.0]])
    cams = [Camera(80, 60, K=K, R=np.eye(3), t=np.zeros(3)), Camera(80, 60, K=K, R=np.eye(3), t=np.array([-1.0, 0.0, 0.0]))]
    eng = FakeEngine()
    monkeypatch.setattr(D, "default_engine", lambda e: eng)
    sgm = ["im_dense_costs", "im_dense_sgm", "im_dense_sgm_choose"]
    for extra, sweep in ((dict(), ["im_dense_sweep"]), (dict(regularisation="sgm"), sgm)):
        eng.ctx.names.clear()
        D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng, speckle=None, holes=None, **extra)
        assert eng.ctx.names == sweep * 2 and not any(n.startswith("im_depth_") for n in eng.ctx.names)
        eng.ctx.names.clear()
        D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng, speckle=(16, 1), **extra)
        assert eng.ctx.names == (sweep + ["im_depth_components", "im_depth_drop_small"]) * 2
        eng.ctx.names.clear()
        D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng, holes=(64, 2), **extra)
        assert eng.ctx.names == (sweep + ["im_depth_components", "im_depth_fill_holes"]) * 2
        eng.ctx.names.clear()
        maps = D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng, speckle=(16, 1), holes=(64, 2), **extra)
        assert eng.ctx.names == (sweep + ["im_depth_components", "im_depth_drop_small", "im_depth_components", "im_depth_fill_holes"]) * 2
        assert maps[0].plane.shape == (60, 80) and maps[0].w.dtype == __import__("torch").float64
    eng.ctx.names.clear()
    D.build_depth_maps(images, cams, depth_range=(8.0, 12.0), engine=eng)
    assert eng.ctx.names == ["im_dense_sweep"] * 2


def test_the_input_map_is_not_modified(monkeypatch):
    import torch
    eng = FakeEngine()
    monkeypatch.setattr(D, "default_engine", lambda e: eng)
    plane = torch.zeros((20, 30), dtype=torch.int16)
    m = D.DepthMap(plane, torch.zeros((20, 30), dtype=torch.float64), torch.zeros((20, 30)), None, None, np.eye(3), np.eye(3), np.zeros(3), (0.1, 0.01, 5))
    out, count = D.remove_speckles(m, engine=eng, return_counts=True)
    assert out.plane.data_ptr() != m.plane.data_ptr() and out.w.data_ptr() != m.w.data_ptr() and out.score.data_ptr() != m.score.data_ptr()
    assert count.dtype == torch.int64 and out.schedule == m.schedule and isinstance(D.remove_speckles(m, engine=eng), D.DepthMap)
    out, count = D.fill_holes(m, engine=eng, return_counts=True)
    assert out.plane.data_ptr() != m.plane.data_ptr() and count.dtype == torch.int64 and isinstance(D.fill_holes(m, engine=eng), D.DepthMap)


def test_dense_series_hands_the_options_down(monkeypatch):
    calls = []
    monkeypatch.setattr(D, "build_dense_cloud", lambda images, cameras, **kw: calls.append(kw) or len(calls))
    D.dense_series([["a0", "a1"]], cameras(), speckle=(8, 0), holes=(32, 1))
    assert calls[0]["speckle"] == (8, 0) and calls[0]["holes"] == (32, 1)
    calls.clear()
    got = []
    monkeypatch.undo()
    monkeypatch.setattr(D, "build_depth_maps", lambda *a, **kw: got.append(kw) or (_ for _ in ()).throw(RuntimeError("far enough")))
    with pytest.raises(RuntimeError, match="far enough"):
        D.build_dense_cloud([np.zeros((60, 80), np.uint8)] * 2, cameras(), depth_range=(20.0, 60.0), speckle=(8, 0), holes=(32, 1))
    assert got[0]["speckle"] == (8, 0) and got[0]["holes"] == (32, 1)
    got.clear()
    with pytest.raises(RuntimeError, match="far enough"):
        D.build_dense_cloud([np.zeros((60, 80), np.uint8)] * 2, cameras(), depth_range=(20.0, 60.0))
    assert "speckle" not in got[0] and "holes" not in got[0]
