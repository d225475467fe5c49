"""The template-matching cases at which the kernels of csrc/templatematch.hip (arithmetic: csrc/tm_pair.h) can go wrong, shared by
tests/test_templatematch_host_cpu.py (a host build of the header) and tests/test_gpu_templatematch_edges.py (the kernels through the C
ABI): one case per code path, each at the smallest (T, S) that reaches it, every claim asserted with the restated plan (check_claims).

A case is a dict: name, T, S, conj_b, A [ha, wa] complex64 (the orientation map of A), B [n_b, hb, wb] complex64, pairs [n, 4] float64
(u, v, initdu, initdv), bidx [n] int32, and, where the maps come from images, img_a [ha, wa] and img_b [n_b, hb, wb] (uint8 or float32)
with A = forient(img_a). Every array is read-only. Expected results (tm_oracle.corr, tm_oracle.oc) are computed once per case and
shared. Image sizes are S plus a few pixels; the two large shapes carry one pair."""
import functools

import numpy as np

import tm_oracle as O

C64 = np.complex64


def _ro(a, dtype=None):
    a = np.array(a, dtype=dtype, order="C")
    a.setflags(write=False)
    return a


def _images(rng, shape, dtype):
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.random(shape, dtype=np.float32)


def _maps(imgs):
    return np.stack([O.forient(i) for i in imgs])


def _case(name, T, S, A, B, pairs, bidx=None, conj_b=1, img_a=None, img_b=None):
    pairs = np.atleast_2d(np.asarray(pairs, np.float64))
    bidx = np.zeros(len(pairs), np.int32) if bidx is None else bidx
    c = dict(name=name, T=T, S=S, conj_b=conj_b, A=_ro(A, C64), B=_ro(B, C64), pairs=_ro(pairs, np.float64), bidx=_ro(bidx, np.int32))
    if img_a is not None:
        c.update(img_a=_ro(img_a), img_b=_ro(img_b))
    return c


def _centre(S, pad):
    """A point whose search window lies `pad` pixels inside an image of S + 2 pad + 1 pixels."""
    return float(S // 2 + pad + (S & 1))


def _path_case(name, T, S, n_pairs, seed, dtype=np.uint8, conj_b=1, n_b=1, size_b=None):
    """Random images of S + 7 pixels (B may differ), n_pairs points around the centre with integer initial displacements."""
    rng = np.random.default_rng(seed)
    ha, wa = S + 7, S + 8
    hb, wb = size_b or (ha, wa)
    img_a, img_b = _images(rng, (ha, wa), dtype), _images(rng, (n_b, hb, wb), dtype)
    c = _centre(S, 3)
    pairs = [[c + rng.integers(-2, 3), c + rng.integers(-2, 3), rng.integers(-1, 2), rng.integers(-1, 2)] for _ in range(n_pairs)]
    pairs[0] = [c, c, 0, 0]
    bidx = np.arange(n_pairs, dtype=np.int32) % n_b
    return _case(name, T, S, O.forient(img_a), _maps(img_b), pairs, bidx, conj_b, img_a, img_b)


# name -> (T, S, pairs, what the plan must show)
PATHS = {
    "R1_ks5_idle_lanes":      (5, 6, 4, lambda p: p["R"] == 1 and p["ks"] == 5 and p["reduce"] > p["stage"] and p["gy"] * p["gx"] * p["ks"] < p["threads"]),
    "R3_stage_above_reduce":  (9, 12, 3, lambda p: 1 < p["R"] < 16 and p["gy"] == p["R"] and p["ks"] == 9 and p["stage"] > p["reduce"] > 0),
    "gy16":                   (20, 36, 2, lambda p: p["gy"] == 16 and p["R"] == 16 and p["ks"] == 16),
    "gy32_above_R_ks3":       (3, 23, 3, lambda p: p["gy"] == 32 > p["R"] and p["ks"] == 3 and p["threads"] == 192),
    "ny3_ks5":                (10, 43, 2, lambda p: p["ny"] == 3 and p["gy"] == 16 and p["ks"] == 5 and p["reduce"] > p["stage"]),
    "nx2_T1":                 (1, 146, 2, lambda p: p["nx"] == 2 and p["ks"] == 1 and O.plan(1, 145)["nx"] == 1),
    "ks1_row_chunks_9_8":     (17, 130, 2, lambda p: p["ks"] == 1 and p["kt"] == 9 and p["ny"] == 4 and p["threads"] == 256),
    "ks3_row_chunks_21_19":   (40, 120, 2, lambda p: p["ks"] == 3 and p["kt"] == 21 and p["ny"] == 5 and p["kx"] == 48),
    "ks_halved":              (56, 57, 2, lambda p: p["ks_first"] == 56 and p["ks"] == 28 and O.plan(55, 56)["ks"] == 55),
    "T_not_multiple_of_ks":   (57, 58, 2, lambda p: p["ks"] == 28 and 57 % p["ks"] and p["kt"] == 28 and O.plan(56, 57)["kt"] * 2 == 56),
    "kx_reduced":             (113, 226, 1, lambda p: p["kx_first"] == 128 and p["kx"] == 112 and p["ks"] == 1 and O.plan(112, 224)["kx"] == 112 == O.plan(112, 224)["kx_first"]),
    "column_chunks":          (129, 130, 1, lambda p: p["kx"] == 128 < 129 and O.plan(128, 129)["kx"] == 128),
    "default_32_128":         (32, 128, 1, lambda p: p["ks"] == 1 and p["ny"] == 3 and p["threads"] == 192),
    "default_128_144":        (128, 144, 1, lambda p: p["ks"] == 16 and p["kt"] == 16 and p["kx"] == 128),
}


def check_claims():
    """Every path case is what its name says, by the restated plan; returns the plans."""
    plans = {}
    for name, (T, S, _, claim) in PATHS.items():
        p = O.plan(T, S)
        assert claim(p), (name, p)
        plans[name] = p
    chunks = lambda T, p: (-(-T // p["kt"]), T - (-(-T // p["kt"]) - 1) * p["kt"])     # noqa: E731  (row chunks, rows of the last)
    assert chunks(17, plans["ks1_row_chunks_9_8"]) == (2, 8) and chunks(40, plans["ks3_row_chunks_21_19"]) == (2, 19)
    assert chunks(57, plans["T_not_multiple_of_ks"]) == (3, 1) and chunks(129, plans["column_chunks"])[0] > 1
    assert all(T % 16 for T in (5, 9, 3, 10, 17, 57, 113, 129))
    return plans


def _window_pairs(T, S, ha, wa, hb, wb):
    """The points of the window rule: non-finite coordinates, half-integer ties, and sweeps in half pixels across every edge of A and B."""
    nan, inf = np.nan, np.inf
    mid = 40.0
    pairs = [[nan, mid, 0, 0], [mid, nan, 0, 0], [mid, mid, nan, 0], [mid, mid, 0, nan], [inf, mid, 0, 0], [-inf, mid, 0, 0], [1e300, mid, 0, 0],
             [mid, 1e300, 0, 0], [mid, mid, 1e300, 0], [100.5, 101.5, 0, 0], [101.5, 100.5, 0, 0], [100.5, 100.5, 0.5, 1.5], [mid, mid, 0, 0]]
    half = np.arange(-3.0, 3.5, 0.5)
    for d in half:
        # the search window across the near and the far edges of B; the template stays inside A, at `mid` where B is the larger
        pairs += [[S / 2 + d, mid, 0, 0], [mid, S / 2 + d, 0, 0], [mid, mid, wb - S / 2 + d - mid, 0], [mid, mid, 0, hb - S / 2 + d - mid]]
        # the template across the edges of A, the search window pushed inside B by the initial displacement
        push = (S - T) / 2 + 4
        pairs += [[T / 2 + d, mid, push, 0], [mid, T / 2 + d, 0, push], [wa - T / 2 + d, mid, -push - 8, 0], [mid, ha - T / 2 + d, 0, -push - 8]]
    bidx = [0] * len(pairs)
    pairs += [[mid, mid, 0, 0]] * 4
    bidx += [-1, 2, 1, -2147483648]                          # n_b = 2: -1 and n_b are out of range
    return np.array(pairs, np.float64), np.array(bidx, np.int32)


def _window_case(T, S, seed):
    rng = np.random.default_rng(seed)
    ha, wa, hb, wb = 118, 121, 125, 119
    img_a, img_b = _images(rng, (ha, wa), np.uint8), _images(rng, (2, hb, wb), np.uint8)
    pairs, bidx = _window_pairs(T, S, ha, wa, hb, wb)
    return _case(f"windows_T{T}_S{S}", T, S, O.forient(img_a), _maps(img_b), pairs, bidx, 1, img_a, img_b)


def _unit_maps(rng, shape):
    ph = rng.uniform(0, 2 * np.pi, shape)
    return (np.cos(ph) + 1j * np.sin(ph)).astype(C64)


def _peak_case():
    """T = 8, S = 20 (R = 12): nine B maps, each A rolled so that the template is found at (mi, mj) of C: on each border of C, and at
    distance 1 ... 5 from it (window sides 3, 5, 7, 9, 9)."""
    rng = np.random.default_rng(77)
    T, S, R = 8, 20, 12
    A = _unit_maps(rng, (S + 9, S + 9))
    spots = [(0, 6), (11, 6), (6, 0), (6, 11), (1, 6), (2, 6), (3, 6), (4, 6), (5, 6)]
    B = np.stack([np.roll(A, (mi - R // 2, mj - R // 2), (0, 1)) for mi, mj in spots])
    c = _centre(S, 4)
    return _case("peaks_border_and_distance_1_to_5", T, S, A, B, [[c, c, 0, 0]] * len(spots), np.arange(len(spots), dtype=np.int32)), spots


def _tie_case(name, T, S, period, seed):
    """B periodic with `period` = (py, px) (0: not periodic along that axis): C repeats exactly, every element summing the same terms in
    the same order."""
    rng = np.random.default_rng(seed)
    hb = S + 9
    A = _unit_maps(rng, (hb, hb))
    cell = _unit_maps(rng, (period[0] or hb, period[1] or hb))
    B = np.tile(cell, (-(-hb // cell.shape[0]), -(-hb // cell.shape[1])))[:hb, :hb]
    c = _centre(S, 4)
    return _case(name, T, S, A, B[None], [[c, c, 0, 0], [c + 1, c - 1, 0, 0]])


def _flat_case():
    img = np.full((40, 41), 200, np.uint8)
    return _case("flat_image", 6, 18, O.forient(img), _maps(img[None]), [[20, 20, 0, 0], [19, 21, 1, 0]], None, 1, img, img[None])


def _nonfinite_cases():
    """T = 5, S = 12: one pair at (10, 10), template rows / columns 7 ... 11 of A, search window rows / columns 4 ... 15 of B."""
    rng = np.random.default_rng(5)
    T, S = 5, 12
    A0, B0 = _unit_maps(rng, (21, 22)), _unit_maps(rng, (1, 21, 22))
    pairs = [[10, 10, 0, 0]]
    out = [_case("nonfinite_none", T, S, A0, B0, pairs)]

    def put(name, a_at=None, b_at=None, value=np.nan):
        A, B = A0.copy(), B0.copy()
        if a_at:
            A[a_at] = value
        if b_at:
            B[0][b_at] = value
        out.append(_case(name, T, S, A, B, pairs))

    put("nonfinite_nan_in_last_column_of_the_window", b_at=(9, 15))       # column S - 1 of the window: only the zero padding multiplies it
    put("nonfinite_nan_in_last_row_of_the_window", b_at=(15, 6))
    put("nonfinite_nan_in_the_template", a_at=(10, 11))
    put("nonfinite_inf_in_B", b_at=(4, 4), value=np.inf)
    put("nonfinite_imaginary_minus_inf_in_B", b_at=(8, 9), value=complex(0.5, -np.inf))
    A, B = A0.copy(), B0.copy()
    A[6, 9] = A[12, 9] = A[9, 6] = A[9, 12] = np.nan
    B[0][3, 8] = B[0][16, 8] = B[0][8, 3] = B[0][8, 16] = np.nan
    out.append(_case("nonfinite_nan_just_outside_both_windows", T, S, A, B, pairs))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """{name: case}"""
    out = []
    for k, (name, (T, S, n, _)) in enumerate(PATHS.items()):
        out.append(_path_case(name, T, S, n, 100 + k))
    out.append(_path_case("conj_b_0_gy16", 20, 36, 2, 201, conj_b=0))
    out.append(_path_case("conj_b_0_R3", 9, 12, 2, 202, conj_b=0))
    out.append(_path_case("float32_images", 10, 43, 2, 203, dtype=np.float32))
    out.append(_path_case("B_larger_than_A_three_B_images", 9, 30, 4, 204, n_b=3, size_b=(41, 45)))
    out.append(_path_case("B_narrower_than_A", 7, 24, 3, 205, n_b=2, size_b=(33, 29)))
    for k, (T, S) in enumerate([(4, 8), (5, 8), (4, 9), (5, 9)]):
        out.append(_window_case(T, S, 300 + k))
    out.append(_peak_case()[0])
    out.append(_tie_case("ties_same_lane", 6, 22, (4, 0), 401))           # R = 16: maxima 4 rows = 64 elements apart
    out.append(_tie_case("ties_other_lanes", 6, 18, (0, 4), 402))         # R = 12: maxima 4 elements apart
    out.append(_tie_case("ties_both", 6, 22, (4, 4), 403))
    out.append(_flat_case())
    out.extend(_nonfinite_cases())
    assert len({c["name"] for c in out}) == len(out)
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def expected_corr(name):
    """{pair: C} of the valid pairs (read-only arrays)."""
    out = O.corr(cases()[name])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_oc(name):
    out = O.oc(cases()[name], expected_corr(name))
    out.setflags(write=False)
    return out


def peak_spots():
    return _peak_case()[1]
