"""The host plumbing every geometry stage shares (csrc/carve.h, csrc/stage_scratch.h; `engine.to_device`), without a GPU: the grid and
alignment helpers against their integer formulas, a Carve's pieces aligned, ascending and disjoint, and the bytes each carving entry point
asks for against the formula its source spelled by hand before the layouts were written down once (restated below from that source): a
context's scratch buffers grow at the same inputs to the same sizes."""
import ctypes
import itertools
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import toolchain  # noqa: E402

SCAN_THREADS, BIN_GROUP = 256, 8


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    lib = toolchain.host_library(str(tmp_path_factory.mktemp("carve_host")), "carve_host_harness.cpp")
    P, I, L, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong
    lib.carve_blocks_of.argtypes, lib.carve_blocks_of.restype = [L, I], L
    lib.carve_up256.argtypes, lib.carve_up256.restype = [U], U
    lib.carve_layout.argtypes, lib.carve_layout.restype = [I, P, P, U, P], U
    lib.carve_at.argtypes, lib.carve_at.restype = [U, U], L
    for name, nargs in (("dsm_group_mean", 1), ("dsm_rasterize", 2), ("binned_stats", 2), ("tracked_points", 1), ("knn_self", 1)):
        f = getattr(lib, "carve_" + name)
        f.argtypes, f.restype = [L] * nargs, U
    return lib


def up256(b):
    return (b + 255) // 256 * 256


def blocks_of(n, per):
    return (n + per - 1) // per


def test_grid_and_alignment_helpers(host_lib):
    for n, per in itertools.product((0, 1, 255, 256, 257, 2 ** 31 - 2), (64, 256)):
        assert host_lib.carve_blocks_of(n, per) == (n + per - 1) // per, (n, per)
        assert host_lib.carve_up256(n) == (n + 255) // 256 * 256 and host_lib.carve_up256(n) % 256 == 0, n


def layout(lib, pieces, slack=0):
    counts = np.array([c for c, _ in pieces], np.uint64)
    elem = np.array([e for _, e in pieces], np.int32)
    offsets = np.empty(len(pieces), np.uint64)
    total = lib.carve_layout(len(pieces), counts.ctypes.data, elem.ctypes.data, slack, offsets.ctypes.data)
    return [int(o) for o in offsets], int(total)


def test_carved_pieces_are_aligned_ascending_and_disjoint(host_lib):
    pieces = list(itertools.product((0, 1, 255, 256, 257), (1, 4, 8)))
    rng = np.random.default_rng(0)
    orders = [pieces, pieces[::-1], sorted(pieces, key=lambda p: p[1])] + [[pieces[i] for i in rng.permutation(len(pieces))] for _ in range(3)]
    for order in orders:
        offsets, total = layout(host_lib, order)
        assert all(o % 256 == 0 for o in offsets)
        assert offsets == sorted(offsets) and offsets[0] == 0
        ends = [o + c * e for o, (c, e) in zip(offsets, order)]
        assert all(end <= nxt for end, nxt in zip(ends, offsets[1:] + [total])), (order, offsets)       # no piece reaches into the next
        assert total == sum(up256(c * e) for c, e in order)
        assert layout(host_lib, order, slack=256)[1] == total + 256
    assert host_lib.carve_at(1, 5) == 256 and host_lib.carve_at(65, 5) == 512       # at(base) = base + offset, in bytes


SIZES = (1, 255, 256, 257, 100003)


def test_entry_points_ask_for_the_bytes_they_always_did(host_lib):
    """Each formula is the `o_x = o_y + up256(...)` chain and the `+ 256` / `+ 512` of the entry point's earlier source, term by term."""
    ll, i4 = 8, 4
    for n in SIZES:
        nb = blocks_of(n, SCAN_THREADS)
        assert host_lib.carve_dsm_group_mean(n) == up256(nb * ll) + up256(n * ll) + 256, n
        assert host_lib.carve_tracked_points(n) == 2 * up256(n * ll) + up256(nb * ll) + 512, n
        assert host_lib.carve_knn_self(n) == 3 * up256(n * 8) + up256(n * i4), n
    for cells, T in itertools.product(SIZES, (0,) + SIZES):
        t1 = max(T, 1)
        assert host_lib.carve_dsm_rasterize(cells, T) == up256(cells * i4) + up256(t1 * ll) + up256(blocks_of(t1, SCAN_THREADS) * ll) + 256, (cells, T)
    for n, n_seg in itertools.product((0,) + SIZES, SIZES):
        want = (up256(n_seg * i4) + up256((n_seg + 1) * ll) + up256((n // BIN_GROUP + 1) * ll) + up256(blocks_of(n_seg, SCAN_THREADS) * ll) + 256)
        assert host_lib.carve_binned_stats(n, n_seg) == want, (n, n_seg)


def test_host_half_of_to_device_copies_read_only_input_without_a_warning():
    import torch
    from icepy4d_amd.engine import host_array
    ro = np.arange(12, dtype=np.float64).reshape(3, 4)
    ro.flags.writeable = False
    views = (ro, ro[:, ::2], np.broadcast_to(np.float32(3.0), (2, 5)), np.frombuffer(b"\x01\x02\x03\x04", np.uint8))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for a in views:
            h = host_array(a)
            assert h.flags.writeable and h.flags.c_contiguous and np.array_equal(h, a) and h.dtype == a.dtype
            assert np.array_equal(torch.from_numpy(h).numpy(), a)
        h = host_array(ro, np.float32)
        assert h.dtype == np.float32 and np.array_equal(torch.from_numpy(h).numpy(), ro.astype(np.float32))
    rw = np.zeros((2, 3), np.int32)
    assert host_array(rw) is rw                         # what is contiguous and writeable already is not copied
