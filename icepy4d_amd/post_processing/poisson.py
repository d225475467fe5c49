"""Poisson surface reconstruction of an oriented cloud on the device (csrc/poisson.hip): what `MeshingPoisson.poisson_meshing` of the
reference's `post_processing/open3d_fun.py` asks Open3D for (`create_from_point_cloud_poisson` and its densities), with the signature of
the `reconstruct=` hook of `open3d_fun.MeshingPoisson` here.

It is not Open3D's adaptive-octree solver. It is a Poisson reconstruction on the dense grid of the finest octree level: the same bounding
cube (centre of the bounding box, side `scale` x largest extent) and the same finest cell size (side / 2^depth), the samples' weights and
normals splatted trilinearly, the divergence as right-hand side, a fixed number of multigrid V-cycles, the iso-value at the weighted mean
of the solution, marching tetrahedra over the Kuhn decomposition of every cell. The definition is DESIGN §4 and tests/poisson_oracle.py,
which the kernels equal bit for bit. Parity with an Open3D binary - its vertices, its triangle count, its density scale - is unpinned.

This module is plumbing: it validates on the host, lays the fields out in torch memory and orders the calls. No CPU fallback: without the
library or a device it raises as the other stages do."""
from collections import namedtuple

import numpy as np
import torch

from .._lib import ptr
from ..engine import default_engine, to_device

MIN_DEPTH, MAX_DEPTH = 2, 9
MAX_POINTS = 1 << 26
CHUNK = 1024
CYCLES = 8

PoissonField = namedtuple("PoissonField", "origin h depth chi iso W")
PoissonField.__doc__ = """The grid (origin [3] float64 numpy, cell size h, depth) and on it, as device tensors [M, M, M] float64 indexed [z, y, x]
with M = 2^depth + 1: the solution `chi` (lower inside for outward normals), the splatted sample weights `W`; `iso` the iso-value."""


def max_depth(engine=None) -> int:
    return int(default_engine(engine).ctx.lib.im_poisson_max_depth())


def _check_depth(depth) -> int:
    if int(depth) != depth or not MIN_DEPTH <= depth <= MAX_DEPTH:
        raise ValueError(f"depth must lie in [{MIN_DEPTH}, {MAX_DEPTH}] (got {depth})")
    return int(depth)


def _shape_of(a):
    return tuple(a.shape)


def _validate(points, normals, scale, cycles):
    """Everything that can be refused before a device is asked for."""
    for name, a in (("points", points), ("normals", normals)):
        if len(_shape_of(a)) != 2 or _shape_of(a)[1] != 3:
            raise ValueError(f"{name} must be [n, 3] (got {_shape_of(a)})")
    if _shape_of(points) != _shape_of(normals):
        raise ValueError(f"points and normals differ in length ({_shape_of(points)[0]} and {_shape_of(normals)[0]})")
    n = _shape_of(points)[0]
    if n == 0:
        raise ValueError("no points")
    if n > MAX_POINTS:
        raise ValueError(f"more than 2^26 points ({n}): down-sample the cloud first")
    if not scale >= 1:
        raise ValueError(f"scale must be >= 1 (got {scale})")
    if int(cycles) != cycles or cycles < 1:
        raise ValueError(f"cycles must be a positive integer (got {cycles})")
    for name, a in (("points", points), ("normals", normals)):
        if not bool((torch.isfinite(a) if isinstance(a, torch.Tensor) else np.isfinite(a)).all()):
            raise ValueError(f"non-finite {name}")
    if bool(((normals * normals).sum(1) == 0).any()):
        raise ValueError("a zero-length normal")


def _as_input(a):
    return a if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)


def grid_of(mn, mx, depth=8, width=0, scale=1.1):
    """(origin [3], h, depth) of the cube around the bounding box [mn, mx]: its centre, side scale x largest extent, 2^depth cells per
    axis; `width > 0` replaces depth by ceil(log2(side / width))."""
    mn, mx = np.asarray(mn, np.float64), np.asarray(mx, np.float64)
    extent = float((mx - mn).max())
    if not extent > 0:
        raise ValueError("a degenerate cloud: its largest extent is 0")
    centre = (mn + mx) * 0.5
    L = scale * extent
    if width > 0:
        depth = int(np.ceil(np.log2(L / width)))
    depth = _check_depth(depth)
    h = L / float(2 ** depth)
    return centre - L * 0.5, h, depth


def _ordered_sum(eng, a, b=None) -> float:
    """The sum of a (or of a * b) in the fixed order of `im_poisson_reduce`, applied until one item is left."""
    n = a.numel()
    while True:
        out = torch.empty((n + CHUNK - 1) // CHUNK, dtype=torch.float64, device=a.device)
        eng.ctx.call("im_poisson_reduce", ptr(a), ptr(b), n, ptr(out), eng.stream_ptr())
        if out.numel() == 1:
            return float(out.item())
        a, b, n = out, None, out.numel()


def _solve(eng, chi, rhs, tmp, h, depth, cycles, each_cycle=None):
    """`cycles` V-cycles on chi (zero at the start): 2 + 2 damped Jacobi sweeps per level, full weighting down, trilinear up, the 3^3 level
    directly. Level l has 2^l + 1 nodes per axis and spacing h 2^(depth - l)."""
    dev = chi.device
    call, st = eng.ctx.call, eng.stream_ptr()
    u, f, t = {depth: chi}, {depth: rhs}, {depth: tmp}
    for l in range(depth - 1, 0, -1):
        m = (2 ** l + 1) ** 3
        u[l], f[l] = torch.empty(m, dtype=torch.float64, device=dev), torch.empty(m, dtype=torch.float64, device=dev)
        t[l] = torch.empty(m, dtype=torch.float64, device=dev) if l > 1 else None

    def smooth(l, h2):
        call("im_poisson_jacobi", ptr(u[l]), ptr(f[l]), l, h2, ptr(t[l]), st)
        call("im_poisson_jacobi", ptr(t[l]), ptr(f[l]), l, h2, ptr(u[l]), st)

    def vcycle(l):
        hl = h * float(2 ** (depth - l))
        h2 = hl * hl
        if l == 1:
            call("im_poisson_coarse", ptr(f[1]), h2, ptr(u[1]), st)
            return
        smooth(l, h2)
        call("im_poisson_restrict", ptr(u[l]), ptr(f[l]), l, h2, ptr(t[l]), ptr(f[l - 1]), st)
        if l - 1 > 1:
            u[l - 1].zero_()
        vcycle(l - 1)
        call("im_poisson_prolong", ptr(u[l - 1]), l, ptr(u[l]), st)
        smooth(l, h2)

    for c in range(cycles):
        vcycle(depth)
        if each_cycle is not None:
            each_cycle(c, chi)


def poisson_field(points, normals, depth=8, width=0, scale=1.1, cycles=CYCLES, grid=None, engine=None, trace=None) -> PoissonField:
    """The indicator field of an oriented cloud on the device. `points`, `normals` [n, 3] (numpy arrays or torch tensors);
    `grid=(origin, h, depth)` fixes the cube (one grid for a series of epochs) where it is otherwise the cloud's own (`grid_of`); every
    point must lie in it. `trace`, a dict, receives copies of W, V [3, M, M, M], rhs and `chis`, chi after
    every cycle (for tests). Raises ValueError for what the definition refuses: differing lengths, no points, more than 2^26, non-finite
    values, a zero-length normal, a degenerate cloud, depth outside [2, 9], scale < 1."""
    points, normals = _as_input(points), _as_input(normals)
    _validate(points, normals, scale, cycles)
    if grid is not None:
        origin, h, depth = np.asarray(grid[0], np.float64).reshape(3), float(grid[1]), _check_depth(grid[2])
        if not (np.isfinite(origin).all() and np.isfinite(h) and h > 0):
            raise ValueError("the grid is not finite or its cell size is not positive")
    elif not isinstance(points, torch.Tensor):
        origin, h, depth = grid_of(points.min(0), points.max(0), depth, width, scale)
    eng = default_engine(engine)
    dev = eng.device
    d_pts, d_nrm = (a.to(device=dev, dtype=torch.float64).contiguous() if isinstance(a, torch.Tensor) else to_device(a, dev, np.float64) for a in (points, normals))
    if grid is None and isinstance(points, torch.Tensor):
        origin, h, depth = grid_of(d_pts.min(0).values.cpu().numpy(), d_pts.max(0).values.cpu().numpy(), depth, width, scale)
    if grid is not None:
        side = h * float(2 ** depth)
        lo, hi = d_pts.min(0).values.cpu().numpy(), d_pts.max(0).values.cpu().numpy()
        if (lo < origin).any() or (hi > origin + side).any():
            raise ValueError("points outside the given grid")
    n, M = d_pts.shape[0], 2 ** depth + 1
    N = M ** 3
    h_grid = np.array([origin[0], origin[1], origin[2], h], np.float64)
    call, st = eng.ctx.call, eng.stream_ptr()
    # four planes: W, V_x, V_y, V_z. Once the right-hand side exists V is dead: its first two planes become chi and the sweep buffer.
    fields = torch.empty((4, N), dtype=torch.float64, device=dev)
    call("im_poisson_splat", ptr(d_pts), ptr(d_nrm), n, h_grid.ctypes.data, depth, ptr(fields), st)
    rhs = torch.empty(N, dtype=torch.float64, device=dev)
    call("im_poisson_divergence", ptr(fields[1:]), depth, h, ptr(rhs), st)
    if trace is not None:
        trace.update(W=fields[0].clone().view(M, M, M), V=fields[1:].clone().view(3, M, M, M), rhs=rhs.clone().view(M, M, M), chis=[])
    W, chi, tmp = fields[0], fields[1], fields[2]
    chi.zero_()
    _solve(eng, chi, rhs, tmp, h, depth, int(cycles), None if trace is None else (lambda c, u: trace["chis"].append(u.clone().view(M, M, M))))
    iso = _ordered_sum(eng, W, chi) / _ordered_sum(eng, W)
    return PoissonField(np.array(origin, np.float64), h, depth, chi.view(M, M, M), iso, W.view(M, M, M))


def extract_surface(field: PoissonField, engine=None):
    """The iso-surface of a field by marching tetrahedra, as device tensors: vertices [V, 3] float64 in ascending edge key, triangles
    [T, 3] int32 ordered by (cell, tetrahedron, triangle) and wound towards higher chi, and per vertex the interpolated weight W."""
    eng = default_engine(engine)
    dev = eng.device
    depth = _check_depth(field.depth)
    N = (2 ** depth + 1) ** 3
    chi, W = field.chi.contiguous(), field.W.contiguous()
    if chi.numel() != N or W.numel() != N:
        raise ValueError("the field does not have (2^depth + 1)^3 nodes")
    call, st = eng.ctx.call, eng.stream_ptr()
    mask = torch.empty(N, dtype=torch.uint8, device=dev)
    base = torch.empty(N, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    call("im_poisson_census", ptr(chi), float(field.iso), depth, ptr(mask), ptr(base), ptr(counts), st)
    nv, nt = (int(c) for c in counts.cpu())
    if nv > MAX_POINTS or nt > MAX_POINTS:
        raise ValueError(f"the surface has more than 2^26 vertices or triangles ({nv}, {nt}): reconstruct at a lower depth")
    vertices = torch.empty((nv, 3), dtype=torch.float64, device=dev)
    weights = torch.empty(nv, dtype=torch.float64, device=dev)
    triangles = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    h_grid = np.array([field.origin[0], field.origin[1], field.origin[2], field.h], np.float64)
    call("im_poisson_extract", ptr(chi), ptr(W), float(field.iso), depth, h_grid.ctypes.data, ptr(mask), ptr(base), nv, nt, ptr(vertices), ptr(weights),
         ptr(triangles), st)
    return vertices, triangles, weights


def density_of(weights, depth) -> np.ndarray:
    """depth + log2(max(weight, 4^-depth)) / 2, on the host: the depth at which the local sampling would put one sample per cell of a
    surface, so values above `depth` occur where a cell holds several samples."""
    return depth + np.log2(np.maximum(np.asarray(weights, np.float64), 4.0 ** -depth)) / 2


def poisson_reconstruct(points, normals, depth=8, width=0, scale=1.1, linear_fit=False, cycles=CYCLES, engine=None):
    """(vertices float64 [V, 3], triangles int32 [T, 3], densities float64 [V]) as numpy arrays: the surface of `poisson_field` by
    `extract_surface`, closed for every input, and per vertex `density_of` its interpolated sample weight. The signature is that of the
    `reconstruct=` hook of `MeshingPoisson`. `linear_fit` is accepted and changes nothing: vertex positions interpolate linearly along
    their grid edge for both values."""
    f = poisson_field(points, normals, depth=depth, width=width, scale=scale, cycles=cycles, engine=engine)
    vertices, triangles, weights = extract_surface(f, engine=engine)
    return vertices.cpu().numpy(), triangles.cpu().numpy(), density_of(weights.cpu().numpy(), f.depth)
