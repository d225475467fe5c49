"""The numpy restatement of the DEM of difference and of the polygon crop (include/icematch.h `im_dod_*`, `im_crop_polygon`):
what csrc/dod.hip and the host build of csrc/dod_cell.h are compared with, bit for bit. Every operation is an IEEE float64 operation in
the order the definition fixes: np.bincount with weights adds in input order, np.cumsum adds left to right.

    ground, ceil [n, 3] float64; vertDim d; X = (d + 1) % 3, Y = (d + 2) % 3; a point with a non-finite coordinate is ignored
    min / max over the kept points of both clouds; w = 1 + floor((max_x - min_x) / s + 0.5), h likewise; no kept point: w = h = 0
    column i = floor((x - min_x) / s + 0.5), row j likewise, cell j w + i
    per cloud and cell: count, sum of the d-coordinate in ascending input index from +0.0, mean = sum / count
    H = mean_ceil - mean_ground where both counts > 0, NaN elsewhere; valid = H finite
    the three sums over cells: chunks of B consecutive cells in ascending index from +0.0, then the partials in ascending chunk index
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g17_dod.npz")
CHUNK = 1024                      # im_dod_chunk(); the tests compare it with the library's
MAX_CELLS = 2 ** 24               # im_dod_max_cells()
FIELDS = ("volume", "addedVolume", "removedVolume", "surface", "matchingPercent", "groundNonMatchingPercent", "ceilNonMatchingPercent",
          "averageNeighborsPerCell", "validCells", "cellCount", "gridWidth", "gridHeight", "minX", "minY", "step", "cellArea")
F = np.float64


def axes(d):
    return (d + 1) % 3, (d + 2) % 3


def kept(pts):
    pts = np.asarray(pts, F).reshape(-1, 3)
    return np.isfinite(pts).all(1)


def lowest(v):
    """min of finite values with -0.0 below +0.0; +inf of nothing"""
    v = np.asarray(v, F)
    if not v.size:
        return F(np.inf)
    m = v.min()
    if m == 0:
        m = F(-0.0) if np.signbit(v[v == 0]).any() else F(0.0)
    return F(m)


def highest(v):
    v = np.asarray(v, F)
    if not v.size:
        return F(-np.inf)
    m = v.max()
    if m == 0:
        m = F(0.0) if (~np.signbit(v[v == 0])).any() else F(-0.0)
    return F(m)


def bounds(pts, d):
    """(min_x, min_y, max_x, max_y) float64 [4] of the kept points, and the number of dropped points"""
    pts = np.asarray(pts, F).reshape(-1, 3)
    k = kept(pts)
    ax, ay = axes(d)
    x, y = pts[k, ax], pts[k, ay]
    return np.array([lowest(x), lowest(y), highest(x), highest(y)], F), int((~k).sum())


def cell_coord(v, mn, s):
    with np.errstate(all="ignore"):
        return np.floor((np.asarray(v, F) - F(mn)) / F(s) + F(0.5))


def grid(bg, bc, s):
    """(min_x, min_y, w, h) of the pair whose clouds have the bounds bg and bc"""
    mn = [lowest([bg[a], bc[a]]) for a in (0, 1)]
    mx = [highest([bg[a], bc[a]]) for a in (2, 3)]
    if not (mn[0] <= mx[0]):
        return F(0.0), F(0.0), 0, 0
    wd, hd = F(1.0) + cell_coord(mx[0], mn[0], s), F(1.0) + cell_coord(mx[1], mn[1], s)
    return mn[0], mn[1], wd, hd


def cells_of(pts, d, min_x, min_y, s, w, h):
    """cell j w + i of every point, -1 for a dropped one"""
    pts = np.asarray(pts, F).reshape(-1, 3)
    ax, ay = axes(d)
    k = kept(pts)
    out = np.full(len(pts), -1, np.int64)
    ti, tj = cell_coord(pts[k, ax], min_x, s), cell_coord(pts[k, ay], min_y, s)
    assert ((ti >= 0) & (ti < w) & (tj >= 0) & (tj < h)).all()          # every kept point is inside the grid
    out[k] = tj.astype(np.int64) * int(w) + ti.astype(np.int64)
    return out


def cell_means(pts, cell, d, n_cells):
    """(count int64, mean float64 with NaN where count == 0)"""
    pts = np.asarray(pts, F).reshape(-1, 3)
    sel = cell >= 0
    count = np.bincount(cell[sel], minlength=n_cells).astype(np.int64)
    with np.errstate(all="ignore"):
        total = np.bincount(cell[sel], weights=pts[sel, d], minlength=n_cells).astype(F)        # adds in input order, from 0.0
        mean = np.where(count > 0, total / count.astype(F), np.nan)
    return count, mean


def chunked_sum(values, select, chunk):
    """values[select] summed in chunks of `chunk` consecutive indices, each ascending from +0.0, then the partials ascending. A value that
    is not selected is replaced by +0.0: a running sum that starts at +0.0 is never -0.0, so adding +0.0 to it changes nothing."""
    n = len(values)
    if n == 0:
        return F(0.0)
    n_chunks = -(-n // chunk)
    m = np.zeros(n_chunks * chunk, F)
    m[:n][select] = values[select]
    with np.errstate(all="ignore"):
        parts = np.cumsum(m.reshape(n_chunks, chunk), axis=1)[:, -1]
        return F(np.cumsum(parts)[-1])


def neighbours(valid):
    """per cell the number of valid cells among its 8 in-grid neighbours"""
    h, w = valid.shape
    p = np.zeros((h + 2, w + 2), np.int64)
    p[1:-1, 1:-1] = valid
    out = np.zeros((h, w), np.int64)
    for dj in (0, 1, 2):
        for di in (0, 1, 2):
            if (dj, di) != (1, 1):
                out += p[dj:dj + h, di:di + w]
    return out


def report_of(Hflat, cg, cc, w, h, min_x, min_y, s, chunk):
    s = F(s)
    with np.errstate(all="ignore"):
        a = s * s
        valid = np.isfinite(Hflat)
        n_valid, filled = int(valid.sum()), int(((cg > 0) | (cc > 0)).sum())
        r = dict.fromkeys(FIELDS, F(0.0))
        r.update(cellCount=F(filled), gridWidth=F(w), gridHeight=F(h), minX=F(min_x), minY=F(min_y), step=s, cellArea=a)
        if n_valid == 0:
            return r
        nb = int(neighbours(valid.reshape(int(h), int(w)))[valid.reshape(int(h), int(w))].sum())
        r["volume"] = a * chunked_sum(Hflat, valid, chunk)
        r["addedVolume"] = a * chunked_sum(Hflat, valid & (Hflat > 0), chunk)
        r["removedVolume"] = a * (F(0.0) - chunked_sum(Hflat, valid & (Hflat < 0), chunk))      # nothing removed: +0.0
        r["surface"] = a * F(n_valid)
        r["matchingPercent"] = (F(100.0) * F(n_valid)) / F(filled)
        r["groundNonMatchingPercent"] = (F(100.0) * F(int(((cg > 0) & (cc == 0)).sum()))) / F(filled)
        r["ceilNonMatchingPercent"] = (F(100.0) * F(int(((cc > 0) & (cg == 0)).sum()))) / F(filled)
        r["averageNeighborsPerCell"] = F(nb) / F(n_valid)
        r["validCells"] = F(n_valid)
    return r


def dod(ground, ceil, d, s, chunk=CHUNK):
    """The whole definition for one pair: dict with H [h, w], report (dict of float64 by FIELDS), report_row [16], cells (ground, ceil),
    counts and means per cloud, dropped (ground, ceil). Raises ValueError where the call is refused."""
    if d not in (0, 1, 2) or not (np.isfinite(s) and s > 0):
        raise ValueError("refused")
    ground, ceil = np.asarray(ground, F).reshape(-1, 3), np.asarray(ceil, F).reshape(-1, 3)
    (bg, dg), (bc, dc) = bounds(ground, d), bounds(ceil, d)
    min_x, min_y, wd, hd = grid(bg, bc, s)
    if not wd * hd <= MAX_CELLS:
        raise ValueError("refused: more cells than the cap")
    w, h = int(wd), int(hd)
    n_cells = w * h
    kg, kc = cells_of(ground, d, min_x, min_y, s, w, h), cells_of(ceil, d, min_x, min_y, s, w, h)
    cg, mg = cell_means(ground, kg, d, n_cells)
    cc, mc = cell_means(ceil, kc, d, n_cells)
    with np.errstate(all="ignore"):
        H = np.where((cg > 0) & (cc > 0), mc - mg, np.nan)
    rep = report_of(H, cg, cc, w, h, min_x, min_y, s, chunk)
    return {"H": H.reshape(h, w), "report": rep, "report_row": np.array([rep[k] for k in FIELDS], F), "cells": (kg, kc), "counts": (cg, cc),
            "means": (mg, mc), "dropped": (dg, dc), "grid": (min_x, min_y, w, h)}


def in_polygon(poly, x, y):
    """Even-odd rule: for every edge (x0, y0) -> (x1, y1), from the last vertex to the first and then in order, toggle if
    (y0 > y) != (y1 > y) and x < (x1 - x0) * (y - y0) / (y1 - y0) + x0. A non-finite coordinate is outside."""
    poly = np.asarray(poly, F).reshape(-1, 2)
    x, y = np.asarray(x, F), np.asarray(y, F)
    inside = np.zeros(x.shape, bool)
    prev = np.roll(poly, 1, axis=0)
    with np.errstate(all="ignore"):
        for (x0, y0), (x1, y1) in zip(prev, poly):
            cross = ((y0 > y) != (y1 > y)) & (x < (x1 - x0) * (y - y0) / (y1 - y0) + x0)
            inside ^= cross
    return inside & np.isfinite(x) & np.isfinite(y)
