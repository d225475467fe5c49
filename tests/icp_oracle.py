"""The restatement of csrc/icp_point.h and csrc/icp.hip in elementwise numpy ("Co-registration of two clouds (ICP) and rigid
transforms"): no `@`, no BLAS, no libm beyond sqrt, so its bits are the same on every machine and equal the device's and the host build's.

Every sum follows the order the kernels state: chunks of ICP_CHUNK source points, thread t of 256 adds points t, t + 256, ... ascending
from +0.0, the xor butterfly 1, 2, 4, 8, 16, 32 inside each wave of 64, the four waves as (w0 + w1) + (w2 + w3); across chunks the same.
A sum is never -0.0 (x + y is -0.0 only for two -0.0 and the sums start at +0.0), so a thread that adds nothing and a thread that adds
+0.0 hold the same bits: the restatement pads every chunk and the chunk list with rows of +0.0."""
import numpy as np

ICP_CHUNK, BLOCK, WAVE, TERMS, SUMS = 1024, 256, 64, 32, 30
I_B, I_RR, I_D2, I_COUNT = 21, 27, 28, 29
POINT_TO_POINT, POINT_TO_PLANE = 0, 1
OK, EMPTY, DEGENERATE = 0, 1, 2
PIVOT = 2.0 ** -40
REC_M, REC_FITNESS, REC_RMSE, REC_COUNT, REC_STATUS, REC_X, REC_PIVOT, REC_SUMS, RECORD = 0, 16, 17, 18, 19, 20, 26, 32, 64
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]
_QUIET = dict(invalid="ignore", over="ignore", divide="ignore")


def _f(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1, 3)


def n_chunks(n):
    return (n + ICP_CHUNK - 1) // ICP_CHUNK


def apply(M, pts, as_vectors=False):
    """p_a = ((M_a0*x + M_a1*y) + M_a2*z) [+ M_a3]"""
    M, p = np.asarray(M, np.float64).reshape(4, 4), _f(pts)
    out = np.empty_like(p)
    with np.errstate(**_QUIET):
        for a in range(3):
            v = ((M[a, 0] * p[:, 0]) + (M[a, 1] * p[:, 1])) + (M[a, 2] * p[:, 2])
            out[:, a] = v if as_vectors else v + M[a, 3]
    return out


def usable(p, normals, n_tgt, idx, method):
    ok = (idx >= 0) & (idx < n_tgt) & np.isfinite(p).all(1)
    if method == POINT_TO_PLANE:
        ok &= np.isfinite(normals[np.clip(idx, 0, max(n_tgt - 1, 0))]).all(1) if n_tgt else False
    return ok


def jacobian(pc, n):
    """[m, 6] = (p' x n, n), each cross component fl(fl(a*b) - fl(c*d))"""
    J = np.empty((len(pc), 6))
    J[:, 0] = (pc[:, 1] * n[:, 2]) - (pc[:, 2] * n[:, 1])
    J[:, 1] = (pc[:, 2] * n[:, 0]) - (pc[:, 0] * n[:, 2])
    J[:, 2] = (pc[:, 0] * n[:, 1]) - (pc[:, 1] * n[:, 0])
    J[:, 3:] = n
    return J


def rows(p, target, normals, idx, centre, method):
    """The rows of every source point: [(J [m, 6], r [m])], one entry for point to plane and three for point to point, with an unusable
    point's entries +0.0; and the mask of usable points."""
    p, tgt, idx = _f(p), _f(target), np.asarray(idx, np.int64)
    c = np.asarray(centre, np.float64).reshape(3)
    m, nt = len(p), len(tgt)
    nrm = _f(normals) if method == POINT_TO_PLANE else np.zeros((nt, 3))
    ok = usable(p, nrm, nt, idx, method)
    inside = (idx >= 0) & (idx < nt)
    safe = np.where(inside, idx, 0)
    q = np.where(inside[:, None], tgt[safe], 0.0) if m and nt else np.zeros((m, 3))
    n = np.where(inside[:, None], nrm[safe], 0.0) if m and nt else np.zeros((m, 3))
    out = []
    with np.errstate(**_QUIET):
        pc, e = p - c[None, :], p - q
        if method == POINT_TO_PLANE:
            r = ((e[:, 0] * n[:, 0]) + (e[:, 1] * n[:, 1])) + (e[:, 2] * n[:, 2])
            out.append((np.where(ok[:, None], jacobian(pc, n), 0.0), np.where(ok, r, 0.0)))
        else:
            for k in range(3):
                u = np.zeros((m, 3))
                u[:, k] = 1.0
                out.append((np.where(ok[:, None], jacobian(pc, u), 0.0), np.where(ok, e[:, k], 0.0)))
    return out, ok


def terms(row_list, ok, d2):
    """The passes a thread adds per point, in order: [m, 32] each; d2 and the count ride in the last one."""
    m = len(ok)
    passes = []
    with np.errstate(**_QUIET):
        for J, r in row_list:
            T = np.zeros((m, TERMS))
            for k, (a, b) in enumerate(UPPER):
                T[:, k] = J[:, a] * J[:, b]
            for a in range(6):
                T[:, I_B + a] = J[:, a] * r
            T[:, I_RR] = r * r
            passes.append(T)
    passes[-1][:, I_D2] = np.where(ok, np.asarray(d2, np.float64), 0.0)
    passes[-1][:, I_COUNT] = np.where(ok, 1.0, 0.0)
    return passes


def block_sum(S):
    """S [..., 256, 32], one row per thread -> [..., 32]: butterfly inside each wave, then (w0 + w1) + (w2 + w3)."""
    v = S.reshape(S.shape[:-2] + (BLOCK // WAVE, WAVE, TERMS))
    lane = np.arange(WAVE)
    with np.errstate(**_QUIET):
        for o in (1, 2, 4, 8, 16, 32):
            v = v + v[..., lane ^ o, :]
        w = v[..., 0, :]
        return (w[..., 0, :] + w[..., 1, :]) + (w[..., 2, :] + w[..., 3, :])


def strided_sum(passes, group):
    """[g, 32] block sums of groups of `group` consecutive rows: thread t adds rows t, t + 256, ... of its group, each row's passes in order."""
    m = len(passes[0])
    g = (m + group - 1) // group
    padded = []
    for T in passes:
        P = np.zeros((g * group, TERMS))
        P[:m] = T
        padded.append(P.reshape(g, group // BLOCK, BLOCK, TERMS))
    S = np.zeros((g, BLOCK, TERMS))
    with np.errstate(**_QUIET):
        for step in range(group // BLOCK):
            for P in padded:
                S = S + P[:, step]
    return block_sum(S)


def partials(p, target, normals, idx, d2, centre, method):
    """[n_chunks, 32]: what im_icp_accumulate writes."""
    row_list, ok = rows(p, target, normals, idx, centre, method)
    if len(ok) == 0:
        return np.zeros((0, TERMS))
    return strided_sum(terms(row_list, ok, d2), ICP_CHUNK)


def total(parts):
    """[32]: the partials summed as im_icp_finish does."""
    parts = np.asarray(parts, np.float64).reshape(-1, TERMS)
    if len(parts) == 0:
        return np.zeros(TERMS)
    steps = (len(parts) + BLOCK - 1) // BLOCK
    return strided_sum([parts], steps * BLOCK)[0]


def solve(S):
    """(x [6], pivots [6], every pivot passed) of A x = -b by LDL^T without pivoting, in icp_solve's order."""
    A = np.zeros((6, 6))
    for k, (a, b) in enumerate(UPPER):
        A[a, b] = A[b, a] = S[k]
    L, d, w, y, x = np.zeros((6, 6)), np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6)
    ok = True
    with np.errstate(**_QUIET):
        for j in range(6):
            for m in range(j):
                w[m] = L[j, m] * d[m]
            v = A[j, j]
            for m in range(j):
                v = v - L[j, m] * w[m]
            d[j] = v
            ok = ok and bool(v > np.float64(PIVOT) * A[j, j])
            for i in range(j + 1, 6):
                u = A[i, j]
                for m in range(j):
                    u = u - L[i, m] * w[m]
                L[i, j] = u / v
        for i in range(6):
            v = -S[I_B + i]
            for m in range(i):
                v = v - L[i, m] * y[m]
            y[i] = v
        for i in range(5, -1, -1):
            v = y[i] / d[i]
            for m in range(i + 1, 6):
                v = v - L[m, i] * x[m]
            x[i] = v
    return x, d, ok


def cayley(w):
    """R [3, 3] of the Cayley map of w."""
    two = np.float64(2.0)
    with np.errstate(**_QUIET):
        ax, ay, az = (np.float64(v) / two for v in w)
        aa = ((ax * ax) + (ay * ay)) + (az * az)
        s, u = np.float64(1.0) + aa, np.float64(1.0) - aa
        return np.array([[(u + two * (ax * ax)) / s, (two * (ax * ay) - two * az) / s, (two * (ax * az) + two * ay) / s],
                         [(two * (ax * ay) + two * az) / s, (u + two * (ay * ay)) / s, (two * (ay * az) - two * ax) / s],
                         [(two * (ax * az) - two * ay) / s, (two * (ay * az) + two * ax) / s, (u + two * (az * az)) / s]])


def update(x, centre, M):
    """M_new = [R | fl(fl(t + c) - R c)] o M."""
    R, c, M = cayley(x[:3]), np.asarray(centre, np.float64).reshape(3), np.asarray(M, np.float64).reshape(4, 4)
    out = np.zeros((4, 4))
    with np.errstate(**_QUIET):
        for a in range(3):
            Rc = ((R[a, 0] * c[0]) + (R[a, 1] * c[1])) + (R[a, 2] * c[2])
            T = (x[3 + a] + c[a]) - Rc
            for j in range(4):
                v = ((R[a, 0] * M[0, j]) + (R[a, 1] * M[1, j])) + (R[a, 2] * M[2, j])
                out[a, j] = v + T if j == 3 else v
    out[3] = (0.0, 0.0, 0.0, 1.0)
    return out


def finish(S, M, centre, n, do_solve=True):
    """The record [64] of im_icp_finish."""
    S, M = np.asarray(S, np.float64).reshape(TERMS), np.asarray(M, np.float64).reshape(4, 4)
    count = S[I_COUNT]
    x, d, status = np.zeros(6), np.zeros(6), OK
    if do_solve:
        x, d, ok = solve(S)
        status = OK if ok and count >= 6.0 else DEGENERATE
    if not count > 0.0:
        status = EMPTY
    rec = np.zeros(RECORD)
    rec[REC_M:REC_M + 16] = (update(x, centre, M) if do_solve and status == OK else M).reshape(16)
    with np.errstate(**_QUIET):
        rec[REC_FITNESS] = count / np.float64(n) if n > 0 else 0.0
        rec[REC_RMSE] = np.sqrt(S[I_D2] / count) if count > 0.0 else 0.0
    rec[REC_COUNT], rec[REC_STATUS] = count, status
    rec[REC_X:REC_X + 6], rec[REC_PIVOT:REC_PIVOT + 6] = x, d
    rec[REC_SUMS:REC_SUMS + SUMS] = S[:SUMS]
    return rec


def nearest(queries, points, radius2):
    """(idx int32 [m], d2 float64 [m]) of im_knn_cross with k = 1: d = q - p, d2 = ((dx*dx) + (dy*dy)) + (dz*dz), the lower index among
    equals, -1 / +inf beyond radius2, without a target or for a non-finite query."""
    q, p = _f(queries), _f(points)
    m = len(q)
    idx, d2o = np.full(m, -1, np.int32), np.full(m, np.inf)
    fin = np.isfinite(q).all(1)
    if len(p) == 0:
        return idx, d2o
    for b in range(0, m, 512):
        sel = np.nonzero(fin[b:b + 512])[0] + b
        if len(sel) == 0:
            continue
        with np.errstate(**_QUIET):
            d = q[sel, None, :] - p[None, :, :]
            d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
        j = np.argmin(d2, axis=1)
        best = d2[np.arange(len(sel)), j]
        keep = ~(best > radius2)
        idx[sel[keep]], d2o[sel[keep]] = j[keep], best[keep]
    return idx, d2o


def default_centre(target):
    t = _f(target)
    if len(t) == 0:
        return np.zeros(3)
    return (t.min(0) + t.max(0)) / np.float64(2.0)


def evaluate(source, target, normals, d_max, M, centre, method, do_solve, search=nearest):
    """One pass: (record [64], idx, d2) at the transform M."""
    p = apply(M, source)
    idx, d2 = search(p, target, np.float64(d_max) * np.float64(d_max))
    parts = partials(p, target, normals, idx, d2, centre, method)
    return finish(total(parts), M, centre, len(p), do_solve), idx, d2


def icp(source, target, normals, d_max, init=None, method=POINT_TO_PLANE, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
        centre=None, search=nearest):
    """The loop of `registration_icp`: (transformation, records [passes, 64], correspondences (idx, d2) of every pass, converged)."""
    M = np.eye(4) if init is None else np.asarray(init, np.float64).reshape(4, 4).copy()
    centre = default_centre(target) if centre is None else np.asarray(centre, np.float64).reshape(3)
    records, corr, converged = [], [], False
    for it in range(max_iteration + 1):
        rec, idx, d2 = evaluate(source, target, normals, d_max, M, centre, method, it < max_iteration, search)
        records.append(rec)
        corr.append((idx, d2))
        if it > 0 and abs(rec[REC_FITNESS] - records[-2][REC_FITNESS]) < relative_fitness and abs(rec[REC_RMSE] - records[-2][REC_RMSE]) < relative_rmse:
            converged = True
            break
        if rec[REC_STATUS] != OK or it == max_iteration:
            break
        M = rec[REC_M:REC_M + 16].reshape(4, 4).copy()
    return M, np.array(records), corr, converged
