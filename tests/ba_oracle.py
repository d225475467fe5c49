"""The restatement of csrc/ba_point.h and csrc/ba.hip in elementwise numpy ("Two-view bundle adjustment with control points"):
no `@`, no BLAS, no libm beyond sqrt, every expression with the header's own grouping, so its bits are the same on every machine and equal
the device's and the host build's. Arrays run over the points of ONE epoch; every sum takes a chunk's points in ascending index from +0.0 and
then the chunks in ascending order."""
import numpy as np

BA_CHUNK, BA_TILE, CAM, DIM, CAMSTATE, EPOCH = 256, 32, 14, 28, 24, 48
N_UPPER, I_B, I_COST, I_COUNT, SUMS, TERMS = 406, 406, 434, 435, 436, 448
F_J, F_R, F_Y, F_Z, F_L, F_D, F_COST, F_OK, FAC = 0, 56, 60, 144, 147, 150, 153, 154, 155
KEEP = FAC - F_Y
RUNNING, OK, MAX_ITER, STALLED, EMPTY, DEGENERATE = -1, 0, 1, 2, 3, 4
STATUS_NAMES = {RUNNING: "RUNNING", OK: "OK", MAX_ITER: "MAX_ITER", STALLED: "STALLED", EMPTY: "EMPTY", DEGENERATE: "DEGENERATE"}
MASK_DEFAULT = 0x7F | (0x7F << 14)
MASK_ALL = (1 << 28) - 1
PIVOT = 2.0 ** -40
ST_LAMBDA, ST_PARITY, ST_DONE, ST_STATUS, ST_ITER, STATE = 0, 1, 2, 3, 4, 8
REC_COST0, REC_COST1, REC_LAMBDA, REC_ACCEPTED, REC_COUNT, REC_STATUS, REC_X, REC_PIVOT, REC_ITER, RECORD = 0, 1, 2, 3, 4, 5, 6, 34, 62, 64
SOL_REC, SOL = 448, 512
UPPER = [(a, b) for a in range(DIM) for b in range(a, DIM)]
_QUIET = dict(invalid="ignore", over="ignore", divide="ignore", under="ignore")


def n_chunks(n):
    return (n + BA_CHUNK - 1) // BA_CHUNK


def initial_state(lambda0=1e-3):
    st = np.zeros(STATE)
    st[ST_LAMBDA], st[ST_STATUS] = lambda0, RUNNING
    return st


def options(lambda_min=1e-12, lambda_max=1e8, ftol=1e-12, max_iter=30, ctol=0.0):
    return np.array([lambda_min, lambda_max, ftol, float(max_iter), ctol])


def camera_state(R, C, K, dist=None):
    """[24]: R row-major, C, fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6"""
    out = np.zeros(CAMSTATE)
    out[:9] = np.asarray(R, np.float64).reshape(9)
    out[9:12] = np.asarray(C, np.float64).reshape(3)
    K = np.asarray(K, np.float64)
    out[12:16] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if dist is not None:
        d = np.asarray(dist, np.float64).reshape(-1)
        out[16:16 + min(len(d), 8)] = d[:8]
    return out


def cayley(w):
    """icp_cayley"""
    ax, ay, az = w[0] / 2.0, w[1] / 2.0, w[2] / 2.0
    aa = ((ax * ax) + (ay * ay)) + (az * az)
    s, u = 1.0 + aa, 1.0 - aa
    return np.array([(u + 2.0 * (ax * ax)) / s, (2.0 * (ax * ay) - 2.0 * az) / s, (2.0 * (ax * az) + 2.0 * ay) / s,
                     (2.0 * (ax * ay) + 2.0 * az) / s, (u + 2.0 * (ay * ay)) / s, (2.0 * (ay * az) - 2.0 * ax) / s,
                     (2.0 * (ax * az) - 2.0 * ay) / s, (2.0 * (ay * az) + 2.0 * ax) / s, (u + 2.0 * (az * az)) / s])


def project(cam, X):
    """ba_project over points X [n, 3]: a dict of the intermediates"""
    with np.errstate(**_QUIET):
        d0, d1, d2 = X[:, 0] - cam[9], X[:, 1] - cam[10], X[:, 2] - cam[11]
        Xc = [((cam[3 * a] * d0) + (cam[3 * a + 1] * d1)) + (cam[3 * a + 2] * d2) for a in range(3)]
        fx, fy, cx, cy = cam[12:16]
        k1, k2, p1, p2, k3, k4, k5, k6 = cam[16:24]
        x, y = Xc[0] / Xc[2], Xc[1] / Xc[2]
        r2 = (x * x) + (y * y)
        num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
        radial = num / den
        dx = ((2.0 * p1) * x) * y + p2 * (r2 + (2.0 * x) * x)
        dy = p1 * (r2 + (2.0 * y) * y) + ((2.0 * p2) * x) * y
        xd = x * radial + dx
        yd = y * radial + dy
        return dict(Xc=Xc, x=x, y=y, r2=r2, num=num, den=den, radial=radial, xd=xd, yd=yd, u=fx * xd + cx, v=fy * yd + cy)


def rows(cam, p, uo, vo, i_s):
    """ba_rows: J [n, 2, 14], Jp [n, 2, 3], r [n, 2]"""
    n = len(uo)
    with np.errstate(**_QUIET):
        fx, fy = cam[12], cam[13]
        k1, k2, p1, p2, k3, k4, k5, k6 = cam[16:24]
        x, y, r2, den, num, radial, Xc = p["x"], p["y"], p["r2"], p["den"], p["num"], p["radial"], p["Xc"]
        dnum = ((3.0 * k3) * r2 + 2.0 * k2) * r2 + k1
        dden = ((3.0 * k6) * r2 + 2.0 * k5) * r2 + k4
        drad = ((dnum * den) - (num * dden)) / (den * den)
        tx, ty = (2.0 * x) * drad, (2.0 * y) * drad
        xx = ((radial + x * tx) + (2.0 * p1) * y) + (6.0 * p2) * x
        xy = (x * ty + (2.0 * p1) * x) + (2.0 * p2) * y
        yx = (y * tx + (2.0 * p1) * x) + (2.0 * p2) * y
        yy = ((radial + y * ty) + (6.0 * p1) * y) + (2.0 * p2) * x
        G = [[fx * xx, fx * xy], [fy * yx, fy * yy]]
        iz = 1.0 / Xc[2]
        e1, e2, e3 = r2 / den, (r2 * r2) / den, ((r2 * r2) * r2) / den
        xyp = (2.0 * x) * y
        s, c, dd = [fx, fy], [x, y], [p["xd"], p["yd"]]
        t1, t2 = [xyp, r2 + (2.0 * y) * y], [r2 + (2.0 * x) * x, xyp]
        J, Jp = np.zeros((n, 2, CAM)), np.zeros((n, 2, 3))
        for i in range(2):
            B = [(G[i][0] * iz) * i_s, (G[i][1] * iz) * i_s, (-(((G[i][0] * x) + (G[i][1] * y)) * iz)) * i_s]
            for k in range(3):
                Jp[:, i, k] = ((B[0] * cam[k]) + (B[1] * cam[3 + k])) + (B[2] * cam[6 + k])
                J[:, i, 3 + k] = -Jp[:, i, k]
            J[:, i, 0] = (B[2] * Xc[1]) - (B[1] * Xc[2])
            J[:, i, 1] = (B[0] * Xc[2]) - (B[2] * Xc[0])
            J[:, i, 2] = (B[1] * Xc[0]) - (B[0] * Xc[1])
            J[:, i, 6] = dd[i] * i_s
            J[:, i, 7] = i_s if i == 0 else 0.0
            J[:, i, 8] = i_s if i == 1 else 0.0
            J[:, i, 9] = ((s[i] * c[i]) * e1) * i_s
            J[:, i, 10] = ((s[i] * c[i]) * e2) * i_s
            J[:, i, 11] = (s[i] * t1[i]) * i_s
            J[:, i, 12] = (s[i] * t2[i]) * i_s
            J[:, i, 13] = ((s[i] * c[i]) * e3) * i_s
        r = np.stack([(p["u"] - uo) * i_s, (p["v"] - vo) * i_s], 1)
    return J, Jp, r


def usable(cams, X, obs, sigma, prior):
    """ba_usable: ok [n], projections, seen [2][n], q [n, 3]"""
    n = len(X)
    with np.errstate(**_QUIET):
        ok = np.isfinite(X).all(1) & (sigma > 0.0) & np.isfinite(sigma)
        n_obs = np.zeros(n, np.int64)
        pr, seen = [], []
        for c in range(2):
            uo, vo = obs[:, 2 * c], obs[:, 2 * c + 1]
            s = ~np.isnan(uo) & ~np.isnan(vo)
            p = project(cams[CAMSTATE * c:CAMSTATE * (c + 1)], X)
            fine = np.isfinite(uo) & np.isfinite(vo) & (p["Xc"][2] > 0.0) & np.isfinite(p["u"]) & np.isfinite(p["v"])
            ok = ok & (~s | fine)
            n_obs += s
            pr.append(p)
            seen.append(s)
        q, full = np.zeros((n, 3)), np.ones(n, bool)
        for k in range(3):
            has = prior[:, 3 + k] > 0.0
            q[:, k] = np.where(has, (X[:, k] - prior[:, k]) / np.where(has, prior[:, 3 + k], 1.0), 0.0)
            ok = ok & np.isfinite(q[:, k])
            full &= has
        return ok & ((n_obs == 2) | ((n_obs == 1) & full)), pr, seen, q


def half_squares(r, q):
    return 0.5 * (((((r[:, 0] * r[:, 0]) + (r[:, 1] * r[:, 1])) + (r[:, 2] * r[:, 2])) + (r[:, 3] * r[:, 3])) +
                  (((q[:, 0] * q[:, 0]) + (q[:, 1] * q[:, 1])) + (q[:, 2] * q[:, 2])))


def _forward3(L, sd, w0, w1, w2):
    t0 = w0
    t1 = w1 - L[0] * t0
    t2 = (w2 - L[1] * t0) - L[2] * t1
    return [t0 / sd[0], t1 / sd[1], t2 / sd[2]]


def factors(cams, X, obs, sigma, prior, lam):
    """ba_point_factors: [n, 155]"""
    cams, X, obs, sigma, prior = (np.asarray(v, np.float64) for v in (cams, X, obs, sigma, prior))
    n = len(X)
    f = np.zeros((n, FAC))
    if n == 0:
        return f
    ok, pr, seen, q = usable(cams, X, obs, sigma, prior)
    with np.errstate(**_QUIET):
        i_s = 1.0 / sigma
        Jp, r = np.zeros((n, 4, 3)), np.zeros((n, 4))
        J = np.zeros((n, 4, CAM))
        for c in range(2):
            j, jp, rr = rows(cams[CAMSTATE * c:CAMSTATE * (c + 1)], pr[c], obs[:, 2 * c], obs[:, 2 * c + 1], i_s)
            use = ok & seen[c]
            r[:, 2 * c:2 * c + 2] = np.where(use[:, None], rr, 0.0)
            Jp[:, 2 * c:2 * c + 2] = np.where(use[:, None, None], jp, 0.0)
            J[:, 2 * c:2 * c + 2] = np.where(use[:, None, None], j, 0.0)
        V, g = [], []
        q = np.where(ok[:, None], q, 0.0)
        for a in range(3):
            has = ok & (prior[:, 3 + a] > 0.0)
            ip = np.where(has, 1.0 / np.where(has, prior[:, 3 + a], 1.0), 0.0)
            g.append(((((Jp[:, 0, a] * r[:, 0]) + (Jp[:, 1, a] * r[:, 1])) + (Jp[:, 2, a] * r[:, 2])) + (Jp[:, 3, a] * r[:, 3])) + q[:, a] * ip)
            for b in range(a, 3):
                v = (((Jp[:, 0, a] * Jp[:, 0, b]) + (Jp[:, 1, a] * Jp[:, 1, b])) + (Jp[:, 2, a] * Jp[:, 2, b])) + (Jp[:, 3, a] * Jp[:, 3, b])
                if b == a:
                    v = v + ip * ip
                    v = v + lam * v
                V.append(v)
        D, L = [None] * 3, [None] * 3
        D[0] = V[0]
        L[0] = V[1] / D[0]
        L[1] = V[2] / D[0]
        w10 = L[0] * D[0]
        D[1] = V[3] - L[0] * w10
        L[2] = (V[4] - L[1] * w10) / D[1]
        D[2] = (V[5] - L[1] * (L[1] * D[0])) - L[2] * (L[2] * D[1])
        sd = [np.sqrt(D[k]) for k in range(3)]
        f[:, F_J:F_R] = J.reshape(n, 56)
        f[:, F_R:F_Y] = r
        for a in range(DIM):
            i0 = 2 * (a // CAM)
            ja, jb = J[:, i0, a % CAM], J[:, i0 + 1, a % CAM]
            y = _forward3(L, sd, (ja * Jp[:, i0, 0]) + (jb * Jp[:, i0 + 1, 0]), (ja * Jp[:, i0, 1]) + (jb * Jp[:, i0 + 1, 1]),
                          (ja * Jp[:, i0, 2]) + (jb * Jp[:, i0 + 1, 2]))
            for k in range(3):
                f[:, F_Y + 3 * a + k] = np.where(ok, y[k], 0.0)
        z = _forward3(L, sd, g[0], g[1], g[2])
        for k in range(3):
            f[:, F_Z + k] = np.where(ok, z[k], 0.0)
            f[:, F_L + k] = np.where(ok, L[k], 0.0)
            f[:, F_D + k] = np.where(ok, D[k], 0.0)
        f[:, F_COST] = np.where(ok, half_squares(r, q), 0.0)
        f[:, F_OK] = np.where(ok, 1.0, 0.0)
    return f


def terms(f):
    """ba_term for every sum: [n, 448]"""
    n = len(f)
    T = np.zeros((n, TERMS))
    with np.errstate(**_QUIET):
        Y = f[:, F_Y:F_Z].reshape(n, DIM, 3)
        J = f[:, F_J:F_R].reshape(n, 4, CAM)
        z, r = f[:, F_Z:F_Z + 3], f[:, F_R:F_R + 4]
        for e, (a, b) in enumerate(UPPER):
            yy = ((Y[:, a, 0] * Y[:, b, 0]) + (Y[:, a, 1] * Y[:, b, 1])) + (Y[:, a, 2] * Y[:, b, 2])
            if a // CAM == b // CAM:
                c = a // CAM
                jj = (J[:, 2 * c, a % CAM] * J[:, 2 * c, b % CAM]) + (J[:, 2 * c + 1, a % CAM] * J[:, 2 * c + 1, b % CAM])
            else:
                jj = 0.0
            T[:, e] = jj - yy
        for a in range(DIM):
            c = a // CAM
            yz = ((Y[:, a, 0] * z[:, 0]) + (Y[:, a, 1] * z[:, 1])) + (Y[:, a, 2] * z[:, 2])
            jr = (J[:, 2 * c, a % CAM] * r[:, 2 * c]) + (J[:, 2 * c + 1, a % CAM] * r[:, 2 * c + 1])
            T[:, I_B + a] = jr - yz
        T[:, I_COST] = f[:, F_COST]
        T[:, I_COUNT] = f[:, F_OK]
    return T


def _ascending(T, group):
    """[g, k] sums of groups of `group` consecutive rows of T [m, k], each from +0.0 in ascending order"""
    m, k = T.shape
    g = (m + group - 1) // group
    P = np.zeros((g * group, k))
    P[:m] = T
    P = P.reshape(g, group, k)
    S = np.zeros((g, k))
    with np.errstate(**_QUIET):
        for i in range(group):
            S = S + P[:, i]
    return S


def partials(f):
    return _ascending(terms(f), BA_CHUNK)


def total(parts):
    S = np.zeros(parts.shape[1])
    with np.errstate(**_QUIET):
        for ch in range(len(parts)):
            S = S + parts[ch]
    return S


def centre_cost(cams, cprior):
    s = 0.0
    with np.errstate(**_QUIET):
        for c in range(2):
            for k in range(3):
                sc = cprior[6 * c + 3 + k]
                rp = (cams[CAMSTATE * c + 9 + k] - cprior[6 * c + k]) / sc if sc > 0.0 else 0.0
                s = s + 0.5 * (rp * rp)
    return np.float64(s)


def reduced(S, cams, cprior, lam, mask):
    A, b = np.zeros((DIM, DIM)), np.array(S[I_B:I_B + DIM], np.float64)
    for m, (a, c) in enumerate(UPPER):
        A[a, c] = A[c, a] = S[m]
    with np.errstate(**_QUIET):
        for c in range(2):
            for k in range(3):
                sc = cprior[6 * c + 3 + k]
                if sc > 0.0:
                    p = CAM * c + 3 + k
                    ip = 1.0 / sc
                    rp = (cams[CAMSTATE * c + 9 + k] - cprior[6 * c + k]) / sc
                    A[p, p] = A[p, p] + ip * ip
                    b[p] = b[p] + rp * ip
        for p in range(DIM):
            A[p, p] = A[p, p] + lam * A[p, p]
    for p in range(DIM):
        if not (mask >> p) & 1:
            A[p, :] = 0.0
            A[:, p] = 0.0
            A[p, p] = 1.0
            b[p] = 0.0
    return A, b


def solve(A, b):
    """ba_solve: x, d, ok"""
    n = DIM
    L, d, y, x = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n)
    ok = True
    with np.errstate(**_QUIET):
        for j in range(n):
            w = [L[j, m] * d[m] for m in range(j)]
            v = A[j, j]
            for m in range(j):
                v = v - L[j, m] * w[m]
            d[j] = v
            ok = ok and bool(v > PIVOT * A[j, j])
            for i in range(j + 1, n):
                u = A[j, i]
                for m in range(j):
                    u = u - L[i, m] * w[m]
                L[i, j] = u / v
        for i in range(n):
            v = -b[i]
            for m in range(i):
                v = v - L[i, m] * y[m]
            y[i] = v
        for i in range(n - 1, -1, -1):
            v = y[i] / d[i]
            for m in range(i + 1, n):
                v = v - L[m, i] * x[m]
            x[i] = v
    return x, d, ok


def step_camera(cam, x):
    out = np.array(cam, np.float64)
    Q = cayley(x[:3])
    for a in range(3):
        for j in range(3):
            out[3 * a + j] = ((Q[3 * a] * cam[j]) + (Q[3 * a + 1] * cam[3 + j])) + (Q[3 * a + 2] * cam[6 + j])
    for k in range(3):
        out[9 + k] = cam[9 + k] + x[3 + k]
    out[12], out[13], out[14], out[15] = cam[12] + x[6], cam[13] + x[6], cam[14] + x[7], cam[15] + x[8]
    out[16], out[17], out[18], out[19], out[20] = cam[16] + x[9], cam[17] + x[10], cam[18] + x[11], cam[19] + x[12], cam[20] + x[13]
    return out


def solve_epoch(S, cams, cprior, lam, mask):
    """ba_solve_epoch: the draft of the record [64] and the candidate cameras [48]"""
    A, b = reduced(S, cams, cprior, lam, mask)
    x, d, ok = solve(A, b)
    count = S[I_COUNT]
    step = ok and count > 0.0
    rec = np.zeros(RECORD)
    with np.errstate(**_QUIET):
        rec[REC_COST0] = S[I_COST] + centre_cost(cams, cprior)
    rec[REC_LAMBDA], rec[REC_ACCEPTED], rec[REC_COUNT] = lam, 1.0 if ok else 0.0, count
    rec[REC_X:REC_X + DIM] = x if step else 0.0
    rec[REC_PIVOT:REC_PIVOT + DIM] = d
    cand = np.array(cams, np.float64)
    if step:
        with np.errstate(**_QUIET):
            for c in range(2):
                cand[CAMSTATE * c:CAMSTATE * (c + 1)] = step_camera(cams[CAMSTATE * c:CAMSTATE * (c + 1)], rec[REC_X + CAM * c:REC_X + CAM * (c + 1)])
    return rec, cand


def point_step(f, x, X):
    """ba_point_step: [n, 3]"""
    n = len(X)
    with np.errstate(**_QUIET):
        q = [f[:, F_Z + k].copy() for k in range(3)]
        for a in range(DIM):
            for k in range(3):
                q[k] = q[k] + f[:, F_Y + 3 * a + k] * x[a]
        s = [q[k] / np.sqrt(f[:, F_D + k]) for k in range(3)]
        e2 = s[2]
        e1 = s[1] - f[:, F_L + 2] * e2
        e0 = (s[0] - f[:, F_L] * e1) - f[:, F_L + 1] * e2
        ok = f[:, F_OK] != 0.0
        out = np.array(X, np.float64).reshape(n, 3)
        for k, e in enumerate((e0, e1, e2)):
            out[:, k] = np.where(ok, X[:, k] + (-e), X[:, k])
    return out


def point_cost(cams, X, obs, sigma, prior, was_usable):
    """ba_point_cost: [n]"""
    n = len(X)
    if n == 0:
        return np.zeros(0)
    ok, pr, seen, q = usable(cams, X, obs, sigma, prior)
    with np.errstate(**_QUIET):
        i_s = 1.0 / sigma
        r = np.zeros((n, 4))
        for c in range(2):
            r[:, 2 * c] = np.where(seen[c], (pr[c]["u"] - obs[:, 2 * c]) * i_s, 0.0)
            r[:, 2 * c + 1] = np.where(seen[c], (pr[c]["v"] - obs[:, 2 * c + 1]) * i_s, 0.0)
        return np.where(was_usable, np.where(ok, half_squares(r, q), np.inf), 0.0)


def residuals(cams, X, obs):
    """ba_point_residuals: [n, 2, 3]"""
    n = len(X)
    res = np.full((n, 2, 3), np.nan)
    if n == 0:
        return res
    _, pr, seen, _ = usable(cams, X, obs, np.ones(n), np.zeros((n, 6)))
    with np.errstate(**_QUIET):
        for c in range(2):
            ex, ey = pr[c]["u"] - obs[:, 2 * c], pr[c]["v"] - obs[:, 2 * c + 1]
            fine = seen[c] & np.isfinite(ex) & np.isfinite(ey) & (pr[c]["Xc"][2] > 0.0)
            res[:, c, 0] = np.where(fine, ex, np.nan)
            res[:, c, 1] = np.where(fine, ey, np.nan)
            res[:, c, 2] = np.where(fine, np.sqrt((ex * ex) + (ey * ey)), np.nan)
    return res


def decide(draft, cost1, opts, st):
    """ba_decide: the record; st is updated in place"""
    rec = np.array(draft, np.float64)
    cost0, lam, it = draft[REC_COST0], draft[REC_LAMBDA], st[ST_ITER]
    status, accepted, nxt = RUNNING, False, lam
    with np.errstate(**_QUIET):
        if not draft[REC_COUNT] > 0.0:
            status = EMPTY
        elif draft[REC_ACCEPTED] == 0.0:
            status = DEGENERATE
        else:
            accepted = bool(cost1 < cost0)
            if accepted:
                nxt = lam / 10.0
                nxt = opts[0] if nxt < opts[0] else nxt
                if (cost0 - cost1) <= opts[2] * cost0 or cost1 <= opts[4]:
                    status = OK
            else:
                nxt = lam * 10.0
                if nxt > opts[1]:
                    status = STALLED
            if status == RUNNING and it + 1.0 >= opts[3]:
                status = MAX_ITER
    rec[REC_COST1] = cost0 if status in (EMPTY, DEGENERATE) else cost1
    rec[REC_ACCEPTED], rec[REC_STATUS], rec[REC_ITER] = 1.0 if accepted else 0.0, float(status), it
    st[ST_LAMBDA] = nxt
    if accepted:
        st[ST_PARITY] = 1.0 - st[ST_PARITY]
    if status != RUNNING:
        st[ST_DONE], st[ST_STATUS] = 1.0, float(status)
    st[ST_ITER] = it + 1.0
    return rec


def iteration(cams, X, obs, sigma, prior, cprior, mask, opts, st):
    """One iteration of one epoch: everything the four kernels write. st is updated in place."""
    lam = st[ST_LAMBDA]
    f = factors(cams, X, obs, sigma, prior, lam)
    parts = partials(f) if len(X) else np.zeros((0, TERMS))
    S = total(parts)
    draft, cand = solve_epoch(S, cams, cprior, lam, mask)
    out = point_step(f, draft[REC_X:REC_X + DIM], X) if len(X) else np.zeros((0, 3))
    cterms = point_cost(cand, out, obs, sigma, prior, f[:, F_OK] != 0.0)
    cparts = _ascending(cterms[:, None], BA_CHUNK)[:, 0] if len(X) else np.zeros(0)
    with np.errstate(**_QUIET):
        cost1 = total(cparts[:, None])[0] + centre_cost(cand, cprior)
    rec = decide(draft, cost1, opts, st)
    return dict(fac=f, parts=parts, sums=S, draft=draft, cand=cand, cand_pts=out, cparts=cparts, rec=rec, accepted=rec[REC_ACCEPTED] == 1.0)


def run(cams, X, obs, sigma, prior, cprior, mask=MASK_DEFAULT, opts=None, st=None):
    """The whole loop of one epoch: final cameras [48], points, state, history [iterations, 64]."""
    opts = options() if opts is None else np.asarray(opts, np.float64)
    st = initial_state() if st is None else np.array(st, np.float64)
    cams, X = np.array(cams, np.float64).reshape(EPOCH), np.array(X, np.float64).reshape(-1, 3)
    obs, sigma, prior = np.asarray(obs, np.float64).reshape(-1, 4), np.asarray(sigma, np.float64).reshape(-1), np.asarray(prior, np.float64).reshape(-1, 6)
    cprior = np.asarray(cprior, np.float64).reshape(12)
    history = []
    while st[ST_DONE] == 0.0:
        it = iteration(cams, X, obs, sigma, prior, cprior, mask, opts, st)
        history.append(it["rec"])
        if it["accepted"]:
            cams, X = it["cand"], it["cand_pts"]
    return cams, X, st, np.array(history).reshape(-1, RECORD)
