"""Numpy restatement of orientation-correlation template matching (`src/icepy4d/matching/templatematch.py`: `forient`, `OC`),
written from its description for random device cases; checked against the reference's own outputs in
tests/golden/g11_templatematch.npz (tests/test_templatematch_cpu.py).

The reference correlates through complex64 FFTs; this oracle forms the same (S - T) x (S - T) block of the correlation directly
in float64 and rounds it to float32, which is what the FFT's result approximates. Everything after C (argmax, mean |C|, edge test,
centroid) runs the same numpy operations on float32 arrays as the reference, so it inherits numpy's rounding."""
import numpy as np


def forient_parts(img):
    """(re, im) of the 3 x 3 complex gradient with zero padding: re = img[y+1, x+1] - img[y-1, x-1], im = img[y+1, x-1] - img[y-1, x+1],
    in float32 (exact for uint8 input)."""
    a = np.asarray(img)
    p = np.zeros((a.shape[0] + 2, a.shape[1] + 2), np.float32)
    p[1:-1, 1:-1] = a
    re = p[2:, 2:] - p[:-2, :-2]
    im = p[2:, :-2] - p[:-2, 2:]
    return re, im


def forient(img):
    """complex64 map: the gradient divided by its modulus (a modulus of 0 is replaced by 1)."""
    re, im = forient_parts(img)
    m = np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2)
    m[m == 0] = 1.0
    return ((re / m).astype(np.float32) + 1j * (im / m).astype(np.float32)).astype(np.complex64)


def corr_block(Aw, Bw, conj_b=True):
    """C[i, j] = sum Re(Aw[ty, tx] * B'[i + ty, j + tx]) with B' = conj(Bw) when conj_b (float64)."""
    T, S = Aw.shape[0], Bw.shape[0]
    R = S - T
    win = np.lib.stride_tricks.sliding_window_view(Bw, (T, T))[:R, :R]
    ar, ai = Aw.real.astype(np.float64), Aw.imag.astype(np.float64)
    br, bi = win.real.astype(np.float64), win.imag.astype(np.float64)
    s = 1.0 if conj_b else -1.0
    return np.einsum("ijyx,yx->ij", br, ar) + s * np.einsum("ijyx,yx->ij", bi, ai)


def oc(A, B, pu, pv, T=128, S=128 + 16, initdu=0, initdv=0, return_c=False):
    """Orientation correlation of every point of pu / pv (any shape; NaN = not tracked). A and B are images (forient applied) or
    complex maps. pu / pv are NOT modified. Returns dict pu, pv, du, dv, peakCorr, meanAbsCorr (and C per point when return_c)."""
    if not np.iscomplexobj(A) or not np.any(np.iscomplex(A)):
        A, B = forient(A), forient(B)
    conj_b = bool(np.any(np.iscomplex(B)))
    pu = np.array(pu, dtype=np.float64, copy=True)
    pv = np.array(pv, dtype=np.float64, copy=True)
    idu = np.zeros(pu.shape) + initdu
    idv = np.zeros(pu.shape) + initdv
    du, dv, pk, mc = (np.full(pu.shape, np.nan) for _ in range(4))
    Cs = {}
    R = S - T
    wkeep = R / 2
    cu = np.arange(-wkeep, wkeep + 1)
    for ii, u in np.ndenumerate(pu):
        if np.isnan(u):
            continue
        v = pv[ii]
        ac = np.round(np.array([u, v])) - (T / 2 % 1)
        bc = np.round(np.array([u, v]) + np.array([idu[ii], idv[ii]])) - (S / 2 % 1)
        pu[ii], pv[ii] = ac
        off = bc - ac
        if np.isnan(u + v):
            continue
        with np.errstate(invalid="ignore"):
            if not np.all(np.isfinite(bc)):
                continue
            b0, b1 = np.trunc(bc[1] - S / 2), np.trunc(bc[1] + S / 2)
            c0, c1 = np.trunc(bc[0] - S / 2), np.trunc(bc[0] + S / 2)
            a0, a1 = np.trunc(ac[1] - T / 2), np.trunc(ac[1] + T / 2)
            d0, d1 = np.trunc(ac[0] - T / 2), np.trunc(ac[0] + T / 2)
        if min(a0, b0, c0, d0) < 0 or b1 >= B.shape[0] or a1 >= A.shape[0] or c1 >= B.shape[1] or d1 >= A.shape[1]:
            continue
        Aw = A[int(a0):int(a0) + T, int(d0):int(d0) + T]
        Bw = B[int(b0):int(b0) + S, int(c0):int(c0) + S]
        C = corr_block(Aw, Bw, conj_b).astype(np.float32)
        if return_c:
            Cs[ii] = C
        mi, mj = np.unravel_index(np.argmax(C), C.shape)
        mc[ii] = np.mean(abs(C))
        edge = min(mi, mj, R - 1 - mi, R - 1 - mj)
        if edge == 0:
            continue
        ww = min(edge, 4)
        c = C[mi - ww:mi + ww + 1, mj - ww:mj + ww + 1]
        uu, vv = np.meshgrid(cu[mj - ww:mj + ww + 1], cu[mi - ww:mi + ww + 1])
        c = c - np.mean(abs(c.ravel()))
        c[c < 0] = 0
        c = c / np.sum(c)
        du[ii] = np.sum(uu * c) + off[0]
        dv[ii] = np.sum(vv * c) + off[1]
        pk[ii] = C[mi, mj]
    out = dict(pu=pu, pv=pv, du=du, dv=dv, peakCorr=pk, meanAbsCorr=mc)
    if return_c:
        out["C"] = Cs
    return out


def derived_inputs(g):
    """Inputs of tests/golden/g11_templatematch.npz that are rebuilt from its stored uint8 images instead of being stored (every
    operation is exactly rounded, so the arrays are the ones tools/gen_golden_templatematch.py passed to the reference)."""
    fa = np.sqrt(g["img1"][:200, :300].astype(np.float32) / np.float32(255))
    fb = g["img2"][:200, :300].astype(np.float32) / np.float32(255)
    return {"float_a": fa, "float_b": fb, "forient_f32_in": fa[40:88, 60:124].copy(),
            "synth_b": np.roll(g["synth_a"], (21, -23), axis=(0, 1))}


def load_g11(path):
    """tests/golden/g11_templatematch.npz with its derived inputs added."""
    g = dict(np.load(path))
    g.update(derived_inputs(g))
    return g


def top_two_margin(C):
    """Distance between the largest and the second-largest value of C (the argmax decision margin)."""
    f = np.sort(np.asarray(C, np.float64).ravel())
    return float(f[-1] - f[-2]) if f.size > 1 else np.inf
