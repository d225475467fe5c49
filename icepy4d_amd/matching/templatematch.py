"""Feature tracking by template matching (reference `src/icepy4d/matching/templatematch.py`): same names, signatures, validation
errors and outputs; the orientation maps and the correlations run on the device (`im_forient`, `im_template_match_oc`,
csrc/templatematch.hip). Every entry point takes an optional `engine=` (an `icepy4d_amd.engine.Engine`; default: the shared
engine of device 0). There is no CPU fallback: without a HIP device the calls raise.

`OC` correlates every point of a call in ONE launch instead of the reference's per-point FFT loop, and `match_many` goes further:
one A image against several B images (what `utils.track_targets.TrackTargets.track` uses for all epochs at once).
Numerics (tests/test_gpu_templatematch.py): the correlation is the direct fp32 sum of the reference's (S - T)^2 block instead of
complex64 FFTs, so peak / mean correlations agree to ~1e-7 T^2 and du / dv to ~1e-4 px; NaN patterns and pu / pv are identical.
A point whose template or search window holds a NaN or an infinity (a float image with masked pixels) gets NaN for du, dv, peakCorr
and meanAbsCorr, as the reference's FFT of such a window gives."""
from typing import List, Tuple

import numpy as np
import torch

from .._lib import ptr
from ..engine import default_engine, to_device


class MatchResult:
    def __init__(self, pu, pv, du, dv, peakCorr, meanAbsCorr, method):
        self.pu = pu
        self.pv = pv
        self.du = du
        self.dv = dv
        self.peakCorr = peakCorr
        self.meanAbsCorr = meanAbsCorr
        self.snr = peakCorr / meanAbsCorr
        self.method = method


def _image_dtype(img: np.ndarray) -> Tuple[np.ndarray, int]:
    """uint8 images go to the device as they are (dtype 0); every other real image as float32 (dtype 1). The reference computes
    `forient` of a float64 image in complex128 before its complex64 FFT buffers round it: here it is rounded to float32 first."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return np.ascontiguousarray(img), 0
    return np.ascontiguousarray(img, dtype=np.float32), 1


def _is_complex_map(x) -> bool:
    return bool(np.any(np.iscomplex(x)))   # `OC` applies forient only when A holds no complex value (`templatematch.py:204-206`)


def _device_maps(eng, images: List[np.ndarray], as_maps: bool):
    """[n][h][w] complex64 maps on the device of equally shaped images: orientation maps of real images through ONE im_forient
    launch, or (as_maps) the inputs themselves as complex64."""
    h, w = images[0].shape
    out = torch.empty((len(images), h, w, 2), dtype=torch.float32, device=eng.device)
    if as_maps:
        host = np.ascontiguousarray(np.stack([np.asarray(im, np.complex64) for im in images]))
        out.copy_(torch.from_numpy(host.view(np.float32).reshape(len(images), h, w, 2)))
        return out
    if any(_is_complex_map(im) for im in images):
        raise ValueError("forient of a complex image is not supported: pass orientation maps as A and B, or real images")
    conv = [_image_dtype(np.real(im)) for im in images]
    dtype = 0 if all(d == 0 for _, d in conv) else 1
    host = np.stack([c if dtype == 0 else c.astype(np.float32) for c, _ in conv])
    d_img = to_device(host, eng.device)
    eng.ctx.call("im_forient", ptr(d_img), dtype, len(images), h, w, ptr(out), eng.stream_ptr())
    return out


def match_many(A, Bs: List[np.ndarray], pu, pv, TemplateWidth: int = 128, SearchWidth: int = 128 + 16, Initialdu=0, Initialdv=0,
               engine=None):
    """`OC(A, B, pu, pv, ...)` for every B of `Bs` (equal shapes), all (point, B) pairs in one correlation launch. pu / pv are not
    modified. Returns a dict of arrays [len(Bs)][*pu.shape]: pu, pv, du, dv, peakCorr, meanAbsCorr."""
    T, S = int(TemplateWidth), int(SearchWidth)
    if not 1 <= T < S:
        raise ValueError(f"template width {T} must be at least 1 and smaller than search width {S}")
    A = np.asarray(A)
    Bs = [np.asarray(b) for b in Bs]
    if A.ndim != 2 or any(b.ndim != 2 for b in Bs) or not Bs:
        raise ValueError("Invalid input images. Provide grayscale images.")
    if any(b.shape != Bs[0].shape for b in Bs):
        raise ValueError("all B images of one call must have the same shape")
    pu = np.asarray(pu, dtype=np.float64)
    pv = np.broadcast_to(np.asarray(pv, dtype=np.float64), pu.shape)
    idu = np.zeros(pu.shape) + Initialdu
    idv = np.zeros(pu.shape) + Initialdv
    eng = default_engine(engine)
    as_maps = _is_complex_map(A)
    dA, dB = _device_maps(eng, [A], as_maps), _device_maps(eng, Bs, as_maps)
    # `B = np.conj(B)` when B holds a complex value (`:217-218`); an orientation map that is entirely real has Bi = 0, so the sign
    # of the imaginary product does not matter for it
    conj_b = 1 if not as_maps else int(any(_is_complex_map(b) for b in Bs))
    n_pts, n_b = pu.size, len(Bs)
    pts = np.stack([pu.ravel(), pv.ravel(), idu.ravel(), idv.ravel()], 1)
    d_pairs = to_device(np.tile(pts, (n_b, 1)), eng.device)
    d_bidx = to_device(np.repeat(np.arange(n_b, dtype=np.int32), n_pts), eng.device)
    n = n_pts * n_b
    d_out = torch.empty((6, max(n, 1)), dtype=torch.float64, device=eng.device)
    ha, wa = A.shape
    hb, wb = Bs[0].shape
    eng.ctx.call("im_template_match_oc", ptr(dA), ha, wa, ptr(dB), n_b, hb, wb, ptr(d_pairs), ptr(d_bidx), n, T, S, conj_b, ptr(d_out),
                 eng.stream_ptr())
    out = d_out.cpu().numpy()[:, :n].reshape((6, n_b) + pu.shape)
    return dict(zip(("pu", "pv", "du", "dv", "peakCorr", "meanAbsCorr"), out))


def OC(A: np.ndarray, B: np.ndarray, pu: np.ndarray, pv: np.ndarray, TemplateWidth: int = 128, SearchWidth: int = 128 + 16,
       Initialdu: float = 0, Initialdv: float = 0, engine=None) -> MatchResult:
    """Orientation correlation of every point of the meshgrid-style arrays pu / pv in image A against image B
    (`templatematch.py:160-329`). As in the reference, pu / pv are overwritten in place with the centres actually used and returned
    in the MatchResult; NaN entries are not tracked."""
    r = match_many(A, [B], pu, pv, TemplateWidth, SearchWidth, Initialdu, Initialdv, engine=engine)
    pu_used, pv_used = r["pu"][0], r["pv"][0]
    if isinstance(pu, np.ndarray) and pu.flags.writeable:
        np.copyto(pu, pu_used.reshape(pu.shape), casting="unsafe")
    else:
        pu = pu_used
    if isinstance(pv, np.ndarray) and pv.flags.writeable and pv.shape == pu_used.shape:
        np.copyto(pv, pv_used.reshape(pv.shape), casting="unsafe")
    else:
        pv = pv_used
    return MatchResult(pu, pv, r["du"][0], r["dv"][0], r["peakCorr"][0], r["meanAbsCorr"][0], method="OC")


def forient(img, engine=None) -> np.ndarray:
    """Orientation map of a real image (`templatematch.py:332-340`) computed on the device: complex64, the 3 x 3 complex gradient
    with zero padding divided by its modulus (a modulus of 0 is replaced by 1)."""
    img = np.asarray(img)
    if img.ndim != 2:
        raise ValueError("forient expects a 2-D image")
    eng = default_engine(engine)
    if not img.size:
        return np.zeros(img.shape, np.complex64)
    return np.ascontiguousarray(_device_maps(eng, [img], False)[0].cpu().numpy()).view(np.complex64)[..., 0]


class TemplateMatch:
    """
    TemplateMatch: Feature tracking by template matching (`templatematch.py:26-157`).

    Args:
        A (np.ndarray): image A as 2D numpy array
        B (np.ndarray): image B as 2D numpy array
        xy (np.ndarray): Pixel coordinates in image A that you would like to find in image B as 2D numpy array of shape n x 2
        method (str, optional): Correlation method. Defaults to "OC".
        template_width (int, optional): Pixel-size of the small templates being cut from image A. Defaults to 128.
        search_width (int, optional): Pixel-size of the search region within image B. Defaults to 128 + 16.
        initialdu (float or array, optional): initial guess of the displacement in x. Defaults to 0.
        initialdv (float or array, optional): initial guess of the displacement in y. Defaults to 0.
        single_points (bool, optional): track only the points of xy (the diagonal of the meshgrid), not the meshgrid of their
            coordinates. Defaults to False.
        engine (optional): the device engine; default: the shared engine of device 0.
    """

    available_methods = ["OC"]

    def __init__(self, A: np.ndarray, B: np.ndarray, xy: np.ndarray = None, method: str = "OC", template_width: int = 128,
                 search_width: int = 128 + 16, initialdu: float = 0, initialdv: float = 0, single_points: bool = False,
                 engine=None) -> None:
        if len(A.shape) != 2 or len(B.shape) != 2:
            raise ValueError("Invalid input images. Provide grayscale images.")

        if xy.shape[1] != 2:
            raise ValueError("Invalid xy shape. Provide 2D array of shape n x 2.")

        if method not in self.available_methods:
            raise ValueError(f"Invalid method. Available methods: {self.available_methods}")

        self.A = A
        self.B = B
        self.method = method
        self.template_width = template_width
        self.search_width = search_width
        self.initialdu = initialdu
        self.initialdv = initialdv
        self.engine = engine

        pu, pv = self.define_grid(pu=xy[:, 0], pv=xy[:, 1])
        if single_points:
            def set_non_diagonal_nan(a):
                out = np.full_like(a, np.nan)
                di = np.diag_indices(a.shape[0])
                out[di] = a[di]
                return out

            pu = set_non_diagonal_nan(pu)
            pv = set_non_diagonal_nan(pv)

        self.pu = pu
        self.pv = pv

    def define_grid(self, pu: np.ndarray = None, pv: np.ndarray = None, step_x: int = None, step_y: int = None,
                    mask: np.ndarray = None) -> Tuple[np.ndarray, np.ndarray]:
        """Meshgrid of pu / pv when both are given; otherwise a regular grid over A with steps step_x / step_y, optionally
        restricted by a boolean mask (`templatematch.py:101-134`)."""
        if pu is not None and pv is not None:
            return np.meshgrid(pu, pv)

        if step_x is None or step_y is None:
            raise ValueError("Provide step_x and step_y for automatic grid generation.")

        x_range = np.arange(self.search_width / 2, self.A.shape[1] - self.search_width / 2 + self.template_width / 2, step_x)
        y_range = np.arange(self.search_width / 2, self.A.shape[0] - self.search_width / 2 + self.template_width / 2, step_y)

        if mask is not None:
            x_range, y_range = np.meshgrid(x_range, y_range)
            mask = np.logical_and(mask, np.logical_and(x_range >= 0, y_range >= 0))
            x_range = x_range[mask]
            y_range = y_range[mask]

        return np.meshgrid(x_range, y_range)

    def match(self) -> MatchResult:
        """One forient pass per image and one correlation launch for every point; returns the MatchResult."""
        if self.method == "OC":
            self.result = OC(self.A, self.B, self.pu, self.pv, self.template_width, self.search_width, self.initialdu,
                             self.initialdv, engine=self.engine)
        return self.result
