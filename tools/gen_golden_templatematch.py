"""Writes tests/golden/g11_templatematch.npz: the reference's own template-matching outputs (`src/icepy4d/matching/templatematch.py`,
`src/icepy4d/utils/track_targets.py`) on crops of the four `assets/img/cam1` epochs and on a synthetic rolled pair.

    python tools/gen_golden_templatematch.py REFERENCE_ROOT

The reference module is loaded from its file, unchanged, with three un-vendored dependencies stubbed:
  - pyfftw: used only as an FFT. `pyfftw.empty_aligned` -> np.empty, `pyfftw.builders.fft2 / ifft2` -> callables around
    np.fft.fft2 / np.fft.ifft2 with the builder's `s` (numpy 2 keeps complex64 in, complex64 out, as FFTW's single precision does)
  - cv2 (track_targets.py only): `imread(path, IMREAD_GRAYSCALE)` returns the array registered for that path; nothing else is used
  - icepy4d.core / icepy4d.utils / tqdm (track_targets.py only): an `Image` with `.name` / `.path`, a no-op logger, the identity
The images are decoded with PIL and converted to 8-bit gray ("L"); the uint8 crops are stored next to the outputs, so the tests never
decode anything. The float32 images and the rolled synthetic image are not stored: `tests/oc_oracle.py:derived_inputs` rebuilds them
from the stored ones with exactly rounded numpy operations, the same recipe here and in the tests. The file is written with fixed zip timestamps: it regenerates byte for byte."""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oc_oracle import derived_inputs  # noqa: E402  (the recipe the tests use to rebuild the inputs that are not stored)
OUT = os.path.join(ROOT, "tests", "golden", "g11_templatematch.npz")
EPOCHS = ["IMG_2637.jpg", "IMG_2658.jpg", "IMG_2671.jpg", "IMG_2687.jpg"]
CROP = (slice(260, 516), slice(400, 784))     # 256 x 384 of the 800 x 1200 frames


def _pyfftw_stub():
    m = types.ModuleType("pyfftw")
    m.config = types.SimpleNamespace(PLANNER_EFFORT=None)
    m.empty_aligned = lambda shape, dtype="complex64", order="C", n=None: np.empty(shape, dtype=dtype, order=order)

    def fft2(a, s=None, **_):
        return lambda x: np.fft.fft2(x, s=None if s is None else tuple(int(v) for v in s))

    def ifft2(a, s=None, **_):
        return lambda x: np.fft.ifft2(x, s=None if s is None else tuple(int(v) for v in s))

    m.builders = types.SimpleNamespace(fft2=fft2, ifft2=ifft2)
    return m


def _load(ref_root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def synthetic_image(rng):
    """Smooth random texture (uint8): rolled by more than wkeep it puts the correlation peak on the edge of C."""
    from scipy import ndimage
    sa = ndimage.gaussian_filter(rng.normal(0, 1, (160, 200)), 6)
    return np.clip((sa - sa.min()) / (sa.max() - sa.min()) * 255, 0, 255).astype(np.uint8)


def main(ref_root):
    from PIL import Image as PILImage

    saved = {k: sys.modules.get(k) for k in ("pyfftw", "cv2", "icepy4d", "icepy4d.core", "icepy4d.utils", "icepy4d.matching",
                                             "icepy4d.matching.templatematch", "tqdm")}
    sys.modules["pyfftw"] = _pyfftw_stub()
    try:
        tm = _load(ref_root, "src/icepy4d/matching/templatematch.py", "icepy4d.matching.templatematch")
        imgs = [np.asarray(PILImage.open(os.path.join(ref_root, "assets/img/cam1", f)).convert("L"))[CROP] for f in EPOCHS]
        g = {f"img{i}": im for i, im in enumerate(imgs)}
        rng = np.random.default_rng(11)

        def run(prefix, A, B, xy, T, S, du0, dv0, single):
            t = tm.TemplateMatch(A=A, B=B, xy=xy, template_width=T, search_width=S, initialdu=du0, initialdv=dv0, single_points=single)
            pu_in, pv_in = t.pu.copy(), t.pv.copy()
            r = t.match()
            g[prefix + "_xy"] = xy
            g[prefix + "_TS"] = np.array([T, S])
            g[prefix + "_pu_in"], g[prefix + "_pv_in"] = pu_in, pv_in
            g[prefix + "_initdu"] = np.zeros(pu_in.shape) + du0
            g[prefix + "_initdv"] = np.zeros(pu_in.shape) + dv0
            for k in ("pu", "pv", "du", "dv", "peakCorr", "meanAbsCorr", "snr"):
                g[f"{prefix}_{k}"] = np.asarray(getattr(r, k), np.float64)

        # TemplateMatch defaults (128 / 144) on a meshgrid, scalar and per-point initial offsets
        xs = np.array([60.0, 80.0, 150.5, 222.0, 300.0, 320.5])
        ys = np.array([70.0, 100.5, 140.0, 160.0, 183.0, 190.0])
        run("grid", imgs[0], imgs[1], np.stack([xs, np.resize(ys, xs.size)], 1), 128, 144, 0, 0, False)
        run("grid_s", imgs[1], imgs[2], np.stack([xs, np.resize(ys, xs.size)], 1), 128, 144, 2.0, -1.5, False)
        n = xs.size
        run("grid_p", imgs[2], imgs[3], np.stack([xs, np.resize(ys, xs.size)], 1), 128, 144,
            rng.integers(-5, 6, (n, n)).astype(np.float64) + 0.5 * rng.integers(0, 2, (n, n)), rng.integers(-5, 6, (n, n)).astype(np.float64), False)
        # odd sizes and odd S - T
        xo = np.array([40.5, 80.0, 131.0, 200.5, 290.0, 340.0])
        run("odd", imgs[0], imgs[3], np.stack([xo, xo * 0.5 + 20.5], 1), 31, 100, 0, 0, False)
        # float32 images
        g["synth_a"] = synthetic_image(rng)
        g["forient_u8_in"] = imgs[3][60:108, 100:164]
        d = derived_inputs(g)     # float images, the rolled synthetic image: recomputed from the stored ones, not stored
        fa, fb = d["float_a"], d["float_b"]
        run("float", fa, fb, np.array([[60.0, 60.0], [100.0, 90.0], [150.5, 120.5], [200.0, 150.0], [240.0, 100.0]]), 48, 81, 0, 0, False)
        # synthetic pair rolled by more than wkeep = 16: peaks on the edge of C
        xsy = np.array([40.0, 60.5, 90.0, 120.0, 150.0])
        run("synth", g["synth_a"], d["synth_b"], np.stack([xsy, xsy * 0.6 + 10], 1), 32, 64, 0, 0, False)
        assert np.any(np.isnan(g["synth_du"]) & ~np.isnan(g["synth_meanAbsCorr"])), "no edge peak in the synthetic case"
        # forient of two images
        g["forient_u8"] = tm.forient(g["forient_u8_in"])
        g["forient_f32"] = tm.forient(d["forient_f32_in"])

        # TrackTargets defaults (32 / 128, single points): master epoch 0, three slaves, ~40 targets
        reg = {}
        cv2 = types.ModuleType("cv2")
        cv2.IMREAD_GRAYSCALE = 0
        cv2.imread = lambda p, flag=None: reg[str(p)]
        core = types.ModuleType("icepy4d.core")

        class Image:
            def __init__(self, path):
                self.path = Path(path)
                self.name = self.path.stem
        core.Image, core.Targets = Image, object
        utils = types.ModuleType("icepy4d.utils")
        utils.setup_logger = lambda *a, **k: None
        utils.get_logger = lambda *a, **k: types.SimpleNamespace(info=lambda *a, **k: None)
        tq = types.ModuleType("tqdm")
        tq.tqdm = lambda x, **k: x
        pkg = types.ModuleType("icepy4d")
        pkg.__path__ = []
        mpkg = types.ModuleType("icepy4d.matching")
        mpkg.__path__ = []
        mpkg.templatematch = tm
        sys.modules.update({"cv2": cv2, "icepy4d": pkg, "icepy4d.core": core, "icepy4d.utils": utils, "tqdm": tq,
                            "icepy4d.matching": mpkg, "icepy4d.matching.templatematch": tm})
        tt = _load(ref_root, "src/icepy4d/utils/track_targets.py", "icepy4d.utils.track_targets")
        h, w = imgs[0].shape
        tx = np.concatenate([rng.uniform(40, w - 40, 30).round(1), rng.integers(50, w - 50, 6) + 0.5, [10.0, w - 20.0, 200.0, np.nan]])
        ty = np.concatenate([rng.uniform(40, h - 40, 30).round(1), rng.integers(50, h - 50, 6) + 0.5, [100.0, 100.0, h - 5.0, 120.0]])
        targets = np.stack([tx, ty], 1)
        names = [f"T{i}" for i in range(len(targets))]
        g["track_targets"] = targets
        with tempfile.TemporaryDirectory() as d:
            for i, im in enumerate(imgs):
                reg[os.path.join(d, f"epoch{i}.png")] = im
            slaves = [Image(os.path.join(d, f"epoch{i}.png")) for i in (1, 2, 3)]
            tr = tt.TrackTargets(master=Path(os.path.join(d, "epoch0.png")), images=slaves, targets=targets.copy(),
                                 out_dir=os.path.join(d, "out"), target_names=names)
            tr.track()
            for i, sl in enumerate(slaves):
                res = tr.results[sl.name]
                for k in ("pu", "pv", "du", "dv", "x_est", "y_est", "snr", "peak_corr", "meanAbsCorr"):
                    g[f"track{i}_{k}"] = np.asarray(res[k], np.float64)
                g[f"track{i}_csv"] = np.frombuffer(open(os.path.join(d, "out", f"{sl.name}.csv"), "rb").read(), np.uint8)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    _save(OUT, g)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e6:.2f} MB)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_golden_templatematch.py REFERENCE_ROOT  (a checkout of franioli/icepy4d)")
    main(sys.argv[1])
