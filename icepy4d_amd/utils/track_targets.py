"""Target tracking through a season of epochs (reference `src/icepy4d/utils/track_targets.py`, `TrackTargets`): same config keys and
defaults, the same result dict per image and byte-identical per-image CSV files. `track()` correlates every target in every slave
image in ONE device launch (`matching.templatematch.match_many`) instead of a process pool; `parallel=True` only selects the list
form of the results that the reference's `pool.map` returns. `viz_tracked` is accepted and skipped with a warning.

master / images may be arrays, paths or objects with `.path` and `.name` (the reference's `icepy4d.core.Image`); paths are read with
`cv2.imread(..., cv2.IMREAD_GRAYSCALE)` as in the reference, which needs OpenCV. An array image is named by its index in `images`."""
import logging
import warnings
from pathlib import Path
from typing import List

import numpy as np

from ..matching.templatematch import TemplateMatch, match_many

logger = logging.getLogger(__name__)


def _read_gray(src) -> np.ndarray:
    if isinstance(src, np.ndarray):
        return src
    try:
        import cv2
    except ImportError as e:
        raise ImportError(f"reading {src} needs OpenCV (cv2); pass the image as a 2-D array instead") from e
    img = cv2.imread(str(src), cv2.IMREAD_GRAYSCALE)
    if img is None:
        raise FileNotFoundError(f"cannot read image {src}")
    return img


class TrackTargets:
    # Define default config
    def_config = {
        "template_width": 32,
        "search_width": 128,
        "viz_tracked": False,
        "verbose": False,
        "snr_threshold": 7.0,
        "parallel": False,
        "num_workers": None,
    }
    valid_methods = ["OC"]

    def __init__(self, master, images: List, targets: np.ndarray, method: str = "OC", out_dir: str = "results",
                 target_names: List[str] = None, engine=None, **config) -> None:
        if not isinstance(images, list):
            raise TypeError("images must be a list of Image objects")

        if not isinstance(master, (Path, str, np.ndarray)):
            raise TypeError("master must be a Path object with the path to the master image (or the image as an array)")

        if not isinstance(targets, np.ndarray) or targets.shape[1] != 2:
            raise TypeError(
                "targets must be a numpy vector of shape (n, 2) containing the image coordinates of the targets to track"
            )

        if method not in self.valid_methods:
            raise ValueError(f"Method {method} currentely not supported. Use {self.valid_methods}")

        self.cfg = {**self.def_config, **config}
        if self.cfg["viz_tracked"]:
            warnings.warn("TrackTargets: viz_tracked is not supported (no drawing); the option is skipped", stacklevel=2)

        self.images = images
        self.targets = targets
        self.target_names = target_names
        self.method = method
        self.engine = engine
        self.out_dir = Path(out_dir)
        self.out_dir.mkdir(parents=True, exist_ok=True)

        self._master = _read_gray(master)
        self._slave = None

        self.results = {}

    @staticmethod
    def _name(slave, i: int) -> str:
        if hasattr(slave, "name") and not isinstance(slave, np.ndarray):
            return slave.name
        if isinstance(slave, (str, Path)):
            return Path(slave).stem
        return str(i)

    @staticmethod
    def _source(slave):
        return slave.path if hasattr(slave, "path") else slave

    def _result(self, slave_name: str, r: dict, k: int) -> dict:
        """The reference's result dict and CSV file (`track_targets.py:101-152`) from row k of `match_many`."""
        target_names = self.target_names
        snr_threshold = self.cfg["snr_threshold"]
        du, dv = r["du"][k], r["dv"][k]
        x_est = self.targets[:, 0] + du
        y_est = self.targets[:, 1] + dv
        with np.errstate(invalid="ignore", divide="ignore"):
            snr = r["peakCorr"][k] / r["meanAbsCorr"][k]
        peak_corr = r["peakCorr"][k]
        result = {
            "image": slave_name,
            "targets_names": target_names,
            "targets_coord": self.targets,
            "pu": r["pu"][k],
            "pv": r["pv"][k],
            "du": du,
            "dv": dv,
            "x_est": x_est,
            "y_est": y_est,
            "snr": snr,
            "peak_corr": peak_corr,
            "meanAbsCorr": r["meanAbsCorr"][k],
        }

        if self.cfg["verbose"]:
            msg = ""
            for n, u, v, s, p in zip(target_names, du, dv, snr, peak_corr):
                if s > snr_threshold:
                    msg += f"{slave_name}\t\t{n}\t{u:.2f}\t\t{v:.2f}\t\t{s:.2f}\t\t{p:.2f}\n"
                else:
                    msg += f"{slave_name}\t\t{n}\tRejected\n"
            print(msg)

        fname = self.out_dir / f"{slave_name}.csv"
        with open(fname, "w") as f:
            f.write("label,x,y\n")
            for name, x, y, s in zip(target_names, x_est, y_est, snr):
                if s > snr_threshold:
                    f.write(f"{name},{x:.3f},{y:.3f}\n")
        return result

    def _match(self, slaves: List[np.ndarray]) -> dict:
        # single_points=True: the diagonal of the meshgrid of the targets' coordinates, i.e. the targets themselves
        TemplateMatch(A=self._master, B=slaves[0], xy=self.targets, method=self.method)   # the reference's validation
        return match_many(self._master, slaves, self.targets[:, 0], self.targets[:, 1], self.cfg["template_width"],
                          self.cfg["search_width"], engine=self.engine)

    def track_image(self, slave) -> dict:
        """Track the targets in one image."""
        i = next((k for k, s in enumerate(self.images) if s is slave), 0)
        r = self._match([_read_gray(self._source(slave))])
        return self._result(self._name(slave, i), r, 0)

    def track(self) -> None:
        """Track the targets in every image: one forient launch for the slaves and one correlation launch for all (target, image)
        pairs of equally sized images."""
        if self.cfg["verbose"]:
            print("Image\t\t\t\t\ttarget\tdu\t\tdv\t\tSNR\t\tPeak Corr")
        imgs = [_read_gray(self._source(s)) for s in self.images]
        names = [self._name(s, i) for i, s in enumerate(self.images)]
        results = [None] * len(imgs)
        by_shape = {}
        for i, im in enumerate(imgs):
            by_shape.setdefault(np.asarray(im).shape, []).append(i)
        for idx in by_shape.values():
            r = self._match([imgs[i] for i in idx])
            for k, i in enumerate(idx):
                results[i] = self._result(names[i], r, k)
        if self.cfg["parallel"]:
            self.results = results
        else:
            for name, res in zip(names, results):
                self.results[name] = res
        logger.info("Tracking completed.")
