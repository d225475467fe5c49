"""Matcher plugin API of the reference (`src/icepy4d/matching/matchers.py`), host side, bound to libicematch.

Same class / method names, arguments and result properties as the reference:
`FeaturesBase` (`:44-48`), `ImageMatcherBase.match` (`:139-261`), the plugin hook
`_match_images(image0, image1, **config) -> (FeaturesBase, FeaturesBase, matches0, mconf)` (`:276-302`),
`_match_by_tile` (`:304-469`), `_tile_selection` (`:471-581`), `LightGlueMatcher` (`:1202-1342`),
`SuperGlueMatcher` (`:826-940`). What differs is only where the arithmetic runs: `_match_images` enqueues the
SuperPoint + LightGlue / SuperGlue kernels of libicematch on the MI355X (no torch modules, no CPU fallback) and
copies the results back once.

Observable quirks of the reference are kept where downstream code can depend on them (q1: LightGlueMatcher with
TileSelection.NONE stores the *unfiltered* keypoints; q4: tiles lose their last row/column; q5: `mconf` of
SuperGlue / tile modes is the keypoint score; q6: tile matches are re-ordered by `np.unique`). Two more are plain bugs,
but they change RESULTS, so they are reproduced by default and can be switched off together with `opt["reference_quirks"] =
False`: q2 - the reference hands its options to `_tile_selection` as ONE keyword (`config=config`, `matchers.py:353-355`), so
`min_matches_per_tile` is never found there and the preselection threshold is always 5 (`:502`), whatever the caller passes
(`main_dev.py:127` passes 3); q7 - a bare `except` around `extract(..., resize=)` silently retries without `resize`
(`:1262-1267`). With the switch off `min_matches_per_tile` is honoured and errors of the resize path propagate. The golden
`tests/golden/g8_preselection.npz` (the reference's own `match()` in PRESELECTION mode) pins the default. q9 (Tk import at
module load) is not reproduced. Weights: the reference downloads / reads `.pth` files at construction; here a state dict (official
key names) is passed through `opt["state_dicts"]` or `opt["weights_dir"]`.
"""
from __future__ import annotations

import logging
import os
from abc import ABC, abstractmethod
from copy import deepcopy
from dataclasses import dataclass
from itertools import product
from pathlib import Path
from typing import Dict, List, Tuple, Union

import numpy as np
import torch

from .._lib import IcematchError
from ..engine import get_engine      # re-exported: matchers.get_engine is where user code finds it
from ..utils import AverageTimer, timeit
from .enums import GeometricVerification, Quality, TileSelection
from .geometric_verification import geometric_verification
from .pyramid import pyr_down, pyr_up
from .tiling import Tiler

logger = logging.getLogger(__name__)

MIN_MATCHES_PER_TILE = 5


def _on_engine_device(method):
    """Runs a matcher method with the engine's device as torch's current device (streams, allocations, graph replays and
    synchronisation then refer to that device whatever the caller's current device is: one process may hold matchers on several GPUs)."""
    import functools

    @functools.wraps(method)
    def wrapped(self, *args, **kwargs):
        with torch.cuda.device(self.engine.device):
            return method(self, *args, **kwargs)
    return wrapped


def check_dict_keys(dict: dict, keys: List[str]):
    """KeyError naming every required option that `dict` lacks (`matchers.py:40-47`)."""
    absent = sorted(set(keys) - set(dict))
    if absent:
        raise KeyError(f"matcher options lack the required entries {absent}")


@dataclass
class FeaturesBase:
    keypoints: np.ndarray
    descriptors: np.ndarray = None
    scores: np.ndarray = None


def _as_device_image(image: np.ndarray) -> np.ndarray:
    """What the kernels take: contiguous uint8 [H, W] (gray) or [H, W, 3] (RGB, `core/images.py:75`). The u8 -> float scaling
    and the gray conversion of 3-channel input happen on the device, per pixel, inside the first convolution, in the
    reference's order and arithmetic (LightGlue flavour: float image, kornia weights, `lightglue/utils.py:35-36`; SuperGlue
    flavour: cv2.cvtColor on uint8, `matchers.py:911-914`): no host pass over the image, no rounding to a uint8 gray."""
    if image.dtype != np.uint8:
        raise TypeError(f"uint8 image expected, got {image.dtype}")
    if image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 3):
        return np.ascontiguousarray(image)
    if image.ndim == 3 and image.shape[2] == 1:
        return np.ascontiguousarray(image[..., 0])
    raise ValueError(f"Not an image: {image.shape}")


def _preprocess_once(x: "torch.Tensor", resize: int) -> Tuple["torch.Tensor", np.ndarray]:
    """One `ImagePreprocessor.__call__` (`lightglue/utils.py:26-39`) on a float [C, h, w] image: kornia `resize(img, resize,
    side="long", antialias=True, align_corners=None, interpolation="bilinear")`, then `rgb_to_grayscale` if C == 3. kornia is
    un-vendored and absent: its published algorithm is restated with torch CPU ops (Gaussian blur with sigma = (factor - 1) / 2
    per axis, kernel size int(max(4 sigma, 3)) made odd, reflect border, before a bilinear `F.interpolate` when downscaling) -
    parity unpinned. Returns (image', scales = [w' / w, h' / h])."""
    import torch.nn.functional as F
    h, w = x.shape[-2:]
    aspect = w / h
    size = (int(resize / aspect), int(resize)) if aspect > 1 else (int(resize), int(resize * aspect))
    if size != (h, w):
        factors = (h / size[0], w / size[1])
        x = x[None]
        if max(factors) > 1:
            sig = [max((f - 1.0) / 2.0, 0.001) for f in factors]
            ks = [int(max(2.0 * 2 * s_, 3)) for s_ in sig]
            ks = [k + 1 if k % 2 == 0 else k for k in ks]

            def gauss(k, s_):
                t = torch.arange(k, dtype=torch.float) - k // 2
                g = torch.exp(-t ** 2 / (2.0 * s_ ** 2))
                return g / g.sum()

            ky, kx = gauss(ks[0], sig[0]), gauss(ks[1], sig[1])
            c = x.shape[1]
            x = F.pad(x, (ks[1] // 2, ks[1] // 2, ks[0] // 2, ks[0] // 2), mode="reflect")
            x = F.conv2d(x, kx.view(1, 1, 1, -1).repeat(c, 1, 1, 1), groups=c)
            x = F.conv2d(x, ky.view(1, 1, -1, 1).repeat(c, 1, 1, 1), groups=c)
        x = F.interpolate(x, size=size, mode="bilinear", align_corners=None)[0]
    scales = np.array([x.shape[-1] / w, x.shape[-2] / h], dtype=np.float32)
    if x.shape[0] == 3:
        x = (0.299 * x[0:1] + 0.587 * x[1:2]) + 0.114 * x[2:3]
    return x, scales


def _resized_gray(image: np.ndarray, resize: int) -> Tuple[np.ndarray, np.ndarray]:
    """`SuperPoint.extract(img, resize=...)` (`lightglue/superpoint.py:217-231`) up to the network input: u8 -> float / 255
    (`matchers.py:1212-1220`), then the reference's TWO `ImagePreprocessor` calls (`superpoint.py:224-227`). The second call sees
    the already resized gray image, so the `scales` that `extract` finally uses are those of the second call - [1, 1] unless
    int() rounds the target size differently for the resized aspect ratio - and the keypoints stay in the RESIZED frame while
    `image_size` is the original (W, H): that observable behaviour is reproduced here. Returns (float32 gray [H', W'] in [0, 1],
    scales of the second call). icepy4d itself never passes `resize` (`matchers.py:1247-1248` reads it from **config,
    `main_dev.py:115-132` does not set it)."""
    x = torch.tensor(image / 255.0, dtype=torch.float)
    x = x.permute(2, 0, 1) if x.dim() == 3 else x[None]
    x, _ = _preprocess_once(x, resize)
    x, scales = _preprocess_once(x, resize)
    return np.ascontiguousarray(x[0].numpy()), scales


_WEIGHT_FILES: Dict[tuple, Dict[str, torch.Tensor]] = {}


def _load_state_dict(opt: dict, model: str, filenames: List[str]) -> Dict[str, torch.Tensor]:
    sds = opt.get("state_dicts") or {}
    if model in sds:
        return sds[model]
    wdir = opt.get("weights_dir") or os.environ.get("ICEPY4D_AMD_WEIGHTS")
    if wdir:
        for fn in filenames:
            p = Path(wdir) / fn
            if p.exists():
                # one load per file version: a matcher per epoch (`main_dev.py:115-132`) re-uses the dict (and, through the
                # fingerprint memo, the device weights and the captured graph)
                st = p.stat()
                key = (str(p.resolve()), st.st_mtime_ns, st.st_size)
                if key not in _WEIGHT_FILES:
                    if len(_WEIGHT_FILES) > 8:
                        _WEIGHT_FILES.clear()
                    _WEIGHT_FILES[key] = torch.load(str(p), map_location="cpu")
                return _WEIGHT_FILES[key]
    raise FileNotFoundError(
        f"No weights for '{model}': pass opt['state_dicts']['{model}'] (official key names) or opt['weights_dir'] "
        f"containing one of {filenames}. (The reference downloads them; this build has no network access.)")


class ImageMatcherABC(ABC):
    """The abstract interface of the reference (`matchers.py:51-65`): a matcher has `match`, `_match_images`, `_match_by_tile`."""

    @abstractmethod
    def match(self):
        ...

    @abstractmethod
    def _match_images(self):
        ...

    @abstractmethod
    def _match_by_tile(self):
        ...


class ImageMatcherBase(ImageMatcherABC):
    def __init__(self, opt: dict = {}) -> None:
        """Base class for matchers: `match()` and everything shared; subclasses implement `_match_images`.

        Raises:
            TypeError: If `opt` is not a dictionary.
        """
        if not isinstance(opt, dict):
            raise TypeError("opt must be a dictionary")
        self._opt = dict(opt)
        # True (default): results identical to the reference also where it ignores an option by accident (q2, q7: module docstring)
        self._reference_quirks = bool(opt.get("reference_quirks", True))
        if opt.get("force_cpu"):
            logger.warning("force_cpu is ignored: the MI355X build has no CPU path")
        self._device_index = int(opt.get("device", 0))
        self._device = f"cuda:{self._device_index}"
        self._engine = None
        self._state_dicts: Dict[str, dict] = {}
        self.reset()

    @property
    def engine(self):
        if self._engine is None:
            self._engine = get_engine(self._device_index, self._state_dicts, bool(self._opt.get("private_engine", False)))
        return self._engine

    def reset(self):
        """Reset the matcher by clearing the features and matches"""
        self._mkpts0 = None
        self._mkpts1 = None
        self._descriptors0 = None
        self._descriptors1 = None
        self._scores0 = None
        self._scores1 = None
        self._mconf = None

    device = property(lambda self: self._device)
    mkpts0 = property(lambda self: self._mkpts0)
    mkpts1 = property(lambda self: self._mkpts1)
    descriptors0 = property(lambda self: self._descriptors0)
    descriptors1 = property(lambda self: self._descriptors1)
    scores0 = property(lambda self: self._scores0)
    scores1 = property(lambda self: self._scores1)
    mconf = property(lambda self: self._mconf)

    @timeit
    @_on_engine_device
    def match(self, image0: np.ndarray, image1: np.ndarray, quality: Quality = Quality.HIGH,
              tile_selection: TileSelection = TileSelection.NONE, **config) -> bool:
        """Matches images and performs geometric verification (`matchers.py:139-261`)."""
        self.timer = AverageTimer()
        gv_method = config.get("geometric_verification", GeometricVerification.PYDEGENSAC)
        threshold = config.get("threshold", 1)
        confidence = config.get("confidence", 0.9999)
        save_dir = config.get("save_dir", None)
        self._save_dir = Path(save_dir) if save_dir is not None else None
        if self._save_dir is not None:
            self._save_dir.mkdir(parents=True, exist_ok=True)

        if config.get("do_viz_matches") or config.get("do_viz_tiles") or config.get("do_viz"):
            logger.warning("match(): the do_viz_* options are accepted but nothing is drawn (visualisation is out of scope)")
        image0_, image1_ = self._resize_images(quality, image0, image1)
        if tile_selection == TileSelection.NONE:
            logger.info("Matching full images...")
            features0, features1, matches0, mconf = self._match_images(image0_, image1_, **config)
        else:
            logger.info("Matching by tiles...")
            features0, features1, matches0, mconf = self._match_by_tile(image0_, image1_, tile_selection, **config)
        features0, features1 = self._resize_features(quality, features0, features1)
        try:
            self._store_features(features0, features1, matches0)
            self._mconf = mconf
        except Exception as e:  # same behaviour as the reference: log and go on (`matchers.py:199-207`)
            logger.error(f"Error storing matches: {e}. Implement your own _store_features() method if the "
                         f"output of your matcher is different from FeaturesBase.")
        self.timer.update("matching")
        logger.info("Matching done!")

        if gv_method is not GeometricVerification.NONE and len(self._mkpts0) != len(self._mkpts1):
            # q1: LightGlueMatcher + TileSelection.NONE stores unpaired keypoint sets; the reference's verification
            # then fails inside pydegensac / cv2 and keeps everything (`geometric_verification.py:79-100`)
            logger.error("Geometric verification skipped: keypoint sets are not paired (use a tile mode)")
        elif gv_method is not GeometricVerification.NONE:
            F, inl = geometric_verification(self._mkpts0, self._mkpts1, method=gv_method, confidence=confidence,
                                            threshold=threshold, engine=self.engine)   # hypotheses scored on the device
            self._F = F
            self._filter_matches_by_mask(inl)
            self.timer.update("geometric_verification")
        if self._save_dir is not None:
            self.save_mkpts_as_txt(self._save_dir)
        self.timer.print("Matching")
        return True

    def _match_images(self, image0: np.ndarray, image1: np.ndarray, **config
                      ) -> Tuple[FeaturesBase, FeaturesBase, np.ndarray, np.ndarray]:
        raise NotImplementedError("Subclasses must implement _match_full_images() method.")

    def _match_by_tile(self, image0: np.ndarray, image1: np.ndarray,
                       tile_selection: TileSelection = TileSelection.PRESELECTION, **config
                       ) -> Tuple[FeaturesBase, FeaturesBase, np.ndarray, np.ndarray]:
        """Tile loop (`matchers.py:304-469`): match every selected tile pair, keep the valid matches, shift them by
        the tile origin, concatenate, `np.unique` on the image-0 points, return 1-to-1 matches."""
        assert isinstance(image0, np.ndarray), "image0 must be a NumPy array"
        assert isinstance(image1, np.ndarray), "image1 must be a NumPy array"
        grid = config.get("grid", [1, 1])
        overlap = config.get("overlap", 0)
        origin = config.get("origin", [0, 0])
        self._tiler = Tiler(grid=grid, overlap=overlap, origin=origin)
        t0_lims, t0_origin = self._tiler.compute_limits_by_grid(image0)
        t1_lims, t1_origin = self._tiler.compute_limits_by_grid(image1)
        # each full image crosses PCIe ONCE per call: the preselection's pyramid and every tile crop read the device copy (round 6: the host
        # crops, their stacking and per-tile uploads were ~50 of the production call's 306 ms, profiles/r06_production_call_kernel_stats.csv)
        self._dev_images = {}
        try:
            return self._match_by_tile_body(image0, image1, t0_lims, t0_origin, t1_lims, t1_origin, tile_selection, **config)
        finally:
            self._dev_images = {}

    def _device_image(self, image: np.ndarray):
        """The device copy of a full image of the current tile call (uint8, contiguous, [H, W] or [H, W, 3])."""
        cache = getattr(self, "_dev_images", None)
        if cache is None:
            cache = self._dev_images = {}
        key = id(image)
        if key not in cache:
            cache[key] = torch.from_numpy(_as_device_image(image)).to(self.engine.device)
        return cache[key]

    def _match_by_tile_body(self, image0, image1, t0_lims, t0_origin, t1_lims, t1_origin, tile_selection, **config):
        tile_pairs = self._tile_selection(image0, image1, t0_lims, t1_lims, tile_selection, **config)

        mk0, mk1 = [np.zeros((0, 2), np.float32)], [np.zeros((0, 2), np.float32)]
        d0, d1 = [np.zeros((256, 0), np.float32)], [np.zeros((256, 0), np.float32)]
        s0, s1 = [np.zeros(0, np.float32)], [np.zeros(0, np.float32)]
        # Row f-1 of the scope table: the reference re-runs SuperPoint on both tiles of EVERY tile pair
        # (`matchers.py:367-394`), i.e. up to 16 x 2 extractions for a 2 x 2 grid. Extraction is a pure function of the
        # tile, so each distinct tile is extracted once on the device and its features are reused by all its pairs
        # (bit-identical results, tested against the per-pair path).
        cache = self._extract_tiles(image0, image1, t0_lims, t1_lims, tile_pairs, **config)
        if cache is not None and not self._opt.get("host_tile_merge", False):
            return self._match_tiles_device(cache, tile_pairs, t0_lims, t1_lims, t0_origin, t1_origin, **config)
        for tidx0, tidx1 in tile_pairs:
            logger.info(f" - Matching tile pair ({tidx0}, {tidx1})")
            lim0, lim1 = t0_lims[tidx0], t1_lims[tidx1]
            if cache is not None:
                f0, f1, matches0, _ = self._match_cached(cache[(0, tidx0)], cache[(1, tidx1)], **config)
            else:
                tile0 = self._tiler.extract_patch(image0, lim0)
                tile1 = self._tiler.extract_patch(image1, lim1)
                f0, f1, matches0, _ = self._match_images(tile0, tile1, **config)
            valid = matches0 > -1
            idx1 = matches0[valid]
            mk0.append(f0.keypoints[valid] + np.array(lim0[0:2]).astype("float32"))
            mk1.append(f1.keypoints[idx1] + np.array(lim1[0:2]).astype("float32"))
            d0.append(f0.descriptors[:, valid])
            d1.append(f1.descriptors[:, idx1])
            s0.append(f0.scores[valid])
            s1.append(f1.scores[idx1])
        mk0 = np.vstack(mk0) + np.array(t0_origin).astype("float32")
        mk1 = np.vstack(mk1) + np.array(t1_origin).astype("float32")
        d0, d1, s0, s1 = np.hstack(d0), np.hstack(d1), np.concatenate(s0), np.concatenate(s1)
        mk0, uniq = np.unique(mk0, axis=0, return_index=True)  # q6: lexicographic re-ordering
        features0 = FeaturesBase(keypoints=mk0, descriptors=d0[:, uniq], scores=s0[uniq])
        features1 = FeaturesBase(keypoints=mk1[uniq], descriptors=d1[:, uniq], scores=s1[uniq])
        matches0 = np.arange(mk0.shape[0])
        mconf = features0.scores[matches0 > -1]  # q5: keypoint scores, not match confidences
        logger.info("Matching by tile completed.")
        return features0, features1, matches0, mconf

    def _tile_selection(self, image0: np.ndarray, image1: np.ndarray, t0_lims: Dict[int, tuple],
                        t1_lims: Dict[int, tuple], method: TileSelection = TileSelection.PRESELECTION, **config
                        ) -> List[Tuple[int, int]]:
        """Tile pairs to match (`matchers.py:471-581`)."""
        def points_in_rect(points: np.ndarray, rect) -> np.ndarray:
            rect = np.asarray(rect)
            return np.all(points > rect[:2], axis=1) & np.all(points < rect[2:], axis=1)

        if self._reference_quirks:
            # q2: the reference's caller passes `config=config` (`matchers.py:353-355`), so this lookup never finds the option there
            # (`:502`) and the threshold is always MIN_MATCHES_PER_TILE = 5 - also for `main_dev.py:127`'s min_matches_per_tile=3
            if config.get("min_matches_per_tile", MIN_MATCHES_PER_TILE) != MIN_MATCHES_PER_TILE:
                logger.info(f"min_matches_per_tile={config['min_matches_per_tile']} is ignored as in the reference (threshold "
                            f"{MIN_MATCHES_PER_TILE}); pass opt['reference_quirks']=False to honour it")
            min_matches_per_tile = MIN_MATCHES_PER_TILE
        else:
            min_matches_per_tile = config.get("min_matches_per_tile", MIN_MATCHES_PER_TILE)
        if method == TileSelection.EXHAUSTIVE:
            return sorted(product(t0_lims.keys(), t1_lims.keys()))
        if method == TileSelection.GRID:
            return sorted(zip(t0_lims.keys(), t1_lims.keys()))
        if method == TileSelection.PRESELECTION:
            # pyramid depth by image height (`matchers.py:516-523`; the >8000 branch is dead in the reference: q3)
            if image0.shape[0] > 4000:
                n_down = 3
            elif image0.shape[0] > 2000:
                n_down = 2
            else:
                n_down = 1
            i0 = pyr_down(image0, self.engine, n_down, device_image=self._pyr_source(image0, **config))   # levels stay on the device
            i1 = pyr_down(image1, self.engine, n_down, device_image=self._pyr_source(image1, **config))
            f0, f1, mtc, _ = self._match_images(i0, i1, max_keypoints=4096)
            vld = mtc > -1
            kp0 = f0.keypoints[vld] * (2 ** n_down)
            kp1 = f1.keypoints[mtc[vld]] * (2 ** n_down)
            pairs = []
            for tidx0, tidx1 in sorted(product(t0_lims.keys(), t1_lims.keys())):
                ret = points_in_rect(kp0, t0_lims[tidx0]) & points_in_rect(kp1, t1_lims[tidx1])
                if int(ret.sum()) > min_matches_per_tile:
                    pairs.append((tidx0, tidx1))
            self.timer.update("preselection")
            return pairs
        raise ValueError(f"unknown tile selection {method}")

    def _pyr_source(self, image: np.ndarray, **config):
        """The device copy of `image` for the pyramid when the tile matcher is going to need it anyway (a subclass with a tile cache); None otherwise."""
        if self._sp_params(**config) is None or image.dtype != np.uint8 or not (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 3)):
            return None
        return self._device_image(image)

    def _resize_images(self, quality: Quality, image0: np.ndarray, image1: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """`matchers.py:583-610`: HIGHEST = pyrUp, HIGH = identity, MEDIUM = pyrDown, LOW = pyrDown twice."""
        if quality == Quality.HIGHEST:
            return pyr_up(image0, self.engine), pyr_up(image1, self.engine)
        if quality == Quality.HIGH:
            return image0, image1
        if quality == Quality.MEDIUM:
            return pyr_down(image0, self.engine), pyr_down(image1, self.engine)
        if quality == Quality.LOW:
            return pyr_down(image0, self.engine, 2), pyr_down(image1, self.engine, 2)
        raise ValueError(f"unknown quality {quality}")

    def _resize_features(self, quality: Quality, features0: FeaturesBase, features1: FeaturesBase):
        """`matchers.py:612-639`."""
        f = {Quality.HIGHEST: 0.5, Quality.HIGH: 1.0, Quality.MEDIUM: 2.0, Quality.LOW: 4.0}[quality]
        if f != 1.0:
            features0.keypoints = features0.keypoints * np.float32(f)
            features1.keypoints = features1.keypoints * np.float32(f)
        return features0, features1

    def _store_features(self, features0: FeaturesBase, features1: FeaturesBase, matches0: np.ndarray,
                        force_overwrite: bool = True) -> bool:
        """Keeps the matched subset: row i of image 0 goes with row matches0[i] of image 1 wherever matches0[i] > -1
        (`matchers.py:641-680`); descriptors are [256, n] column-wise, as the reference stores them."""
        for f in (features0, features1):
            assert isinstance(f, FeaturesBase), "features0 / features1 must be FeaturesBase objects"
        have_matches = self._mkpts0 is not None and self._mkpts1 is not None
        if have_matches and not force_overwrite:
            logger.warning("matches are already stored and force_overwrite is False: keeping the old ones")
            return False
        self._valid = matches0 > -1
        rows0, rows1 = np.flatnonzero(self._valid), matches0[self._valid]
        self._mkpts0, self._mkpts1 = features0.keypoints[rows0], features1.keypoints[rows1]
        if features0.descriptors is not None:
            self._descriptors0, self._descriptors1 = features0.descriptors[:, rows0], features1.descriptors[:, rows1]
        if features0.scores is not None:
            self._scores0, self._scores1 = features0.scores[rows0], features1.scores[rows1]
        return True

    def _filter_matches_by_mask(self, inlMask: np.ndarray) -> None:
        """Drops the matches the verification rejected from every stored per-match array (`matchers.py:682-700`)."""
        for name, axis in (("_mkpts0", 0), ("_mkpts1", 0), ("_descriptors0", 1), ("_descriptors1", 1), ("_scores0", 0), ("_scores1", 0)):
            arr = getattr(self, name)
            if arr is not None:
                setattr(self, name, np.compress(inlMask, arr, axis=axis))
        if self._mconf is not None and len(self._mconf) == len(inlMask):
            self._mconf = self._mconf[inlMask]

    def save_mkpts_as_txt(self, savedir: Union[str, Path], delimiter: str = ",", header: str = "x,y") -> None:
        """Save keypoints in a .txt file (`matchers.py:802-824`)."""
        path = Path(savedir)
        path.mkdir(parents=True, exist_ok=True)
        np.savetxt(path / "keypoints_0.txt", self.mkpts0, delimiter=delimiter, newline="\n", header=header)
        np.savetxt(path / "keypoints_1.txt", self.mkpts1, delimiter=delimiter, newline="\n", header=header)

    # ------------------------------------------------------------------ visualisation entry points (out of scope: accepted, skipped)
    def viz_matches_mpl(self, *args, **kwargs) -> None:
        """`matchers.py:702-737` draws with matplotlib; visualisation is outside the hot-path scope: accepted and skipped with a
        warning, so that scripts written against the reference keep running."""
        logger.warning("viz_matches_mpl(): nothing is drawn (visualisation is out of scope of icepy4d_amd)")

    def viz_matches_cv2(self, *args, **kwargs) -> None:
        """`matchers.py:739-800` (OpenCV drawing): accepted and skipped with a warning."""
        logger.warning("viz_matches_cv2(): nothing is drawn (visualisation is out of scope of icepy4d_amd)")

    # ------------------------------------------------------------------ per-tile feature cache (tile modes)
    def _sp_params(self, **config):
        """(nms_radius, threshold, border, max_keypoints, flavour) of this matcher's SuperPoint; None = no tile cache."""
        return None

    def _extract_tiles(self, image0, image1, t0_lims, t1_lims, tile_pairs, **config):
        params = self._sp_params(**config)
        if params is None or not tile_pairs:
            return None
        radius, thr, border, max_k, flavour = params            # max_k < 0: every candidate (SuperGlue's max_keypoints = -1)
        eng = self.engine
        todo = sorted({(0, a) for a, _ in tile_pairs} | {(1, b) for _, b in tile_pairs})
        tiles = {}
        for k in todo:        # views of the device copy of the full image (`Tiler.extract_patch`'s slice): no host crop, no per-tile upload
            lim = (t0_lims if k[0] == 0 else t1_lims)[k[1]]
            tiles[k] = self._device_image(image0 if k[0] == 0 else image1)[lim[1]:lim[3], lim[0]:lim[2]]
        hmax, wmax = max(t.shape[0] for t in tiles.values()), max(t.shape[1] for t in tiles.values())
        cap = int(self._opt.get("max_keypoints_cap", 16384)) if max_k < 0 else int(max_k)
        cache = {}
        by_shape = {}
        for k in todo:
            by_shape.setdefault(tuple(tiles[k].shape), []).append(k)
        for shape, keys in by_shape.items():
            for i in range(0, len(keys), 2):  # two equal-sized tiles per launch
                grp = keys[i:i + 2]
                batch = torch.stack([tiles[k] for k in grp])      # one strided device copy per tile
                while True:
                    eng.reserve(hmax, wmax, 2, max(cap, 1))
                    eng.superpoint(batch, radius, thr, border, max_k, flavour=flavour)
                    if max_k >= 0 or max(eng.candidates()) <= eng.max_kpts:
                        break
                    cap = max(eng.candidates())                 # unlimited and more candidates than rows: grow, extract again
                for slot, k in enumerate(grp):
                    cache[k] = dict(kpts=eng.kpts[slot].clone(), scores=eng.scores[slot].clone(), desc=eng.desc[slot].clone(),
                                    n=eng.n[slot:slot + 1].clone(), shape=shape[:2])
        K = eng.max_kpts
        for c in cache.values():   # the workspace may have grown after a tile was cached: same row count everywhere
            if c["kpts"].shape[0] < K:
                pad = K - c["kpts"].shape[0]
                c["kpts"] = torch.nn.functional.pad(c["kpts"], (0, 0, 0, pad))
                c["scores"] = torch.nn.functional.pad(c["scores"], (0, pad))
                c["desc"] = torch.nn.functional.pad(c["desc"], (0, 0, 0, pad))
        return cache

    def _match_cached(self, c0: dict, c1: dict, **config):
        raise NotImplementedError

    def _enqueue_cached(self, c0: dict, c1: dict, **config) -> None:
        """Enqueue the matcher on one cached tile pair (no synchronisation); results land in the engine's buffers."""
        raise NotImplementedError

    def _match_tiles_device(self, cache, tile_pairs, t0_lims, t1_lims, t0_origin, t1_origin, **config):
        """Row f-1 of the scope table, second half: the whole tile loop of `matchers.py:367-469` without a host round
        trip per tile pair. Every pair is enqueued back to back (its [K] match vector is kept on the device); then ONE
        selection over all pairs gathers the matched keypoints from the per-tile feature banks, shifts them by the tile
        and image origins (same two fp32 additions, same order as the host loop), removes duplicate image-0 points the
        way `np.unique(axis=0)` does (lexicographic order, first occurrence kept: q6) and only the surviving rows -
        keypoints, 256-float descriptors, scores - cross PCIe. Output identical to the host merge (tested)."""
        eng = self.engine
        dev, K = eng.device, eng.max_kpts
        keys = sorted({(0, a) for a, _ in tile_pairs} | {(1, b) for _, b in tile_pairs})
        slot = {k: i for i, k in enumerate(keys)}
        KP = torch.stack([cache[k]["kpts"] for k in keys])          # [T, K, 2]
        SC = torch.stack([cache[k]["scores"] for k in keys])        # [T, K]
        DE = torch.stack([cache[k]["desc"] for k in keys])          # [T, K, 256]
        NN = torch.cat([cache[k]["n"] for k in keys])               # [T] int32
        P = len(tile_pairs)
        # tile pairs of equal shapes share their launches (a batch dimension over pairs inside the matcher's kernels): the
        # reference's loop (`matchers.py:367-394`) becomes one forward per group of up to `tile_pairs_per_launch` pairs
        groups: Dict[tuple, List[int]] = {}
        for p, (tidx0, tidx1) in enumerate(tile_pairs):
            groups.setdefault((cache[(0, tidx0)]["shape"], cache[(1, tidx1)]["shape"]), []).append(p)
        per_launch = max(1, min(int(self._opt.get("tile_pairs_per_launch", 8)), self._max_pairs_per_launch()))
        biggest = min(per_launch, max(len(v) for v in groups.values()))
        eng.reserve(eng.max_h, eng.max_w, 2 * biggest, K)
        M = torch.empty(P, K, dtype=torch.int32, device=dev)
        for plist in groups.values():
            for i in range(0, len(plist), per_launch):
                chunk = plist[i:i + per_launch]
                logger.info(f" - Matching tile pairs {[tile_pairs[p] for p in chunk]}")
                self._enqueue_cached_group([(cache[(0, tile_pairs[p][0])], cache[(1, tile_pairs[p][1])]) for p in chunk], **config)
                for j, p in enumerate(chunk):
                    M[p].copy_(eng.matches[2 * j])
        # one library call for the whole tail of the loop (`im_merge_tile_matches`): selection of the valid matches of every
        # pair, the two fp32 origin shifts, `np.unique(axis=0, return_index=True)` (lexicographic order, first occurrence) by
        # counting ranks on the device; then row gathers of descriptors / scores for the surviving matches only
        from .._lib import ptr
        slots = torch.tensor([[slot[(0, a)], slot[(1, b)]] for a, b in tile_pairs], dtype=torch.int32, device=dev)
        off = torch.tensor([[float(t0_lims[a][0]), float(t0_lims[a][1]), float(t1_lims[b][0]), float(t1_lims[b][1])]
                            for a, b in tile_pairs], dtype=torch.float32, device=dev)
        origin = np.array([t0_origin[0], t0_origin[1], t1_origin[0], t1_origin[1]], dtype=np.float32)
        cap = P * K
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        idx0 = torch.empty(cap, dtype=torch.int32, device=dev)
        idx1 = torch.empty(cap, dtype=torch.int32, device=dev)
        kp0 = torch.empty(cap, 2, device=dev)
        kp1 = torch.empty(cap, 2, device=dev)
        NN32 = NN.to(torch.int32)
        eng.ctx.call("im_merge_tile_matches", P, K, ptr(M), ptr(slots), ptr(off), origin.ctypes.data, ptr(KP), ptr(NN32), ptr(count),
                     ptr(idx0), ptr(idx1), ptr(kp0), ptr(kp1), eng.stream_ptr())
        S = int(count.item())                                       # the only host round trip of the tile loop
        out = []
        for idx, cols, bank in ((idx0, 256, DE), (idx1, 256, DE), (idx0, 1, SC), (idx1, 1, SC)):
            dst = torch.empty(S, cols, device=dev)
            eng.ctx.call("im_gather_rows", ptr(bank), cols, ptr(idx), S, ptr(dst), eng.stream_ptr())
            out.append(dst)
        d0, d1, sc0, sc1 = out
        features0 = FeaturesBase(keypoints=kp0[:S].cpu().numpy(), descriptors=np.ascontiguousarray(d0.cpu().numpy().T),
                                 scores=sc0[:, 0].cpu().numpy())
        features1 = FeaturesBase(keypoints=kp1[:S].cpu().numpy(), descriptors=np.ascontiguousarray(d1.cpu().numpy().T),
                                 scores=sc1[:, 0].cpu().numpy())
        matches0 = np.arange(features0.keypoints.shape[0])
        mconf = features0.scores[matches0 > -1]  # q5: keypoint scores, not match confidences
        logger.info("Matching by tile completed.")
        return features0, features1, matches0, mconf

    def _max_pairs_per_launch(self) -> int:
        return 1

    def _enqueue_cached_group(self, pairs: list, **config) -> None:
        """Enqueue the matcher on a group of cached tile pairs of equal shapes; pair j's matches land in rows 2j, 2j + 1 of
        the engine's output buffers. Default: one pair per call."""
        assert len(pairs) == 1
        self._enqueue_cached(pairs[0][0], pairs[0][1], **config)

    def _load_cached_pair(self, c0: dict, c1: dict, pair: int = 0) -> None:
        eng = self.engine
        for slot, c in enumerate((c0, c1)):
            slot += 2 * pair
            eng.kpts[slot].copy_(c["kpts"]); eng.scores[slot].copy_(c["scores"]); eng.desc[slot].copy_(c["desc"])
            eng.n[slot:slot + 1].copy_(c["n"])

    def _features_from_engine(self):
        (k0, d0, s0), (k1, d1, s1), out = self.engine.pair_to_host(0, channels_first=True, pageable=bool(self._opt.get("pageable_results", False)))
        f0 = FeaturesBase(keypoints=k0, descriptors=d0, scores=s0)
        f1 = FeaturesBase(keypoints=k1, descriptors=d1, scores=s1)
        return f0, f1, out

    # ------------------------------------------------------------------ shared device plumbing
    def _upload_pair(self, g0: np.ndarray, g1: np.ndarray) -> List[torch.Tensor]:
        dev = self.engine.device
        if g0.shape == g1.shape:
            return [torch.from_numpy(np.stack([g0, g1])).to(dev)]
        return [torch.from_numpy(g0[None].copy()).to(dev), torch.from_numpy(g1[None].copy()).to(dev)]


class SuperGlueMatcher(ImageMatcherBase):
    def __init__(self, opt: dict) -> None:
        """Options as in the reference (`matchers.py:829-890`): 'weights', 'keypoint_threshold', 'max_keypoints',
        'match_threshold', 'force_cpu' (+ 'nms_radius', 'sinkhorn_iterations')."""
        if not isinstance(opt, dict):
            raise TypeError("opt must be a dictionary")
        cfg = self._build_superglue_config(opt)
        super().__init__({**opt, **cfg})
        self._cfg = cfg
        self._state_dicts = {"superpoint": _load_state_dict(opt, "superpoint", ["superpoint_v1.pth"]),
                             "superglue": _load_state_dict(opt, "superglue", [f"superglue_{cfg['superglue']['weights']}.pth"])}
        self.engine   # binds (or creates) the engine that holds exactly these weights

    def _build_superglue_config(self, opt: dict) -> dict:
        """Defaults of the reference (`matchers.py:854-890`) under the caller's options, split per model."""
        o = dict(weights="outdoor", keypoint_threshold=0.001, max_keypoints=-1, match_threshold=0.3, force_cpu=False,
                 nms_radius=3, sinkhorn_iterations=20)
        o.update(opt)
        check_dict_keys(o, ["weights", "keypoint_threshold", "max_keypoints", "match_threshold", "force_cpu"])
        sp_keys, sg_keys = ("nms_radius", "keypoint_threshold", "max_keypoints"), ("weights", "sinkhorn_iterations", "match_threshold")
        return {"superpoint": {k: o[k] for k in sp_keys}, "superglue": {k: o[k] for k in sg_keys}, "force_cpu": o["force_cpu"]}

    def viz_matches(self, *args, **kwargs) -> None:
        """`matchers.py:942-1002` (SuperGlue's own plot): accepted and skipped with a warning."""
        logger.warning("viz_matches(): nothing is drawn (visualisation is out of scope of icepy4d_amd)")

    def _sp_params(self, **config):
        sp = self._cfg["superpoint"]
        return sp["nms_radius"], sp["keypoint_threshold"], 4, int(sp["max_keypoints"]), 1

    def _enqueue_cached(self, c0: dict, c1: dict, **config) -> None:
        sg = self._cfg["superglue"]
        self._load_cached_pair(c0, c1)
        self.engine.superglue(c0["shape"], c1["shape"], sg["sinkhorn_iterations"], sg["match_threshold"])

    def _match_cached(self, c0: dict, c1: dict, **config):
        self._enqueue_cached(c0, c1, **config)
        self.engine.synchronize()
        f0, f1, out = self._features_from_engine()
        matches0 = out["matches0"]
        return f0, f1, matches0, f0.scores[matches0 > -1]

    @_on_engine_device
    def _match_images(self, image0: np.ndarray, image1: np.ndarray, **config):
        """`SuperGlueMatcher._match_images` (`matchers.py:892-940`) on the GPU."""
        g0, g1 = _as_device_image(image0), _as_device_image(image1)
        sp, sg = self._cfg["superpoint"], self._cfg["superglue"]
        eng = self.engine
        unlimited = sp["max_keypoints"] < 0
        # `max_keypoints = -1` (icepy4d's default, `matchers.py:859`) keeps EVERY candidate
        # (`SuperGlue/models/superpoint.py:196-203`). The workspace is sized for opt["max_keypoints_cap"] candidates per
        # image (default 16384) and grown to the device-side candidate count whenever an image has more: extraction is then
        # repeated once, nothing is ever cut silently.
        cap = int(self._opt.get("max_keypoints_cap", 16384)) if unlimited else int(sp["max_keypoints"])
        ups = self._upload_pair(g0, g1)
        while True:
            eng.reserve(max(g0.shape[0], g1.shape[0]), max(g0.shape[1], g1.shape[1]), 2, max(cap, 1))
            n_cand = []
            for slot, up in enumerate(ups):   # one batched launch, or one per image if the sizes differ
                eng.superpoint(up, sp["nms_radius"], sp["keypoint_threshold"], 4, -1 if unlimited else cap, flavour=1, slot=slot)
                if unlimited:
                    n_cand += eng.candidates()
            if not unlimited or max(n_cand) <= eng.max_kpts:
                break
            cap = max(n_cand)
            logger.info(f"SuperPoint found {cap} candidates: growing the keypoint workspace from {eng.max_kpts}")
        eng.superglue(g0.shape[:2], g1.shape[:2], sg["sinkhorn_iterations"], sg["match_threshold"])
        (k0, d0, s0), (k1, d1, s1), out = eng.pair_to_host(0, channels_first=True, pageable=bool(self._opt.get("pageable_results", False)))    # one round of async copies, one synchronisation
        features0 = FeaturesBase(keypoints=k0, descriptors=d0, scores=s0)
        features1 = FeaturesBase(keypoints=k1, descriptors=d1, scores=s1)
        matches0 = out["matches0"]
        mconf = features0.scores[matches0 > -1]  # q5 (`matchers.py:936-938`)
        return features0, features1, matches0, mconf


class LOFTRMatcher(ImageMatcherBase):
    """The reference's kornia-hosted LoFTR matcher (`matchers.py:1005-1200`) is outside the hot-path scope (BASELINE north_star names
    SuperPoint / SuperGlue / LightGlue). The NAME exists, as in the reference's `from .matchers import *`, so that imports keep
    working; constructing one fails loudly instead of silently matching with something else."""

    def __init__(self, opt: dict = {}) -> None:
        raise NotImplementedError("LOFTRMatcher is not part of icepy4d_amd (the MI355X build covers SuperGlueMatcher and "
                                  "LightGlueMatcher); use the reference implementation for LoFTR")


class LightGlueMatcher(ImageMatcherBase):
    def __init__(self, opt: dict = {}) -> None:
        """SuperPoint + LightGlue (`matchers.py:1205-1209`). The reference rebuilds both models and reloads their
        weights inside every `_match_images` call (`:1256-1258`); here they are uploaded once."""
        self._localfeatures = opt.get("features", "superpoint")
        if self._localfeatures != "superpoint":
            raise ValueError("only features='superpoint' is supported (DISK is outside the hot-path scope)")
        super().__init__(opt)
        self._state_dicts = {"superpoint": _load_state_dict(opt, "superpoint", ["superpoint_v1.pth"]),
                             "lightglue": _load_state_dict(opt, "lightglue", ["superpoint_lightglue.pth",
                                                                              "superpoint_lightglue_v0-1_arxiv-pth"])}
        self.engine   # binds (or creates) the engine that holds exactly these weights
        self._lg_conf = {k: opt[k] for k in ("depth_confidence", "width_confidence", "filter_threshold", "pruning_min_kpts") if k in opt}

    def _sp_params(self, **config):
        if config.get("resize", None) is not None:
            return None
        return 4, 0.0005, 4, int(config.get("max_keypoints", 10240)), 0

    def _enqueue_cached(self, c0: dict, c1: dict, **config) -> None:
        self._load_cached_pair(c0, c1)
        (h0, w0), (h1, w1) = c0["shape"], c1["shape"]
        self.engine.lightglue((w0, h0), (w1, h1), **self._lg_conf)

    def _max_pairs_per_launch(self) -> int:
        return 16

    def _enqueue_cached_group(self, pairs: list, **config) -> None:
        for j, (c0, c1) in enumerate(pairs):
            self._load_cached_pair(c0, c1, pair=j)
        (h0, w0), (h1, w1) = pairs[0][0]["shape"], pairs[0][1]["shape"]
        self.engine.lightglue((w0, h0), (w1, h1), n_pairs=len(pairs), **self._lg_conf)

    def _match_cached(self, c0: dict, c1: dict, **config):
        self._enqueue_cached(c0, c1, **config)
        self.engine.synchronize()
        f0, f1, out = self._features_from_engine()
        matches0 = out["matches0"]
        self._last = out
        return f0, f1, matches0, out["matching_scores0"][matches0 > -1]

    @_on_engine_device
    def _match_images(self, image0: np.ndarray, image1: np.ndarray, **config):
        """`LightGlueMatcher._match_images` (`matchers.py:1226-1304`) on the GPU: returns
        (FeaturesBase, FeaturesBase, matches0 [K] int64, mconf [S] = scores of the valid matches)."""
        max_keypoints = config.get("max_keypoints", 10240)
        if config.get("resize", None) is not None:
            if not self._reference_quirks:
                return self._match_images_resized(image0, image1, int(config["resize"]), int(max_keypoints))
            try:
                return self._match_images_resized(image0, image1, int(config["resize"]), int(max_keypoints))
            except IcematchError:    # a library / device error (`Context.check`: out of memory, guard failure, HIP error) is not the
                raise                # resize option's failure: hiding it behind a second forward would lose the message
            except Exception as e:   # q7 (`matchers.py:1262-1267`): the reference's bare `except` calls `extract(image)` WITHOUT the option
                # (any other failure, torch's RuntimeErrors out of an unusable `resize` included, falls through to the reference's retry),
                # i.e. with the preprocessor's default resize = 1024 (`lightglue/superpoint.py:106-110, 217-227`) - not "no resize"
                logger.warning(f"extract(resize={config['resize']!r}) failed ({type(e).__name__}: {e}): retrying with the extractor's "
                               "default resize=1024, as the reference does")
                return self._match_images_resized(image0, image1, 1024, int(max_keypoints))
        g0, g1 = _as_device_image(image0), _as_device_image(image1)
        eng = self.engine
        eng.reserve(max(g0.shape[0], g1.shape[0]), max(g0.shape[1], g1.shape[1]), 2, int(max_keypoints))
        if g0.shape == g1.shape and self._opt.get("use_graph", True):
            # the ~190 launches of a pair have no host dependency: captured once per (shape, keypoint budget, matcher
            # settings) into a HIP graph and replayed on later calls (icepy4d matches the same camera pair epoch after
            # epoch). The cache lives on the ENGINE, so the fresh matcher object the reference's driver builds for every
            # epoch (`main_dev.py:115-132`) finds the graph of the previous one; entries captured before a workspace
            # re-allocation or a weight reload (engine.generation) are dropped.
            key = (g0.shape, int(max_keypoints), tuple(sorted(self._lg_conf.items())), eng.generation)
            sm = eng.graphs.get(key)
            if sm is None:
                from ..sequence import SequenceMatcher
                sm = SequenceMatcher(eng, g0.shape[0], g0.shape[1], int(max_keypoints), channels=1 if g0.ndim == 2 else 3,
                                     **self._lg_conf)
                key = key[:3] + (eng.generation,)       # the constructor may have grown the workspace
                for k in [k for k in eng.graphs if k[3] != eng.generation]:
                    del eng.graphs[k]                   # stale captures
                while len(eng.graphs) >= int(self._opt.get("max_cached_graphs", 16)):
                    del eng.graphs[next(iter(eng.graphs))]   # oldest first: a long run over many image shapes stays bounded
                sm._capture()
                eng.graphs[key] = sm
            # page-locked staging owned by the captured entry: two host copies of one image each instead of np.stack + a
            # pageable upload; the previous call has synchronised, so the buffer is free
            if getattr(sm, "_stage_in", None) is None:
                sm._stage_in = torch.empty(sm._inp.shape, dtype=torch.uint8, pin_memory=True)
            st_np = sm._stage_in.numpy()
            np.copyto(st_np[0], g0)
            np.copyto(st_np[1], g1)
            sm._inp.copy_(sm._stage_in, non_blocking=True)
            sm._graph.replay()
        else:
            for slot, up in enumerate(self._upload_pair(g0, g1)):   # one batched launch, or one per image if the sizes differ
                eng.superpoint(up, 4, 0.0005, 4, int(max_keypoints), flavour=0, slot=slot)
            eng.lightglue((g0.shape[1], g0.shape[0]), (g1.shape[1], g1.shape[0]), **self._lg_conf)
        (k0, d0, s0), (k1, d1, s1), out = eng.pair_to_host(0, channels_first=True, pageable=bool(self._opt.get("pageable_results", False)))    # one round of async copies, one synchronisation
        features0 = FeaturesBase(keypoints=k0, descriptors=d0, scores=s0)
        features1 = FeaturesBase(keypoints=k1, descriptors=d1, scores=s1)
        matches0 = out["matches0"]
        mconf = out["matching_scores0"][matches0 > -1]
        self._last = out
        return features0, features1, matches0, mconf

    def _match_images_resized(self, image0: np.ndarray, image1: np.ndarray, resize: int, max_keypoints: int):
        """`extract(image, resize=resize)` (`lightglue/superpoint.py:217-231`): the images are resized (long side = `resize`) and
        converted to gray on the HOST (kornia's algorithm restated, `_resized_gray`), extraction runs on the float gray images,
        keypoints are mapped by `(k + 0.5) / scales - 0.5` with the scales of the reference's SECOND preprocessor call (normally
        [1, 1]: they stay in the resized frame, as in the reference), `image_size` stays the original (W, H)."""
        eng = self.engine
        g, sc = zip(*(_resized_gray(im, resize) for im in (image0, image1)))
        eng.reserve(max(x.shape[0] for x in g), max(x.shape[1] for x in g), 2, max_keypoints)
        for slot in (0, 1):
            eng.superpoint(torch.from_numpy(g[slot][None]).to(eng.device), 4, 0.0005, 4, max_keypoints, flavour=0, slot=slot)
            s_ = torch.from_numpy(sc[slot]).to(eng.device)
            eng.kpts[slot] = (eng.kpts[slot] + 0.5) / s_[None, :] - 0.5
        eng.lightglue((image0.shape[1], image0.shape[0]), (image1.shape[1], image1.shape[0]), **self._lg_conf)
        self.engine.synchronize()
        f0, f1, out = self._features_from_engine()
        matches0 = out["matches0"]
        self._last = out
        return f0, f1, matches0, out["matching_scores0"][matches0 > -1]

    def _store_features(self, features0: FeaturesBase, features1: FeaturesBase, matches0: np.ndarray,
                        force_overwrite: bool = True) -> bool:
        """q1 (`matchers.py:1306-1342`): the LightGlue override ignores `matches0` and stores ALL keypoints."""
        assert isinstance(features0, FeaturesBase), "features0 must be a FeaturesBase object"
        assert isinstance(features1, FeaturesBase), "features1 must be a FeaturesBase object"
        if self._mkpts0 is not None and self._mkpts1 is not None and force_overwrite is False:
            return False
        self._mkpts0, self._mkpts1 = features0.keypoints, features1.keypoints
        if features0.descriptors is not None:
            self._descriptors0, self._descriptors1 = features0.descriptors, features1.descriptors
        if features0.scores is not None:
            self._scores0, self._scores1 = features0.scores, features1.scores
        return True
