"""`ccw_sort_points` of the reference's `utils/geospatial.py`: what the polygon crop orders an outline with."""
import numpy as np


def ccw_sort_points(p: np.ndarray) -> np.ndarray:
    """The rows of p [n, 2] by ascending arctan2(x - mean_x, y - mean_y) around their mean (the reference's argument order and its
    unstable argsort)."""
    p = np.asarray(p)
    d = p - np.mean(p, axis=0)
    return p[np.argsort(np.arctan2(d[:, 0], d[:, 1])), :]
