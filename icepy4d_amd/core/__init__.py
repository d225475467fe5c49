"""The part of `icepy4d.core` the reconstruction needs (reference `src/icepy4d/core/camera.py`, `core/point_cloud.py`)."""
from .camera import Camera, read_opencv_calibration  # noqa: F401
from .point_cloud import PointCloud  # noqa: F401
