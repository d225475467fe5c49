from .timer import AverageTimer, timeit  # noqa: F401
from . import binned_stats, geospatial, homography, point_cloud_filters, tracking_features_utils, transformations  # noqa: F401,E402
