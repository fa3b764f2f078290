"""sfmx — MI355X-native SfM matching + bundle-adjustment hot path.

Python host layer over the C ABI in ``include/sfmx.h`` (libsfmx.so).  The
package directory is ``sfm-mvs-pipeline_amd/``; add it to ``sys.path`` and
``import sfmx``.
"""
from . import _lib  # noqa: F401  (fails loudly if libsfmx.so is missing)
from .matching import (  # noqa: F401
    BFMatcher, NORM_L2, NORM_HAMMING, LOWE_RATIO, DMATCH_DTYPE, Scene, Shot, ShotMatches,
    IFeatureMatchingStrategy, UnorderedFeatureMatchingStrategy, VideoFeatureMatchingStrategy,
    GridFeatureMatchingStrategy, calculate_shot_matches, match_pairs, pairs_unordered, pairs_video, pairs_grid,
)

from . import homography, scene, mvs, features, triangulate, pose, pnp, cloud, report, sfm  # noqa: F401,E402
from .report import (  # noqa: F401,E402
    reprojection_errors, reprojection_errors_device, colorize_pointcloud, colorize_pointcloud_device,
    writeToReprojectionErrorStatisticsCSV, writeToReprojectionErrorHistogramCSV, colorizePointcloud, writeToPLY,
)
from .triangulate import triangulate_matches, triangulate_matches_device, triangulateMatch  # noqa: F401,E402
from .pose import relative_poses, relative_poses_device, findCameraPoseFromMatch  # noqa: F401,E402
from .pnp import (  # noqa: F401,E402
    register_poses, register_poses_device, distinct_3d2d_points, distinct_3d2d_points_device,
    findCameraPoseFrom3d2dMatch,
)
from .scene import merge_pointcloud_3d2d  # noqa: F401,E402

__version__ = "0.1.0"
