"""kimimaro_amd -- MI355X-native TEASAR skeletonization (the hot path of seung-lab/kimimaro).

Public names follow kimimaro/__init__.py:18-25 for the part that is in scope.
Importing the package never touches the GPU; calling skeletonize() without libkimi_hip.so + an
MI355X raises HipUnavailableError (there is deliberately no CPU fallback).
"""
import os as _os

# one hardware queue per stream of the lanes (kimimaro_amd/lanes.py): the HIP runtime reads this once, at its first call
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")

from ._abi import HipUnavailableError, KimiHipError  # noqa: F401
from .intake import DEFAULT_TEASAR_PARAMS, DimensionError, connect_points, skeletonize, synapses_to_targets  # noqa: F401
from .lanes import skeletonize_many  # noqa: F401
from .ops import voxel_connectivity_graph  # noqa: F401
from .post import (components_many, cross_sectional_area_chunked, cross_sectional_area_filled_chunked, fill_all_holes_chunked,  # noqa: F401
                   join_close_components, join_close_components_many, oversegment_chunked, paths_many, postprocess, postprocess_many,
                   remove_dust_many, remove_loops_many, remove_ticks_many, skeletonize_chunked, skeletonize_graph_chunked,
                   synapses_to_targets_chunked, voxel_connectivity_graph_chunked)
from .skeleton import Skeleton  # noqa: F401
from .utility import (cross_sectional_area, cross_sectional_area_filled, cross_sectional_area_single,  # noqa: F401
                      extract_skeleton_from_binary_image, oversegment)

__version__ = "0.1.0"
