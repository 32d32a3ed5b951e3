"""pipelines/detection_3d.py of the reference (numba CPU JIT + scipy there) on sdflabel_amd.pipelines.detection_3d: same names and results.

The package next to this file (__init__.py) makes pipelines.detection_3d resolve here, whichever of the two `pipelines` directories comes
first on sys.path, so `from pipelines.detection_3d import Detection3DEvaluator, clean_kitti_data, CoordinateFrame` of the reference's
evaluate_dump.py and refine_css.py gets the device evaluator.  pipelines.constants still resolves to the reference's file, which holds the
default threshold tables.  Imports neither numba, scipy nor mpi4py; without a GPU the evaluator raises SdfrError.
"""
from sdflabel_amd.pipelines.detection_3d import (CoordinateFrame, Detection3DEvaluator, Metrics, angle_diff, clean_kitti_data,  # noqa: F401
                                                 difficulty_by_distance, get_thresholds)
