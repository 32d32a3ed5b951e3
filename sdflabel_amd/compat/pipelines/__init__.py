"""`pipelines` of the reference with this directory searched first: pipelines.rotate_iou, pipelines.detection_3d and pipelines.train_css resolve here, every
other pipelines module (constants, evaluate_dump, refine_css, ...) to the reference's own pipelines/ found on sys.path.

A regular package, not a namespace portion.  `python main.py` puts the reference root ahead of every PYTHONPATH entry, and a namespace
package's search path follows sys.path order, so the reference's numba.cuda rotate_iou.py would win.  A regular package found anywhere on
sys.path takes precedence over namespace directories found before it; extend_path then appends the other `pipelines` directories on
sys.path after this one.
"""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
