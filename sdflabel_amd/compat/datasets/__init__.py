"""`datasets` of the reference with this directory searched first: datasets.crops resolves here, every other datasets module (kitti, ...) to
the reference's own datasets/ found on sys.path (a regular package that extends its search path, like compat/pipelines)."""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
