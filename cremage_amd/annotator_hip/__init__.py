"""ControlNet's HED annotator (modules/annotator/hed) on HIP kernels."""
from .hed import ControlNetHED_Apache2, DoubleConvBlock, HEDdetector  # noqa: F401
