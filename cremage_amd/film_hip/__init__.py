"""FILM frame interpolation (modules/frame_interpolation_pytorch) on HIP kernels."""
from .interpolator import Interpolator  # noqa: F401
