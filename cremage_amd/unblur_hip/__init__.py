"""Cremage's face unblur / colorize network (modules/unblur_face) on HIP kernels."""
from .model import (ConvAct, ConvTransposeAct, MultiHeadSelfAttention, ResnetBlock, ResnetSingleBlock, ResnetSingleTransposeBlock,  # noqa: F401
                    ResnetTransposeBlock, UnblurCremageModelV6)
