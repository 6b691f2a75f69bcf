"""ControlNet's HED edge detector on HIP kernels - drop-ins for modules/annotator/hed/__init__.py (`DoubleConvBlock` :17-33,
`ControlNetHED_Apache2` :36-53, `HEDdetector` :56-78).  Same constructor signatures, module tree and parameter names (`norm`,
`blockK.convs.J.{weight,bias}`, `blockK.projection.{weight,bias}`: 37 keys, 14 716 168 parameters), so ControlNetHED.pth loads with
strict=True.  fp32 class only, as the reference runs it (`.float()`, :63).

Layout.  The network is a VGG-16 trunk: 13 3 x 3 convs with ReLU, four 2 x 2 max pools, five 1 x 1 projections to one channel.
  * block1.convs.0 has 3 input channels: the thin-channel conv (`crg_conv_small`) on the fp32 image.
  * Every other 3 x 3 conv is the fp32-class conv on the (hi, lo) half-type planes of its input.
  * Everything between two convs is ONE launch of `ops.relu_pool_proj` on the conv's fp32 output: inside a block it writes the planes of
    relu(h) for the next conv; behind a block's last conv it writes the planes of maxpool2x2(relu(h)) - the next block's operand - and the
    block's projection of relu(h).  No ReLU'd, pooled or concatenated fp32 tensor exists; the conv output is read once.
  * `x - norm` on the 3-channel input is a torch operation (3 of the network's 5 000 channel planes), as is the cast of the bytes.
A `DoubleConvBlock` called on its own with down_sampling=True pools an arbitrary input, which no kernel here does (inside the network the
pool is fused behind the previous block's ReLU): that entry uses F.max_pool2d and says so.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from .._lib import CrgError

Planes = Tuple[torch.Tensor, torch.Tensor]


def _fp32_only(module: torch.nn.Module, what: str) -> None:
    for p in module.parameters():
        if p.dtype != torch.float32:
            raise NotImplementedError(f"{what}: {p.dtype} parameters - fp32 class only (the reference runs this network in fp32)")


def _image(x: torch.Tensor, channels: int, what: str) -> torch.Tensor:
    if x.dim() != 4 or x.dtype != torch.float32 or x.shape[1] != channels:
        raise CrgError(f"{what}: a float32 [N, {channels}, H, W] image expected, got {tuple(x.shape)} {x.dtype}")
    if not x.is_cuda:
        raise CrgError(f"{what}: the image must live on a HIP device (no CPU fallback exists)")
    return ops.to_channels_last(x)


class DoubleConvBlock(torch.nn.Module):
    """hed/__init__.py:17-33"""

    def __init__(self, input_channel, output_channel, layer_number):
        super().__init__()
        self.convs = torch.nn.Sequential()
        self.convs.append(torch.nn.Conv2d(in_channels=input_channel, out_channels=output_channel, kernel_size=(3, 3), stride=(1, 1), padding=1))
        for i in range(1, layer_number):
            self.convs.append(torch.nn.Conv2d(in_channels=output_channel, out_channels=output_channel, kernel_size=(3, 3), stride=(1, 1), padding=1))
        self.projection = torch.nn.Conv2d(in_channels=output_channel, out_channels=1, kernel_size=(1, 1), stride=(1, 1), padding=0)

    def run(self, x: Optional[torch.Tensor], planes: Optional[Planes], pool: bool = False, keep: bool = False):
        """The block on its operand - the fp32 channels-last image `x` where the first conv is the thin-channel one (<= 8 input channels),
        else the (hi, lo) planes.  Returns (pooled planes of the block's output or None, projection [N, 1, H, W], the last conv's fp32
        output before the ReLU if `keep`)."""
        last = len(self.convs) - 1
        pooled = proj = h = None
        for i, conv in enumerate(self.convs):
            if planes is None:
                h = ops.conv2d(x, conv.weight, conv.bias, padding=1)
            else:
                h = ops.conv2d(planes[0], conv.weight, conv.bias, padding=1, x_lo=planes[1])
            if i < last:
                planes, _, _ = ops.relu_pool_proj(h, planes=True)
            else:
                _, pooled, proj = ops.relu_pool_proj(h, pool=True if pool else None, proj=(self.projection.weight, self.projection.bias))
        return pooled, proj, (h if keep else None)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, down_sampling: bool = False):
        """The reference's call: (relu'd output of the last conv, projection), both fp32 [N, C, H, W].  Pooling an arbitrary input is
        F.max_pool2d here (see the module docstring); the ReLU'd output is `ops.leaky_split(slope=0)` of the conv output."""
        _fp32_only(self, "DoubleConvBlock")
        cin = self.convs[0].in_channels
        x = _image(x, cin, "DoubleConvBlock")
        if down_sampling:
            if min(x.shape[2:]) < 2:
                raise CrgError(f"DoubleConvBlock: a {x.shape[2]} x {x.shape[3]} image has no 2 x 2 window")
            x = ops.to_channels_last(F.max_pool2d(x, kernel_size=(2, 2), stride=(2, 2)))
        thin = cin <= 8
        _, proj, h = self.run(x if thin else None, None if thin else ops.split_bf16(x), keep=True)
        return ops.leaky_split(h, 0.0)[0], proj


class ControlNetHED_Apache2(torch.nn.Module):
    """hed/__init__.py:36-53.  forward(x): x float32 [N, 3, H, W] with values 0 .. 255 on the device; returns the five projections, fp32
    [N, 1, H / 2^k, W / 2^k] (floor), k = 0 .. 4."""

    def __init__(self):
        super().__init__()
        self.norm = torch.nn.Parameter(torch.zeros(size=(1, 3, 1, 1)))
        self.block1 = DoubleConvBlock(input_channel=3, output_channel=64, layer_number=2)
        self.block2 = DoubleConvBlock(input_channel=64, output_channel=128, layer_number=2)
        self.block3 = DoubleConvBlock(input_channel=128, output_channel=256, layer_number=3)
        self.block4 = DoubleConvBlock(input_channel=256, output_channel=512, layer_number=3)
        self.block5 = DoubleConvBlock(input_channel=512, output_channel=512, layer_number=3)

    def half(self):
        raise NotImplementedError("ControlNetHED_Apache2: fp32 class only (the reference runs this network in fp32)")

    def bfloat16(self):
        raise NotImplementedError("ControlNetHED_Apache2: fp32 class only (the reference runs this network in fp32)")

    @torch.no_grad()
    def forward(self, x: torch.Tensor):
        _fp32_only(self, "ControlNetHED_Apache2")
        if x.dim() != 4 or x.dtype != torch.float32 or x.shape[1] != 3 or not x.is_cuda:
            raise CrgError(f"ControlNetHED_Apache2: a float32 [N, 3, H, W] image on the device expected, got {tuple(x.shape)} {x.dtype} on {x.device}")
        if min(x.shape[2:]) < 16:
            raise CrgError(f"ControlNetHED_Apache2: a {x.shape[2]} x {x.shape[3]} image leaves block5 an empty grid (four 2 x 2 pools: both edges >= 16)")
        h = ops.to_channels_last(x - self.norm)
        projections: List[torch.Tensor] = []
        planes = None
        blocks = [self.block1, self.block2, self.block3, self.block4, self.block5]
        for k, block in enumerate(blocks):
            planes, proj, _ = block.run(h if k == 0 else None, planes, pool=k < 4)
            projections.append(proj)
        return tuple(projections)


class HEDdetector:
    """hed/__init__.py:56-78 around a given network (the reference's constructor downloads ControlNetHED.pth; here the caller loads it).
    detector(image): image uint8 [H, W, 3] - a numpy array, or with glue="device" also a device tensor - to the uint8 edge map [H, W].
    glue="host" (default): the five projections are downloaded and fused by postprocess.hed_fuse_host, a numpy array is returned.
    glue="device": one launch of ops.hed_fuse, the edge map stays on the device (a uint8 tensor) - the same bytes."""

    def __init__(self, model: ControlNetHED_Apache2, glue: str = "host"):
        if glue not in ("host", "device"):
            raise ValueError(f"HEDdetector: glue must be 'host' or 'device', got {glue!r}")
        self.netNetwork = model.eval()
        self.glue = glue

    @torch.no_grad()
    def projections(self, input_image):
        """the five projections [1, 1, h, w] on the device"""
        dev = next(self.netNetwork.parameters()).device
        if isinstance(input_image, np.ndarray):
            input_image = torch.from_numpy(input_image.copy()).to(dev)  # (:70: a copy - the wrapper hands over a flipped, read-only view)
        if input_image.dim() != 3 or input_image.shape[2] != 3 or input_image.dtype != torch.uint8:
            raise CrgError(f"HEDdetector: a uint8 [H, W, 3] image expected, got {tuple(input_image.shape)} {input_image.dtype}")
        x = input_image.to(dev).permute(2, 0, 1)[None].float()  # 'h w c -> 1 c h w' (:70-71)
        return self.netNetwork(x)

    @torch.no_grad()
    def __call__(self, input_image, glue: Optional[str] = None):
        glue = self.glue if glue is None else glue
        if glue not in ("host", "device"):
            raise ValueError(f"HEDdetector: glue must be 'host' or 'device', got {glue!r}")
        if glue == "host" and not isinstance(input_image, np.ndarray):
            raise CrgError("HEDdetector: a device tensor needs glue='device'")
        H, W = int(input_image.shape[0]), int(input_image.shape[1])
        edges = self.projections(input_image)
        if glue == "device":
            return ops.hed_fuse(edges, (H, W))[0]
        from ..postprocess import hed_fuse_host
        return hed_fuse_host([e.detach().cpu().numpy().astype(np.float32)[0, 0] for e in edges], (H, W))
