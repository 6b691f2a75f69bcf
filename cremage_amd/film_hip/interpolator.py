"""FILM frame interpolation on HIP kernels - drop-in for modules/frame_interpolation_pytorch (`Interpolator` interpolator.py:87-168,
`FeatureExtractor` feature_extractor.py:82-161, `PyramidFlowEstimator` pyramid_flow_estimator.py:37-154, `Fusion` fusion.py:53-126,
`Conv2d` util.py:147-166).  Same constructor signatures, module tree and parameter names, so a `film_net` state dict loads with
strict=True.  fp32 class only (Cremage's Video Generator passes half=False): half-precision parameters raise.

Layout.  Activations are fp32 channels-last.  The two input frames run as ONE batch of 2 B samples (frame 0 first) through the image
pyramid, the siamese feature extractor and - forward flow in samples [0, B), backward flow in [B, 2 B) - the flow estimator, so every
conv is launched once for both directions.  None of the reference's torch.cat's runs: each concat is a buffer whose column slices are
written in place by the kernels of film.hip (ops.leaky_split / warp_flow / scale_into):
  * level i of the cascaded feature pyramid and of a flow predictor's input share one buffer [2 B, 2 C_i, h, w]: the sub-tree
    extractor's LeakyReLU writes columns [0, C_i) (with the 2 x 2 mean for its next level out of the same pass), the warp of the OTHER
    frame's features - a strided source view of the same buffer - writes [C_i, 2 C_i);
  * level i of the fusion's input is [warped image 0 | warped features 0 | warped image 1 | warped features 1 | dt * backward flow |
    (1 - dt) * forward flow | the coarser level's 2 x 2 conv | zero slots]: 2 (3 + C_i) + 4 columns are 2 mod 8, the fp32-class conv
    route wants a multiple of 8, so the buffer is rounded up with zeroed columns and the weight with zero columns (packed once).
  * `dt` never multiplies a flow tensor on its way to the warp: the warp takes the per-sample scalar.
Convs are `ops.conv2d` on the fp32-class route (3 x 3, 1 x 1, the thin 3 -> C and C -> 2 / 3 kernels).  The 2 x 2 conv behind the
nearest x 2 (fusion.py:84, :120-121; util.py:161-162 pads bottom / right) is that route's 3 x 3 conv with the upsampling folded into
its gather: taps embedded top-left in a zero 3 x 3 kernel, padding (0, 0, 2, 2).
Only exact pyramids are built: H and W must be multiples of 2 ** (pyramid_levels - 1), which the reference's load_image(align=64)
guarantees for the default configuration; every F.interpolate(size=level_size) is then an exact x 2.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn as nn

from .. import ops
from .._lib import CrgError

_COLOR = 3
_weights = ops.TensorKeyedCache()


def _round8(c: int) -> int:
    return (c + 7) // 8 * 8


def laid_out_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], cin: int):
    """(weight, bias) of a FILM conv in the shape the conv route takes, built once per parameter: input columns zero-padded up to the
    `cin` channels of the (zero-slotted) input buffer; a 2 x 2 kernel embedded top-left in a zero 3 x 3 one, its <= 8 output channels
    padded to 16 with zero rows (the thin-channel kernels know neither upsampling nor one-sided padding)."""
    cout, wc, ks, _ = weight.shape
    if cin < wc:
        raise CrgError(f"film conv: the input has {cin} channels, the weight expects {wc}")
    if cin == wc and ks != 2:
        return weight, bias
    r = _weights.get((weight,) if bias is None else (weight, bias), (cin,))
    if r is not None:
        return r
    with torch.no_grad():
        co = 16 if (ks == 2 and cout <= 8) else cout
        k3 = 3 if ks == 2 else ks
        w = torch.zeros((co, cin, k3, k3), dtype=weight.dtype, device=weight.device)
        w[:cout, :wc, :ks, :ks] = weight
        b = bias
        if bias is not None and co != cout:
            b = torch.zeros((co,), dtype=bias.dtype, device=bias.device)
            b[:cout] = bias
    return _weights.put((weight,) if bias is None else (weight, bias), (cin,), (w, b))


def film_conv(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], *, upsample2x: bool = False) -> torch.Tensor:
    """util.Conv2d without its activation on a dense fp32 channels-last x [N, C, H, W], C >= the weight's input channels with the surplus
    columns zero.  Kernel 1 / 3: 'same'; kernel 2: zero pad bottom / right (util.py:161-162), behind a nearest x 2 with `upsample2x`."""
    cout, ks = weight.shape[0], weight.shape[2]
    w, b = laid_out_weight(weight, bias, x.shape[1])
    if ks == 2:
        y = ops.conv2d(x, w, b, padding=(0, 0, 2, 2), upsample2x=upsample2x)
        return y if y.shape[1] == cout else y[:, :cout]
    if upsample2x:
        raise CrgError("film conv: only the 2 x 2 conv sits behind an upsampling")
    return ops.conv2d(x, w, b, padding=ks // 2)


class Conv2d(nn.Sequential):
    """util.py:147-166: [0] is the nn.Conv2d that holds the parameters, `activation` LeakyReLU(0.2) or None."""

    def __init__(self, in_channels, out_channels, size, activation: Optional[str] = "relu"):
        if activation not in (None, "relu"):
            raise ValueError(f"Conv2d: activation {activation!r} (None or 'relu', which is LeakyReLU(0.2))")
        super().__init__(nn.Conv2d(in_channels, out_channels, size))  # the parameter container; film_conv does the padding
        self.size = size
        self.activation = nn.LeakyReLU(0.2) if activation else None

    def forward(self, x, *, out=None, pool=None, upsample2x: bool = False):
        """`out`: the slice that takes the activated result (default: in place of the conv's output); `pool`: also return its 2 x 2 mean"""
        y = film_conv(x, self[0].weight, self[0].bias, upsample2x=upsample2x)
        if self.activation is None:
            if out is not None or pool:
                raise CrgError("film Conv2d: a conv without activation returns its own output")
            return y
        y, _, pooled = ops.leaky_split(y, self.activation.negative_slope, out=y if out is None else out, pool=pool)
        return (y, pooled) if pool else y


class SubTreeExtractor(nn.Module):
    def __init__(self, in_channels=3, channels=64, n_layers=4):
        super().__init__()
        widths = [in_channels] + [channels << j for j in range(n_layers)]  # stage j: two 3 x 3 convs at channels << j
        self.convs = nn.ModuleList(nn.Sequential(Conv2d(widths[j], widths[j + 1], 3), Conv2d(widths[j + 1], widths[j + 1], 3)) for j in range(n_layers))

    def forward(self, image: torch.Tensor, slices: List[torch.Tensor]) -> None:
        """Level j of the sub-tree goes to slices[j]; only the len(slices) levels somebody reads are computed (the reference runs all
        of its convs and drops the rest, feature_extractor.py:115-120, :149-160)."""
        head = image
        for j, dst in enumerate(slices):
            head = self.convs[j][0](head)
            if j + 1 < len(slices):
                _, head = self.convs[j][1](head, out=dst, pool=True)
            else:
                self.convs[j][1](head, out=dst)


class FeatureExtractor(nn.Module):
    def __init__(self, in_channels=3, channels=64, sub_levels=4):
        super().__init__()
        self.extract_sublevels = SubTreeExtractor(in_channels, channels, sub_levels)
        self.sub_levels = sub_levels
        self.channels = channels

    def level_channels(self, i: int) -> int:
        return sum(self.channels << j for j in range(min(i, self.sub_levels - 1) + 1))

    def forward(self, image_pyramid: List[torch.Tensor], buffers: List[torch.Tensor]) -> None:
        """buffers[i][:, :C_i] becomes level i of the cascaded pyramid: cat(S_i_0, S_(i-1)_1, ...) of feature_extractor.py:155-160"""
        levels = len(image_pyramid)
        for i, image in enumerate(image_pyramid):
            n = min(levels - i, self.sub_levels)
            off = [sum(self.channels << k for k in range(j)) for j in range(n)]
            self.extract_sublevels(image, [buffers[i + j][:, off[j]:off[j] + (self.channels << j)] for j in range(n)])


class FlowEstimator(nn.Module):
    def __init__(self, in_channels: int, num_convs: int, num_filters: int):
        super().__init__()
        widths = [in_channels] + [num_filters] * num_convs  # num_convs 3 x 3 convs, then 1 x 1 to half the width, then 1 x 1 to the flow
        self._convs = nn.ModuleList([Conv2d(a, b, 3) for a, b in zip(widths[:-1], widths[1:])])
        self._convs.append(Conv2d(widths[-1], num_filters // 2, 1))
        self._convs.append(Conv2d(num_filters // 2, 2, 1, activation=None))  # the flow itself: no activation

    def forward(self, net: torch.Tensor) -> torch.Tensor:
        """net: the [features_a | features_b] buffer"""
        for conv in self._convs:
            net = conv(net)
        return net


class PyramidFlowEstimator(nn.Module):
    def __init__(self, filters: int = 64, flow_convs: tuple = (3, 3, 3, 3), flow_filters: tuple = (32, 64, 128, 256)):
        super().__init__()
        # predictor i reads [features_a | features_b] of level i: twice the filters << 0 .. filters << i of the cascaded pyramid
        predictors = [FlowEstimator(2 * sum(filters << j for j in range(i + 1)), flow_convs[i], flow_filters[i]) for i in range(len(flow_convs))]
        self._predictor = predictors[-1]  # shared by every level from len(flow_convs) - 1 on
        self._predictors = nn.ModuleList(reversed(predictors[:-1]))  # the reference's order: coarse to fine

    def predictor(self, level: int) -> FlowEstimator:
        n = len(self._predictors)
        return self._predictors[n - 1 - level] if level < n else self._predictor

    def forward(self, buffers: List[torch.Tensor], channels: List[int]):
        """buffers[i]: [2 B, 2 C_i, h, w] with the features of frame 0 / frame 1 in columns [0, C_i) of samples [0, B) / [B, 2 B).
        Returns (residuals, flows), fine to coarse, forward direction in samples [0, B), backward in [B, 2 B).  `flows` is
        util.flow_pyramid_synthesis of the residuals: the very sums this loop forms (pyramid_flow_estimator.py:140, :153)."""
        levels = len(buffers)
        B = buffers[0].shape[0] // 2
        last, c = buffers[-1], channels[-1]
        ops.scale_into(last[B:, :c], out=last[:B, c:])  # coarsest level: features_b unwarped
        ops.scale_into(last[:B, :c], out=last[B:, c:])
        v = self.predictor(levels - 1)(last)
        residuals, flows = [v], [v]
        for i in range(levels - 2, -1, -1):
            buf, c = buffers[i], channels[i]
            up = ops.flow_up2_add(v)
            ops.warp_flow(buf[B:, :c], up[:B], out=buf[:B, c:])
            ops.warp_flow(buf[:B, :c], up[B:], out=buf[B:, c:])
            res = self.predictor(i)(buf)
            v = ops.flow_up2_add(v, res)
            residuals.insert(0, res)
            flows.insert(0, v)
        return residuals, flows


def aligned_width(stages: int, filters: int) -> int:
    """columns of a fusion input whose features come from `stages` sub-tree stages: two frames of (RGB + features + a 2-channel flow)"""
    return 2 * (_COLOR + 2 + sum(filters << j for j in range(stages)))


class Fusion(nn.Module):
    """fusion.py:53-126.  convs[k] serves level n_layers - 1 - k: [2 x 2 conv of the upsampled coarser result, 3 x 3 conv of
    cat(level input, that), 3 x 3 conv]; the widths follow the reference's arithmetic (:79-90) so that its state dict fits."""

    def __init__(self, n_layers=4, specialized_layers=3, filters=64):
        super().__init__()
        self.output_conv = nn.Conv2d(filters, 3, 1)
        self.convs = nn.ModuleList()
        below, skip = aligned_width(n_layers, filters), None
        for i in reversed(range(n_layers)):
            nf = filters << min(i, specialized_layers)
            self.convs.append(nn.ModuleList([Conv2d(below, nf, 2, activation=None), Conv2d(below + (skip or nf), nf, 3), Conv2d(nf, nf, 3)]))
            below, skip = nf, aligned_width(i, filters) - nf // 2

    def level_filters(self, i: int) -> int:
        return self.convs[len(self.convs) - 1 - i][0][0].out_channels

    def forward(self, pyramid: List[torch.Tensor], widths: List[int]) -> torch.Tensor:
        """pyramid[i]: the level's buffer, its first widths[i] columns written, room for the upsampled coarser level behind them"""
        if len(pyramid) != len(self.convs) + 1:
            raise ValueError(f"Fusion: {len(pyramid)} pyramid levels for {len(self.convs)} decoder levels")
        net = pyramid[-1]
        for k, layers in enumerate(self.convs):
            i = len(self.convs) - 1 - k
            up = layers[0](net, upsample2x=True)
            ops.scale_into(up, out=pyramid[i][:, widths[i]:widths[i] + up.shape[1]])
            net = layers[2](layers[1](pyramid[i]))
        return film_conv(net, self.output_conv.weight, self.output_conv.bias)


class Interpolator(nn.Module):
    def __init__(self, pyramid_levels=7, fusion_pyramid_levels=5, specialized_levels=3, sub_levels=4, filters=64, flow_convs=(3, 3, 3, 3),
                 flow_filters=(32, 64, 128, 256)):
        super().__init__()
        if fusion_pyramid_levels != sub_levels + 1 or fusion_pyramid_levels > pyramid_levels:
            raise NotImplementedError(f"Interpolator: the fusion decoder has sub_levels = {sub_levels} levels and reads sub_levels + 1 pyramid levels "
                                      f"(fusion.py:79-90, :112-124); fusion_pyramid_levels = {fusion_pyramid_levels} of {pyramid_levels} is not restated")
        if len(flow_convs) != len(flow_filters) or not 1 <= len(flow_convs) <= pyramid_levels or sub_levels > len(flow_convs):
            raise NotImplementedError(f"Interpolator: flow_convs {flow_convs!r} / flow_filters {flow_filters!r} do not describe one predictor per "
                                      f"specialised level of a {pyramid_levels}-level pyramid with {sub_levels} sub-levels")
        if filters % 8:
            raise NotImplementedError(f"Interpolator: filters = {filters} (a multiple of 8 is built)")
        self.pyramid_levels = pyramid_levels
        self.fusion_pyramid_levels = fusion_pyramid_levels
        self.extract = FeatureExtractor(3, filters, sub_levels)
        self.predict_flow = PyramidFlowEstimator(filters, flow_convs, flow_filters)
        self.fuse = Fusion(sub_levels, specialized_levels, filters)

    def half(self):
        raise NotImplementedError("Interpolator: fp32 class only (the Video Generator passes half=False)")

    def bfloat16(self):
        raise NotImplementedError("Interpolator: fp32 class only (the Video Generator passes half=False)")

    @property
    def align(self) -> int:
        return 1 << (self.pyramid_levels - 1)

    def _check(self, x0, x1, batch_dt):
        for p in self.parameters():
            if p.dtype != torch.float32:
                raise NotImplementedError(f"Interpolator: {p.dtype} parameters - fp32 class only (the Video Generator passes half=False)")
        if x0.dim() != 4 or x0.shape != x1.shape or x0.shape[1] != _COLOR:
            raise CrgError(f"Interpolator: two [B, 3, H, W] frames expected, got {tuple(x0.shape)} and {tuple(x1.shape)}")
        if x0.dtype != torch.float32 or x1.dtype != torch.float32:
            raise NotImplementedError(f"Interpolator: {x0.dtype} frames - fp32 class only")
        B, _, H, W = x0.shape
        if H % self.align or W % self.align:
            raise CrgError(f"Interpolator: {H} x {W} frames - height and width must be multiples of 2 ** (pyramid_levels - 1) = {self.align} "
                           "(pipeline.interpolate_frames pads as the reference's load_image does)")
        if batch_dt.numel() != B:
            raise CrgError(f"Interpolator: batch_dt must be [B, 1] = [{B}, 1], got {tuple(batch_dt.shape)}")

    def _run(self, x0, x1, batch_dt):
        self._check(x0, x1, batch_dt)
        B, _, H, W = x0.shape
        dev, L, FL = x0.device, self.pyramid_levels, self.fusion_pyramid_levels
        dt = batch_dt.detach().to(device=dev, dtype=torch.float32).reshape(B)
        one_minus = 1 - dt
        images = [ops.nchw_to_nhwc(torch.cat([x0, x1], 0), torch.float32)]
        for _ in range(L - 1):
            images.append(ops.avg_pool2(images[-1]))
        chans = [self.extract.level_channels(i) for i in range(L)]
        feats = [ops.empty_image(2 * B, 2 * chans[i], H >> i, W >> i, torch.float32, dev) for i in range(L)]
        self.extract(images, feats)
        residuals, flows = self.predict_flow(feats, chans)

        # the fusion's input (interpolator.py:138-157): image 0 and its features warped by dt * backward flow, image 1 and its
        # features by (1 - dt) * forward flow, then the two scaled flows
        pyramid, widths = [], []
        for i in range(FL):
            c, width = chans[i], 2 * (_COLOR + chans[i]) + 4
            room = self.fuse.level_filters(i) if i < FL - 1 else 0
            buf = ops.empty_image(B, _round8(width + room), H >> i, W >> i, torch.float32, dev)
            if buf.shape[1] > width + room:
                buf[:, width + room:].zero_()
            fwd, bwd = flows[i][:B], flows[i][B:]
            ops.warp_flow(images[i][:B], bwd, dt, out=buf[:, 0:_COLOR])
            ops.warp_flow(feats[i][:B, :c], bwd, dt, out=buf[:, _COLOR:_COLOR + c])
            ops.warp_flow(images[i][B:], fwd, one_minus, out=buf[:, _COLOR + c:2 * _COLOR + c])
            ops.warp_flow(feats[i][B:, :c], fwd, one_minus, out=buf[:, 2 * _COLOR + c:width - 4])
            ops.scale_into(bwd, dt, out=buf[:, width - 4:width - 2])
            ops.scale_into(fwd, one_minus, out=buf[:, width - 2:width])
            pyramid.append(buf)
            widths.append(width)
        return self.fuse(pyramid, widths), residuals, flows

    @torch.no_grad()
    def debug_forward(self, x0, x1, batch_dt) -> Dict[str, List[torch.Tensor]]:
        image, residuals, flows = self._run(x0, x1, batch_dt)
        B = x0.shape[0]
        nchw = lambda t: ops.nhwc_to_nchw(t, torch.float32)  # noqa: E731
        return {
            "image": [nchw(image)],
            "forward_residual_flow_pyramid": [nchw(r[:B]) for r in residuals],
            "backward_residual_flow_pyramid": [nchw(r[B:]) for r in residuals],
            "forward_flow_pyramid": [nchw(f[:B]) for f in flows[:self.fusion_pyramid_levels]],
            "backward_flow_pyramid": [nchw(f[B:]) for f in flows[:self.fusion_pyramid_levels]],
        }

    @torch.no_grad()
    def forward(self, x0, x1, batch_dt) -> torch.Tensor:
        return ops.nhwc_to_nchw(self._run(x0, x1, batch_dt)[0], torch.float32)
