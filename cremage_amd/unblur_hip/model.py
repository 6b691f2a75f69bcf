"""Cremage's face unblur / colorize network on HIP kernels - drop-ins for modules/unblur_face (`MultiHeadSelfAttention` mha.py:15-83;
`ResnetSingleBlock`, `ResnetSingleTransposeBlock`, `ResnetBlock`, `ResnetTransposeBlock`, `ConvAct`, `ConvTransposeAct`,
`UnblurCremageModelV6` cremage_model_v6.py:15-504).  Same constructor signatures, module tree and parameter names, so the reference's
sd['model_state_dict'] loads with strict=True; the same class serves the Unblur and the Colorize button with two weight files.  fp32 class
only, as the reference runs it: half-precision parameters raise.

Layout.  An activation travels as (x, planes): x the fp32 channels-last image, planes = (hi, lo) the two half-type planes the fp32-class
convs read.  Both come out of ONE pass: the tail of every single block, y = SiLU(GN2(conv2) + skip) (:94-98, :194-198), is
`ops.group_norm_add_act`, which writes y - the next block's identity skip - and its planes; gn1 + act1 is the same kernel without skip
writing planes alone (nothing reads that fp32 tensor).  Where the producing conv handed over a GroupNorm statistics side channel the
kernel folds it instead of reading the tensor for statistics.
  * ConvTranspose2d(4, 2, 1) - conv1 and conv_skip of every up level's first block, and ConvTransposeAct - is `ops.conv_transpose2d`.
  * None of the up path's torch.concat([x, h[i]]) runs (:501): the concat only ever feeds two transposed convs, which read planes, so
    it exists as one pair of plane buffers; the previous up block writes its planes into columns [0, Cx), the down tap's are copied
    behind them.
  * The first layer has 3 channels and stride 2: the input is laid out once as 16 zero-slotted channels, the weights of
    down_blocks.0.blocks.0 get zero columns (packed once); 16, not 8, because convs of <= 8 input channels belong to the thin-channel
    kernel, which is stride 1 only.
  * ConvAct: the 2 x 2 'valid' conv on the 2 x 2 image is a `linear` over [B, 4 Cin] with the weight laid out once as [Cout, (kh, kw, ci)];
    the 1 x 1 convs are `linear` over the tokens.
  * Attention: q / k / out are fp32-class `ops.linear`, V comes out transposed (`ops.linear_transposed`), the core is
    `ops.attention(..., flash=True)`.  Its output REPLACES x - there is no residual (:242-246).
Quirks kept: min(32, C) groups; 28 groups at 112 channels in the transposed blocks (:155-157); no concat for up blocks 0 and 8.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from .. import ops
from .._lib import CrgError

_weights = ops.TensorKeyedCache()
_FIRST_SLOTS = 16  # channels of the zero-slotted network input
Planes = Tuple[torch.Tensor, torch.Tensor]


def _fp32_only(module: nn.Module, what: str) -> None:
    for p in module.parameters():
        if p.dtype != torch.float32:
            raise NotImplementedError(f"{what}: {p.dtype} parameters - fp32 class only (the reference runs this network in fp32)")


def _slotted_weight(weight: torch.Tensor, cin: int) -> torch.Tensor:
    """a conv weight whose input columns are zero-padded up to the `cin` channels of a zero-slotted input, built once per parameter"""
    if weight.shape[1] == cin:
        return weight
    r = _weights.get((weight,), ("slots", cin))
    if r is None:
        with torch.no_grad():
            w = torch.zeros((weight.shape[0], cin) + tuple(weight.shape[2:]), dtype=weight.dtype, device=weight.device)
            w[:, :weight.shape[1]] = weight
        r = _weights.put((weight,), ("slots", cin), w)
    return r


def _valid_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, k, k] -> [Cout, (kh, kw, ci)]: the matrix of a 'valid' k x k conv on a k x k channels-last image, built once"""
    r = _weights.get((weight,), ("valid",))
    if r is None:
        r = _weights.put((weight,), ("valid",), weight.detach().permute(0, 2, 3, 1).reshape(weight.shape[0], -1).contiguous())
    return r


def _image(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() != 4 or x.dtype != torch.float32:
        raise CrgError(f"{what}: a [B, C, H, W] float32 image expected, got {tuple(x.shape)} {x.dtype}")
    return ops.to_channels_last(x)


def _slot_input(x: torch.Tensor) -> torch.Tensor:
    """x (channels-last) with zero channels appended up to the multiple-of-8 width the conv route takes (3 -> 16)"""
    c = x.shape[1]
    if c % 8 == 0 and c > 8:
        return x
    slots = max(_FIRST_SLOTS, (c + 7) // 8 * 8)
    buf = ops.empty_image(x.shape[0], slots, x.shape[2], x.shape[3], torch.float32, x.device)
    buf[:, c:].zero_()
    ops.scale_into(x, out=buf[:, :c])
    return buf


def _groups(c: int, transposed: bool) -> int:
    return 28 if (transposed and c == 112) else min(32, c)  # cremage_model_v6.py:56-57, :152-157


class MultiHeadSelfAttention(nn.Module):
    """mha.py:15-83.  forward(q, k, v) on [B, T, C] tokens; the network only ever calls it with q is k is v."""

    def __init__(self, embed_size: int, heads: int):
        super().__init__()
        self.embed_size = embed_size
        self.heads = heads
        self.head_dim = embed_size // heads
        assert self.head_dim * heads == embed_size, "Embedding size must be divisible by heads"
        self.values = nn.Linear(embed_size, embed_size, bias=False)
        self.keys = nn.Linear(embed_size, embed_size, bias=False)
        self.queries = nn.Linear(embed_size, embed_size, bias=False)
        self.out = nn.Linear(embed_size, embed_size)

    @torch.no_grad()
    def forward(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        _fp32_only(self, "MultiHeadSelfAttention")
        for t in (q, k, v):
            if t.dim() != 3 or t.dtype != torch.float32 or t.shape[2] != self.embed_size:
                raise CrgError(f"MultiHeadSelfAttention: float32 [B, T, {self.embed_size}] tokens expected, got {tuple(t.shape)} {t.dtype}")
        if k.shape[1] != v.shape[1] or q.shape[0] != k.shape[0] or q.shape[0] != v.shape[0]:
            raise CrgError("MultiHeadSelfAttention: k and v must hold the same tokens, all three the same batch")
        qq = ops.linear(q.contiguous(), self.queries.weight)
        kk = ops.linear(k.contiguous(), self.keys.weight)
        vt = ops.linear_transposed(v.contiguous(), self.values.weight)
        o = ops.attention(qq, kk, vt, self.heads, k.shape[1], self.head_dim ** -0.5, flash=True)
        return ops.linear(o, self.out.weight, self.out.bias)


class _SingleBase(nn.Module):
    """what ResnetSingleBlock and ResnetSingleTransposeBlock share: gn1 + act1, conv2, the fused tail"""
    transposed = False

    def _norms(self, out_channels: int, num_groups: int):
        g = min(num_groups, out_channels)
        if self.transposed and out_channels == 112:
            g = 28
        self.gn1 = nn.GroupNorm(g, out_channels)
        self.gn2 = nn.GroupNorm(g, out_channels)
        self.act1 = nn.SiLU()
        self.act2 = nn.SiLU()

    def _initialize_weights(self):
        if self.conv_skip is not None:
            nn.init.xavier_uniform_(self.conv_skip.weight)
        nn.init.xavier_uniform_(self.conv1.weight)
        nn.init.xavier_uniform_(self.conv2.weight)

    def _heads(self, x: Optional[torch.Tensor], planes: Planes):
        """(conv1 output, skip) - the two things the subclasses do differently"""
        raise NotImplementedError

    def run(self, x: Optional[torch.Tensor], planes: Planes, out_planes=True, fp32: bool = True):
        """x: the fp32 image (needed only where the skip is the identity), planes: its (hi, lo).  Returns (y, planes of y); `out_planes`
        may name two destinations (column slices of a concat buffer), `fp32=False` skips the fp32 image."""
        h, skip = self._heads(x, planes)
        _, hp = ops.group_norm_add_act(h, self.gn1.weight, self.gn1.bias, self.gn1.num_groups, self.gn1.eps, silu=True, planes=True, fp32=False)
        h = ops.conv2d(hp[0], self.conv2.weight, None, padding=1, x_lo=hp[1], gn_stats=True)
        return ops.group_norm_add_act(h, self.gn2.weight, self.gn2.bias, self.gn2.num_groups, self.gn2.eps, skip=skip, silu=True, planes=out_planes, fp32=fp32)

    @torch.no_grad()
    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        _fp32_only(self, type(self).__name__)
        x = _image(inputs, type(self).__name__)
        xs = _slot_input(x)
        return self.run(xs, ops.split_bf16(xs))[0]


class ResnetSingleBlock(_SingleBase):
    """cremage_model_v6.py:15-98"""

    def __init__(self, in_channels, out_channels, stride=1, num_groups=32):
        super().__init__()
        self.conv_skip = None
        if stride == 2 or in_channels != out_channels:
            self.conv_skip = nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=stride, bias=False)
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=False)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False)
        self.stride = stride
        self._norms(out_channels, num_groups)
        self._initialize_weights()

    def _heads(self, x, planes):
        hi, lo = planes
        cin = hi.shape[1]
        skip = x
        if self.conv_skip is not None:
            skip = ops.conv2d(hi, _slotted_weight(self.conv_skip.weight, cin), None, stride=self.stride, padding=0, x_lo=lo)
        elif x is None:
            raise CrgError("ResnetSingleBlock: an identity skip needs the fp32 image")
        return ops.conv2d(hi, _slotted_weight(self.conv1.weight, cin), None, stride=self.stride, padding=1, x_lo=lo, gn_stats=True), skip


class ResnetSingleTransposeBlock(_SingleBase):
    """cremage_model_v6.py:101-199: with in_channels > out_channels conv1 and conv_skip are ConvTranspose2d(4, 2, 1), else conv1 is a 3 x 3
    conv and the skip the identity"""
    transposed = True

    def __init__(self, in_channels, out_channels, stride=1, num_groups=32):
        super().__init__()
        self.conv_skip = None
        if in_channels > out_channels:
            self.conv_skip = nn.ConvTranspose2d(in_channels, out_channels, kernel_size=4, stride=2, bias=False, padding=1)
            self.conv1 = nn.ConvTranspose2d(in_channels, out_channels, kernel_size=4, stride=2, bias=False, padding=1)
        else:
            self.conv1 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False)
        self._norms(out_channels, num_groups)
        self._initialize_weights()

    def _heads(self, x, planes):
        hi, lo = planes
        if self.conv_skip is not None:
            return ops.conv_transpose2d(hi, lo, self.conv1.weight), ops.conv_transpose2d(hi, lo, self.conv_skip.weight)
        if x is None:
            raise CrgError("ResnetSingleTransposeBlock: an identity skip needs the fp32 image")
        return ops.conv2d(hi, self.conv1.weight, None, padding=1, x_lo=lo, gn_stats=True), x


class _BlockBase(nn.Module):
    single = ResnetSingleBlock

    def __init__(self, in_channels, out_channels, stride=1, num_blocks=6, heads=8):
        super().__init__()
        self.blocks = nn.ModuleList()
        self.attentions = nn.ModuleList()
        self.blocks.append(self.single(in_channels, out_channels, stride=stride))
        for _ in range(num_blocks - 1):
            self.blocks.append(self.single(out_channels, out_channels, stride=1))
        if heads > 0:  # one attention behind the single blocks
            self.attentions.append(MultiHeadSelfAttention(out_channels, heads))

    def run(self, x: Optional[torch.Tensor], planes: Planes, out_planes=True):
        """Returns (y, planes of y); out_planes: True or two destinations"""
        last = len(self.blocks) - 1
        attend = len(self.attentions) > 0
        for i, block in enumerate(self.blocks):
            x, planes = block.run(x, planes, out_planes=out_planes if (i == last and not attend) else True)
        if attend:
            n, c, h, w = x.shape
            t = ops.tokens_of(x)
            x = ops.image_of(self.attentions[0](t, t, t), h, w)  # replaces x: no residual (:242-246)
            _, planes, _ = ops.leaky_split(x, 1.0, fp32=False, planes=out_planes)
        return x, planes

    @torch.no_grad()
    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        _fp32_only(self, type(self).__name__)
        x = _image(inputs, type(self).__name__)
        xs = _slot_input(x)
        return self.run(xs, ops.split_bf16(xs))[0]


class ResnetBlock(_BlockBase):
    """cremage_model_v6.py:202-248"""
    single = ResnetSingleBlock


class ResnetTransposeBlock(_BlockBase):
    """cremage_model_v6.py:250-292"""
    single = ResnetSingleTransposeBlock


class ConvAct(nn.Module):
    """cremage_model_v6.py:295-344: Conv2d + SiLU.  The network has it as 1 x 1 convs and as the 2 x 2 'valid' conv on the 2 x 2 image; both
    are one `linear` with the SiLU in its epilogue.  Anything else is not restated."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, **kwargs):
        super().__init__(**kwargs)
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding)
        self.act = nn.SiLU()
        nn.init.xavier_uniform_(self.conv.weight)

    def run(self, x: torch.Tensor) -> torch.Tensor:
        n, c, h, w = x.shape
        k = self.conv.kernel_size[0]
        if self.conv.kernel_size != (k, k) or self.conv.padding != (0, 0) or (k > 1 and (h, w) != (k, k)) or (k == 1 and self.conv.stride != (1, 1)):
            raise NotImplementedError(f"ConvAct: kernel {self.conv.kernel_size} stride {self.conv.stride} padding {self.conv.padding} on a {h} x {w} image "
                                      "(built: 1 x 1 convs, and a k x k conv without padding on a k x k image)")
        if k == 1:
            return ops.image_of(ops.linear(ops.tokens_of(x), self.conv.weight, self.conv.bias, act="silu"), h, w)
        y = ops.linear(ops.tokens_of(x).reshape(n, 1, h * w * c), _valid_weight(self.conv.weight), self.conv.bias, act="silu")
        return ops.image_of(y, 1, 1)

    @torch.no_grad()
    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        _fp32_only(self, "ConvAct")
        return self.run(_image(inputs, "ConvAct"))


class ConvTransposeAct(nn.Module):
    """cremage_model_v6.py:347-397: ConvTranspose2d(4, 2, 1) + SiLU, bias and activation in the kernel's epilogue"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, **kwargs):
        super().__init__(**kwargs)
        self.conv = nn.ConvTranspose2d(in_channels, out_channels, kernel_size, stride, padding)
        self.act = nn.SiLU()
        nn.init.xavier_uniform_(self.conv.weight)

    def run(self, planes: Planes) -> torch.Tensor:
        if self.conv.kernel_size != (4, 4) or self.conv.stride != (2, 2) or self.conv.padding != (1, 1):
            raise NotImplementedError(f"ConvTransposeAct: kernel {self.conv.kernel_size} stride {self.conv.stride} padding {self.conv.padding} (built: 4 / 2 / 1)")
        return ops.conv_transpose2d(planes[0], planes[1], self.conv.weight, self.conv.bias, silu=True)

    @torch.no_grad()
    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        _fp32_only(self, "ConvTransposeAct")
        return self.run(ops.split_bf16(_image(inputs, "ConvTransposeAct")))


class UnblurCremageModelV6(nn.Module):
    """cremage_model_v6.py:400-504"""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.down_blocks = nn.ModuleList()
        self.mid_blocks = nn.ModuleList()
        self.up_blocks = nn.ModuleList()
        ns = [3, 16, 32, 64, 128, 256, 512, 1024]
        ns2 = [16, 32, 64, 128, 256, 512, 1024, 2048]
        heads = [0, 0, 0, 8, 8, 8, 8, 0]
        for i in range(7):
            self.down_blocks.append(ResnetBlock(ns[i], ns2[i], 2, heads=heads[i]))
        self.down_blocks.append(ConvAct(ns[7], ns2[7], 2, 1, padding=0))
        self.mid_blocks.append(ConvAct(2048, 4096, 1))
        self.mid_blocks.append(MultiHeadSelfAttention(4096, heads=8))
        self.mid_blocks.append(ConvAct(4096, 2048, 1))
        ns = [2048, 2048, 1536, 1024, 640, 384, 224, 128, 64]
        ns2 = [1024, 1024, 768, 512, 320, 192, 112, 64, 3]
        heads = [0, 8, 8, 8, 8, 0, 0, 0, 0]
        self.up_blocks.append(ConvTransposeAct(ns[0], ns2[0], 4, 2, padding=1))
        for i in range(1, 8):
            self.up_blocks.append(ResnetTransposeBlock(ns[i], ns2[i], 2, heads=heads[i]))
        self.up_blocks.append(nn.Conv2d(ns[8], ns2[8], 3, 1, padding=1))

    def half(self):
        raise NotImplementedError("UnblurCremageModelV6: fp32 class only (the reference runs this network in fp32)")

    def bfloat16(self):
        raise NotImplementedError("UnblurCremageModelV6: fp32 class only (the reference runs this network in fp32)")

    def _run(self, inputs: torch.Tensor):
        _fp32_only(self, "UnblurCremageModelV6")
        x = _image(inputs, "UnblurCremageModelV6")
        n, c, hh, ww = x.shape
        if c != 3 or (hh, ww) != (256, 256):
            raise CrgError(f"UnblurCremageModelV6: [B, 3, 256, 256] faces expected (seven stride-2 levels, then a 2 x 2 'valid' conv), got {tuple(x.shape)}")
        dev = x.device
        x = _slot_input(x)
        planes = ops.split_bf16(x)
        x = None  # down_blocks.0.blocks.0 has a conv_skip
        taps: List[torch.Tensor] = []
        tap_planes: List[Planes] = []
        for block in list(self.down_blocks)[:7]:
            x, planes = block.run(x, planes)
            taps.append(x)
            tap_planes.append(planes)
        x = self.down_blocks[7].run(x)
        taps.append(x)
        x = self.mid_blocks[0].run(x)
        t = ops.tokens_of(x)
        x = ops.image_of(self.mid_blocks[1](t, t, t), 1, 1)
        x = mid = self.mid_blocks[2].run(x)
        y = self.up_blocks[0].run(ops.split_bf16(x))
        # the concat of up block i, i = 1 .. 7, as planes: [this path | tap 7 - i]
        cx, side = y.shape[1], y.shape[2]
        ct = taps[6].shape[1]
        cat = (ops.empty_image(n, cx + ct, side, side, ops.HALF, dev), ops.empty_image(n, cx + ct, side, side, ops.HALF, dev))
        ops.leaky_split(y, 1.0, fp32=False, planes=(cat[0][:, :cx], cat[1][:, :cx]))
        for i in range(1, 8):
            tp = tap_planes[7 - i]
            cat[0][:, cx:].copy_(tp[0])
            cat[1][:, cx:].copy_(tp[1])
            block = self.up_blocks[i]
            if i < 7:
                cx, side = block.blocks[0].conv2.out_channels, 2 * side
                ct = taps[6 - i].shape[1]
                nxt = (ops.empty_image(n, cx + ct, side, side, ops.HALF, dev), ops.empty_image(n, cx + ct, side, side, ops.HALF, dev))
                x, _ = block.run(None, cat, out_planes=(nxt[0][:, :cx], nxt[1][:, :cx]))
                cat = nxt
            else:
                x, planes = block.run(None, cat)
        last = self.up_blocks[8]
        out = ops.conv2d(planes[0], last.weight, last.bias, padding=1, x_lo=planes[1])
        return out, taps, mid

    @torch.no_grad()
    def debug_forward(self, inputs: torch.Tensor) -> Dict[str, List[torch.Tensor]]:
        """the output, the eight `h` taps of the down path and the mid output, each contiguous NCHW fp32"""
        out, taps, mid = self._run(inputs)
        nchw = lambda t: ops.nhwc_to_nchw(t, torch.float32)  # noqa: E731
        return {"out": [nchw(out)], "h": [nchw(t) for t in taps], "mid": [nchw(mid)]}

    @torch.no_grad()
    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        return ops.nhwc_to_nchw(self._run(inputs)[0], torch.float32)
