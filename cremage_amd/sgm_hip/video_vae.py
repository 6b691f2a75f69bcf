"""Stable Video Diffusion first stage on HIP kernels - drop-in for modules/sdxl/sgm/modules/autoencoding/temporal_ae.py
(`VideoResBlock` :16-81, `AE3DConv` :84-105, `VideoDecoder` :291-347) and `AutoencodingEngine` (sgm/models/autoencoder.py:102-215),
configured by the first_stage_config of scripts/sampling/configs/svd_xt_1_1.yaml.  Same constructor signatures, module tree and
parameter names, so the `first_stage_model.*` keys of an `svd*.safetensors` state dict load unchanged.

Layout.  Activations stay [(b t), C, h, w] channels-last - the same bytes as [b, t, h w, C] tokens - and the reference's
`(b t) c h w <-> b c t h w` rearranges never run:
  * the spatial layers (ResnetBlock, AttnBlock, Upsample, the 3x3 output conv) are the image decoder's (ldm_hip.vae), on b t samples;
  * `time_stack` of a VideoResBlock (sgm openaimodel.py:242-358 with dims=3, kernel (3, 1, 1), no embedding): its GroupNorms see the
    frames of one video as ONE sample (the existing kernel on b samples of t h w pixels).  fp32 class: the norm writes the two half-type
    planes, `ops.conv_frames_x3` reads them - no fp32 round trip between norm and conv; the second conv takes the identity skip and the
    blend in its epilogue.  Half type: `ops.conv_frames`.
    The blend (temporal_ae.py:77-78) is alpha * time_stack(x) + (1 - alpha) * x = x + alpha * c with c what time_stack adds to its
    input: alpha weights the TEMPORAL branch here - the opposite sense to the UNet's AlphaBlender (video.py) - so rscale = alpha;
  * `AE3DConv.time_mix_conv` on the 3 pixel channels is `ops.conv_frames_thin`.
`time_mode` "all" / "attn-only" need the reference's VideoBlock (temporal attention inside the VAE) and raise NotImplementedError.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Union

import torch
import torch.nn as nn

from .. import ops
from ..ldm_hip.latent_diffusion import instantiate_from_config
from ..ldm_hip.nn import Conv2d, SiLU, normalization, zero_module
from ..ldm_hip.vae import Decoder, DiagonalGaussianDistribution, ResnetBlock


def _frame_kernel(video_kernel_size, what: str) -> None:
    """Only the (3, 1, 1) kernel of the SVD configurations is restated.  An int 3 is NOT that kernel: the reference hands it to
    conv_nd(3, ...) / Conv3d as it is and builds a 3 x 3 x 3 conv, whose weights no (3, 1, 1) kernel can take."""
    ks = list(video_kernel_size) if isinstance(video_kernel_size, Iterable) else video_kernel_size
    if ks != [3, 1, 1]:
        raise NotImplementedError(f"{what}: video_kernel_size {video_kernel_size!r} - only [3, 1, 1] (svd_xt_1_1.yaml) is restated "
                                  "(temporal_ae.py:28-42, :87-97: anything else is a conv over space as well)")


class _FrameConv(nn.Conv3d):
    """Parameter container of a (3, 1, 1) conv along the frame axis ([Cout, Cin, 3, 1, 1]); the owning block calls the ops arm."""


class TimeStack(nn.Module):
    """`ResBlock(channels, emb_channels=0, dims=3, kernel_size=[3, 1, 1], skip_t_emb=True)` of sgm openaimodel.py:242-358, same parameter
    names: GroupNorm32 (eps 1e-5) over (C / 32, t, h, w) + SiLU + frame conv, twice, identity skip; no embedding (emb_layers is None)."""

    def __init__(self, channels: int):
        super().__init__()
        self.channels = self.out_channels = channels
        self.in_layers = nn.Sequential(normalization(channels), SiLU(), _FrameConv(channels, channels, (3, 1, 1), padding=(1, 0, 0)))
        self.emb_layers = None
        self.out_layers = nn.Sequential(normalization(channels), SiLU(), nn.Dropout(p=0.0),
                                        zero_module(_FrameConv(channels, channels, (3, 1, 1), padding=(1, 0, 0))))
        self.skip_connection = nn.Identity()

    @staticmethod
    def _video_norm(norm, x, b, h, w, split):
        """GroupNorm + SiLU over (C / 32, t, h, w): the frames of a video are one sample of t * h rows (TimeStackResBlock._video_norm);
        `split`: the result as the (hi, lo) token planes of the fp32 class"""
        F, S, C = x.shape
        y = norm(ops.image_of(x.reshape(b, (F // b) * S, C), (F // b) * h, w), silu=True, split=split)
        if split:
            return tuple(ops.tokens_of(p).reshape(F, S, C) for p in y)
        return ops.tokens_of(y).reshape(F, S, C)

    def forward(self, x, frames: int, h: int, w: int, rscale: torch.Tensor):
        """x [(b t), s, c] tokens -> x + rscale[frame] * (what the block adds to x)"""
        b = x.shape[0] // frames
        c1, c2 = self.in_layers[2], self.out_layers[3]
        if x.dtype == torch.float32:
            hi, lo = self._video_norm(self.in_layers[0], x, b, h, w, True)
            y = ops.conv_frames_x3(hi, lo, c1.weight, c1.bias, frames=frames)
            hi, lo = self._video_norm(self.out_layers[0], y, b, h, w, True)
            return ops.conv_frames_x3(hi, lo, c2.weight, c2.bias, frames=frames, residual=x, rscale=rscale)
        y = self._video_norm(self.in_layers[0], x, b, h, w, False)
        y = ops.conv_frames(y, c1.weight, c1.bias, frames=frames)
        y = self._video_norm(self.out_layers[0], y, b, h, w, False)
        return ops.conv_frames(y, c2.weight, c2.bias, frames=frames, residual=x, rscale=rscale)


class VideoResBlock(ResnetBlock):
    def __init__(self, out_channels, *args, dropout=0.0, video_kernel_size=3, alpha=0.0, merge_strategy="learned", **kwargs):
        super().__init__(out_channels=out_channels, dropout=dropout, *args, **kwargs)
        if dropout:
            raise NotImplementedError("inference-only: dropout must be 0")
        _frame_kernel([3, 1, 1] if video_kernel_size is None else video_kernel_size, "VideoResBlock")
        self.time_stack = TimeStack(out_channels)
        self.merge_strategy = merge_strategy
        if merge_strategy == "fixed":
            self.register_buffer("mix_factor", torch.Tensor([alpha]))
        elif merge_strategy == "learned":
            self.register_parameter("mix_factor", nn.Parameter(torch.Tensor([alpha])))
        else:
            raise ValueError(f"unknown merge strategy {merge_strategy}")

    def get_alpha(self, bs=None):
        if self.merge_strategy == "fixed":
            return self.mix_factor
        return torch.sigmoid(self.mix_factor)

    def forward(self, x, temb=None, skip_video=False, timesteps=None):
        # the statistics side channel of conv2 feeds the NEXT block's per-frame norm1: behind a time stack nobody reads it
        xs = super().forward(x, temb, gn_stats=bool(skip_video))
        if skip_video:
            return xs
        if timesteps is None:
            timesteps = getattr(self, "timesteps", None)  # as the reference: an attribute nobody sets - the caller passes it
        F, _, h, w = xs.shape
        if not timesteps or F % timesteps:
            raise ValueError(f"VideoResBlock: a batch of {F} images is no whole number of videos of {timesteps} frames")
        alpha = self.get_alpha().detach().float().reshape(-1).expand(F)
        y = self.time_stack(ops.tokens_of(ops.to_channels_last(xs)), timesteps, h, w, rscale=alpha)
        return ops.image_of(y, h, w)


class AE3DConv(Conv2d):
    def __init__(self, in_channels, out_channels, video_kernel_size=3, *args, **kwargs):
        super().__init__(in_channels, out_channels, *args, **kwargs)
        _frame_kernel(video_kernel_size, "AE3DConv")
        if out_channels > 8:
            raise NotImplementedError(f"AE3DConv: {out_channels} output channels (the thin frame conv takes at most 8)")
        self.time_mix_conv = nn.Conv3d(in_channels=out_channels, out_channels=out_channels, kernel_size=(3, 1, 1), padding=(1, 0, 0))

    def forward(self, input, timesteps, skip_video=False):
        x = super().forward(input)
        if skip_video:
            return x
        x = ops.to_channels_last(x)
        F, _, h, w = x.shape
        y = ops.conv_frames_thin(ops.tokens_of(x), self.time_mix_conv.weight, self.time_mix_conv.bias, frames=timesteps)
        return ops.image_of(y, h, w)


class VideoDecoder(Decoder):
    available_time_modes = ["all", "conv-only", "attn-only", "only-last-conv"]

    def __init__(self, *args, video_kernel_size: Union[int, list] = 3, alpha: float = 0.0, merge_strategy: str = "learned",
                 time_mode: str = "conv-only", **kwargs):
        assert time_mode in self.available_time_modes, f"time_mode parameter has to be in {self.available_time_modes}"
        if time_mode in ("all", "attn-only"):
            raise NotImplementedError(f"VideoDecoder: time_mode {time_mode!r} needs VideoBlock (temporal attention in the VAE, "
                                      "temporal_ae.py:108-175, :322-330), which is not restated; the SVD configurations use 'conv-only'")
        super().__init__(*args, **kwargs)
        self.video_kernel_size, self.alpha, self.merge_strategy, self.time_mode = video_kernel_size, alpha, merge_strategy, time_mode
        if time_mode == "conv-only":  # _make_resblock (:338-347): every ResnetBlock of the decoder becomes a VideoResBlock
            def video_block(blk: ResnetBlock):
                return VideoResBlock(blk.out_channels, in_channels=blk.in_channels, conv_shortcut=blk.use_conv_shortcut, dropout=0.0,
                                     temb_channels=self.temb_ch, video_kernel_size=video_kernel_size, alpha=alpha, merge_strategy=merge_strategy)
            self.mid.block_1, self.mid.block_2 = video_block(self.mid.block_1), video_block(self.mid.block_2)
            for up in self.up:
                up.block = nn.ModuleList([video_block(blk) for blk in up.block])
        c = self.conv_out  # _make_conv (:332-336)
        self.conv_out = AE3DConv(c.in_channels, c.out_channels, video_kernel_size, kernel_size=3, stride=1, padding=1)

    def get_last_layer(self, skip_time_mix=False, **kwargs):
        return self.conv_out.time_mix_conv.weight if not skip_time_mix else self.conv_out.weight

    @staticmethod
    def frames_per_video(z, timesteps: Optional[int] = None) -> int:
        """`timesteps` as the caller gave it, or - None - the whole batch as ONE video.  The reference's `decode_first_stage`
        (sgm/models/diffusion.py:126-133) passes timesteps = len(chunk) only to a decoder that is an instance of ITS `VideoDecoder` class;
        this class is not, so under the reference's DiffusionEngine it is called as decoder(z) - and len(chunk) is z.shape[0]."""
        t = z.shape[0] if timesteps is None else int(timesteps)
        if t < 1 or z.shape[0] % t:
            raise ValueError(f"VideoDecoder: a batch of {z.shape[0]} frames is no whole number of videos of {t} frames")
        return t

    def forward(self, z, timesteps: Optional[int] = None, skip_video: bool = False):
        """z: channels-last latents [(b t), C, h, w] in the compute dtype -> frames; timesteps None = one video of z.shape[0] frames"""
        return self._decode(z, self.frames_per_video(z, timesteps), skip_video)

    def _decode(self, z, timesteps: int, skip_video: bool):
        """sgm model.py:730-763; `mid.attn_1` and the Upsample layers take no video arguments"""
        self.last_z_shape = z.shape
        kw = dict(skip_video=skip_video, timesteps=timesteps)
        res = (lambda blk, h: blk(h, None, **kw)) if self.time_mode == "conv-only" else (lambda blk, h: blk(h))
        h = self.conv_in(z)
        h = res(self.mid.block_1, h)
        h = self.mid.attn_1(h)
        h = res(self.mid.block_2, h)
        for i_level in reversed(range(self.num_resolutions)):
            for i_block in range(self.num_res_blocks + 1):
                h = res(self.up[i_level].block[i_block], h)
                if len(self.up[i_level].attn) > 0:
                    h = self.up[i_level].attn[i_block](h)
            if i_level != 0:
                h = self.up[i_level].upsample(h)
        return self.conv_out(self.norm_out(h, silu=True), timesteps, skip_video=skip_video)


class DiagonalGaussianRegularizer(nn.Module):
    """sgm/modules/autoencoding/regularizers/__init__.py:13-31, with the noise of the sample as an explicit argument."""

    def __init__(self, sample: bool = True):
        super().__init__()
        self.sample = sample

    def get_trainable_parameters(self):
        yield from ()

    def forward(self, z: torch.Tensor, noise: Optional[torch.Tensor] = None):
        posterior = DiagonalGaussianDistribution(z)
        out = posterior.sample(noise) if self.sample else posterior.mode()
        kl = 0.5 * torch.sum(posterior.mean ** 2 + posterior.var - 1.0 - posterior.logvar, dim=[1, 2, 3])
        return out, {"kl_loss": torch.sum(kl) / kl.shape[0]}


class AutoencodingEngine(nn.Module):
    """sgm/models/autoencoder.py:102-215 without the training plumbing: encoder / decoder / regularization from their configs
    (parameter names `encoder.*`, `decoder.*`; there is no quant_conv in this class).  NCHW tensors at the boundary, channels-last in
    the compute dtype inside, as ldm_hip.vae.AutoencoderKL."""

    def __init__(self, *args, encoder_config: Dict, decoder_config: Dict, loss_config: Optional[Dict] = None, regularizer_config: Dict,
                 optimizer_config: Optional[Dict] = None, lr_g_factor: float = 1.0, ckpt_engine=None, ckpt_path: Optional[str] = None,
                 additional_decode_keys=None, **kwargs):
        super().__init__()
        if ckpt_engine is not None or ckpt_path is not None:
            raise NotImplementedError("AutoencodingEngine: load the state dict from outside (ckpt_engine / ckpt_path are not restated)")
        self.encoder = instantiate_from_config(encoder_config)
        self.decoder = instantiate_from_config(decoder_config)
        self.loss = nn.Identity()
        self.regularization = instantiate_from_config(regularizer_config)
        self.additional_decode_keys = set(additional_decode_keys or [])
        self.compute_dtype: Optional[torch.dtype] = None

    def resolve_compute_dtype(self) -> torch.dtype:
        if self.compute_dtype is not None:
            return self.compute_dtype
        return ops.HALF if self.decoder.conv_in.weight.dtype in (torch.bfloat16, torch.float16) else torch.float32

    def get_last_layer(self):
        return self.decoder.get_last_layer()

    def encode(self, x: torch.Tensor, return_reg_log: bool = False, unregularized: bool = False, *, noise: Optional[torch.Tensor] = None):
        """image [n, 3, H, W] NCHW in [-1, 1] -> the regularised latent [n, 4, H / 8, W / 8] fp32.  Positional order of the reference
        (autoencoder.py:196-201); `noise`, keyword-only: the sample's N(0, 1) draw"""
        cdt = self.resolve_compute_dtype()
        z = ops.nhwc_to_nchw(self.encoder(ops.nchw_to_nhwc(x, cdt)), torch.float32)
        if unregularized:
            return z, dict()
        z, reg_log = self.regularization(z, noise)
        return (z, reg_log) if return_reg_log else z

    def decode(self, z: torch.Tensor, **kwargs) -> torch.Tensor:
        """latents [(b t), 4, h, w] NCHW -> frames [(b t), 3, 8 h, 8 w] NCHW fp32; kwargs (`timesteps`, `skip_video`) go to the decoder; without
        `timesteps` the batch is one video - what the reference's decode_first_stage means when it calls decode(chunk) bare"""
        cdt = self.resolve_compute_dtype()
        return ops.nhwc_to_nchw(self.decoder(ops.nchw_to_nhwc(z, cdt), **kwargs), torch.float32)

    def forward(self, x: torch.Tensor, *, noise: Optional[torch.Tensor] = None, **additional_decode_kwargs):
        z, reg_log = self.encode(x, return_reg_log=True, noise=noise)
        return z, self.decode(z, **additional_decode_kwargs), reg_log
