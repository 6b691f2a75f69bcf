"""Stable Video Diffusion UNet on HIP kernels - drop-in for modules/sdxl/sgm/modules/diffusionmodules/video_model.py (`VideoResBlock`
:12-81, `VideoUNet` :84-493), modules/sdxl/sgm/modules/video_attention.py (`VideoTransformerBlock` :16-141, `SpatialVideoTransformer`
:147-302) and `AlphaBlender` (diffusionmodules/util.py:350-407), configured by scripts/sampling/configs/svd_xt_1_1.yaml.  Same
constructor signatures, module tree and parameter names, so an `svd*.safetensors` state dict loads unchanged.

Layout.  Activations stay [(b t), C, h, w] channels-last from conv_in to the output conv - the same bytes as [b, t, h w, C] tokens - and
the reference's rearranges never run:
  * spatial layers (ResBlock, BasicTransformerBlock, Down / Upsample) are the image UNet's, on b t samples;
  * `time_stack` of a VideoResBlock: its GroupNorms see the frames of one video as ONE sample (the existing kernel on b samples of
    t h w pixels), its (3, 1, 1) convs are `ops.conv_frames`; the first takes the per-frame embedding rows as `cvec`
    (exchange_temb_dims), the second takes the identity skip and the AlphaBlender in its epilogue: x + (1 - alpha_f) conv(...);
  * `time_stack` of a SpatialVideoTransformer: LayerNorms, projections and feed-forwards are token-wise and run as they are;
    attention across the frames of a pixel is `ops.attention_frames` on the column slices of one Q | K | V launch; the temporal
    cross-attention reads `context[::t]` ([b, M, ctx]: every pixel and frame of a video shares its keys), i.e. the image
    cross-attention with b samples of t h w queries.
Structural options the SVD configurations never set raise NotImplementedError.
"""
from __future__ import annotations

from typing import List, Optional, Union

import torch
import torch.nn as nn

from .. import ops
from ..ldm_hip import transformer as T
from ..ldm_hip.nn import SiLU, conv_nd, linear, normalization, timestep_embedding, zero_module
from ..ldm_hip.unet import Downsample, ResBlock, TimestepBlock, Upsample
from ..ldm_hip.unet import UNetModel as _SD15UNet
from .transformer import CrossAttention, SpatialTransformer


def _frames_of(x: torch.Tensor, frames: Optional[int], what: str) -> int:
    if not frames or x.shape[0] % frames:
        raise ValueError(f"{what}: a batch of {x.shape[0]} images is no whole number of videos of {frames} frames")
    return x.shape[0] // frames


class AlphaBlender(nn.Module):
    """util.py:350-407: alpha * x_spatial + (1 - alpha) * x_temporal with alpha fixed, learned (sigmoid of a parameter), or learned with
    image-only frames passed through (alpha = 1 where `image_only_indicator` is set)."""
    strategies = ["learned", "fixed", "learned_with_images"]

    def __init__(self, alpha: float, merge_strategy: str = "learned_with_images", rearrange_pattern: str = "b t -> (b t) 1 1"):
        super().__init__()
        if merge_strategy not in self.strategies:
            raise ValueError(f"merge_strategy needs to be in {self.strategies}")
        if rearrange_pattern not in ("b t -> (b t) 1 1", "b t -> b 1 t 1 1"):
            raise NotImplementedError(f"AlphaBlender: rearrange pattern {rearrange_pattern!r}")
        self.merge_strategy = merge_strategy
        self.rearrange_pattern = rearrange_pattern
        if merge_strategy == "fixed":
            self.register_buffer("mix_factor", torch.Tensor([alpha]))
        else:
            self.register_parameter("mix_factor", nn.Parameter(torch.Tensor([alpha])))

    def get_alpha(self, image_only_indicator: Optional[torch.Tensor]) -> torch.Tensor:
        """The reference's tensor: shape [1] (fixed, learned) or the indicator [b, t] laid out by the rearrange pattern."""
        if self.merge_strategy == "fixed":
            return self.mix_factor
        if self.merge_strategy == "learned":
            return torch.sigmoid(self.mix_factor)
        assert image_only_indicator is not None, "need image_only_indicator ..."
        alpha = torch.where(image_only_indicator.bool(), torch.ones(1, 1, device=image_only_indicator.device),
                            torch.sigmoid(self.mix_factor)[..., None])
        b, t = alpha.shape
        return alpha.reshape(b * t, 1, 1) if self.rearrange_pattern == "b t -> (b t) 1 1" else alpha.reshape(b, 1, t, 1, 1)

    def frame_alpha(self, image_only_indicator: Optional[torch.Tensor], frames: int) -> torch.Tensor:
        """alpha per frame, fp32 [frames] in (b t) order - what the per-frame kernels take, whichever pattern the module was built with."""
        a = self.get_alpha(image_only_indicator).detach().float().reshape(-1)
        return a.expand(frames) if a.numel() == 1 else a

    def forward(self, x_spatial: torch.Tensor, x_temporal: torch.Tensor, image_only_indicator: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[(b t), s, c] tokens (either pattern: the layout is the same bytes)."""
        return ops.blend_frames(self.frame_alpha(image_only_indicator, x_spatial.shape[0]), x_spatial, x_temporal)


class _FrameConv(nn.Conv3d):
    """Parameter container of a (3, 1, 1) conv along the frame axis ([Cout, Cin, 3, 1, 1]); forward = ops.conv_frames on tokens."""

    def forward(self, x, frames: int, **fused):
        return ops.conv_frames(x, self.weight, self.bias, frames=frames, **fused)


class TimeStackResBlock(TimestepBlock):
    """The `ResBlock(dims=3, kernel_size=(3, 1, 1), exchange_temb_dims=True)` of video_model.py:42-55, same parameter names.  Works on
    [(b t), s, c] tokens; `rscale` = 1 - alpha per frame folds the AlphaBlender behind it into the second conv."""

    def __init__(self, channels: int, emb_channels: int, kernel_size):
        super().__init__()
        if list(kernel_size) != [3, 1, 1]:
            raise NotImplementedError(f"video_kernel_size {kernel_size}: only [3, 1, 1] (the SVD configurations) is restated")
        self.channels = self.out_channels = channels
        self.in_layers = nn.Sequential(normalization(channels), SiLU(), _FrameConv(channels, channels, (3, 1, 1), padding=(1, 0, 0)))
        self.emb_layers = nn.Sequential(SiLU(), linear(emb_channels, channels))
        self.out_layers = nn.Sequential(normalization(channels), SiLU(), nn.Dropout(p=0.0),
                                        zero_module(_FrameConv(channels, channels, (3, 1, 1), padding=(1, 0, 0))))
        self.skip_connection = nn.Identity()

    @staticmethod
    def _video_norm(norm, x, b, h, w):
        """GroupNorm + SiLU over (C / 32, t, h, w): the frames of a video are one sample of t * h rows"""
        F, S, C = x.shape
        y = norm(ops.image_of(x.reshape(b, (F // b) * S, C), (F // b) * h, w), silu=True)
        return ops.tokens_of(y).reshape(F, S, C)

    def forward(self, x, emb, frames: int, h: int, w: int, rscale: Optional[torch.Tensor] = None):
        b = x.shape[0] // frames
        emb_out = self.emb_layers[1](ops.silu(emb), out_dtype=torch.float32)  # [(b t), C]: one row per frame
        y = self._video_norm(self.in_layers[0], x, b, h, w)
        y = self.in_layers[2](y, frames, cvec=emb_out)
        y = self._video_norm(self.out_layers[0], y, b, h, w)
        return self.out_layers[3](y, frames, residual=x, rscale=rscale)


class VideoResBlock(ResBlock):
    def __init__(self, channels: int, emb_channels: int, dropout: float, video_kernel_size: Union[int, List[int]] = 3,
                 merge_strategy: str = "fixed", merge_factor: float = 0.5, out_channels: Optional[int] = None, use_conv: bool = False,
                 use_scale_shift_norm: bool = False, dims: int = 2, use_checkpoint: bool = False, up: bool = False, down: bool = False):
        super().__init__(channels, emb_channels, dropout, out_channels=out_channels, use_conv=use_conv,
                         use_scale_shift_norm=use_scale_shift_norm, dims=dims, use_checkpoint=use_checkpoint, up=up, down=down)
        if dropout:
            raise NotImplementedError("inference-only: dropout must be 0")
        ks = [video_kernel_size] * 3 if isinstance(video_kernel_size, int) else list(video_kernel_size)
        self.time_stack = TimeStackResBlock(self.out_channels, emb_channels, ks)
        self.time_mixer = AlphaBlender(alpha=merge_factor, merge_strategy=merge_strategy, rearrange_pattern="b t -> b 1 t 1 1")

    def forward(self, x, emb, num_video_frames: int, image_only_indicator: Optional[torch.Tensor] = None):
        xs = super().forward(x, emb)
        _frames_of(xs, num_video_frames, "VideoResBlock")
        F, _, h, w = xs.shape
        # alpha x + (1 - alpha) (x + c) = x + (1 - alpha) c, c = what time_stack adds to its input: skip and blend in one epilogue
        one_minus = 1.0 - self.time_mixer.frame_alpha(image_only_indicator, F)
        y = self.time_stack(ops.tokens_of(xs), emb, num_video_frames, h, w, rscale=one_minus)
        return ops.image_of(y, h, w)


class VideoTransformerBlock(nn.Module):
    ATTENTION_MODES = {"softmax": CrossAttention, "softmax-xformers": CrossAttention, "softmax-hip": CrossAttention}

    def __init__(self, dim, n_heads, d_head, dropout=0.0, context_dim=None, gated_ff=True, checkpoint=True, timesteps=None, ff_in=False,
                 inner_dim=None, attn_mode="softmax", disable_self_attn=False, disable_temporal_crossattention=False,
                 switch_temporal_ca_to_sa=False):
        super().__init__()
        attn_cls = self.ATTENTION_MODES[attn_mode]
        self.ff_in = ff_in or inner_dim is not None
        if inner_dim is None:
            inner_dim = dim
        assert int(n_heads * d_head) == inner_dim
        self.is_res = inner_dim == dim
        if self.ff_in:
            self.norm_in = nn.LayerNorm(dim)
            self.ff_in = T.FeedForward(dim, dim_out=inner_dim, dropout=dropout, glu=gated_ff)
        self.timesteps = timesteps
        self.disable_self_attn = disable_self_attn
        self.attn1 = attn_cls(query_dim=inner_dim, heads=n_heads, dim_head=d_head, dropout=dropout,
                              context_dim=context_dim if disable_self_attn else None)
        self.ff = T.FeedForward(inner_dim, dim_out=dim, dropout=dropout, glu=gated_ff)
        if disable_temporal_crossattention:
            if switch_temporal_ca_to_sa:
                raise ValueError
            self.attn2 = None
        else:
            self.norm2 = nn.LayerNorm(inner_dim)
            self.attn2 = attn_cls(query_dim=inner_dim, heads=n_heads, dim_head=d_head, dropout=dropout,
                                  context_dim=None if switch_temporal_ca_to_sa else context_dim)
        self.norm1 = nn.LayerNorm(inner_dim)
        self.norm3 = nn.LayerNorm(inner_dim)
        self.switch_temporal_ca_to_sa = switch_temporal_ca_to_sa
        self.checkpoint = checkpoint  # activation checkpointing: nothing to do at inference

    def _frame_attention(self, attn: CrossAttention, norm: nn.LayerNorm, x, frames):
        """x + to_out(attention over the frames of each pixel): LayerNorm + Q | K | V in one launch, the kernel reads its column slices"""
        wq, wk, wv = attn.to_q.weight, attn.to_k.weight, attn.to_v.weight
        c = wq.shape[0]
        qkv = ops.ln_linear_auto(x, norm, attn._stack(wq, wk, wv))
        o = ops.attention_frames(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], attn.heads, frames=frames, scale=attn.scale)
        return ops.linear(o, attn.to_out[0].weight, attn.to_out[0].bias, residual=x)

    @staticmethod
    def _video_attention(attn: CrossAttention, norm: nn.LayerNorm, x, context, frames):
        """x + attn(norm(x), context) with the context of a VIDEO ([b, M, ctx]): its t * s tokens are the queries of one sample"""
        F, S, C = x.shape
        xv = x.reshape(F // frames, frames * S, C)
        return attn(xv, context=context, residual=xv, ln=norm).reshape(F, S, C)

    def forward(self, x: torch.Tensor, context: Optional[torch.Tensor] = None, timesteps: Optional[int] = None) -> torch.Tensor:
        """x [(b t), s, c] tokens; context [b, M, ctx] - one per video (the reference repeats it over the pixels: the same keys)."""
        assert self.timesteps or timesteps
        assert not (self.timesteps and timesteps) or self.timesteps == timesteps
        frames = self.timesteps or timesteps
        _frames_of(x, frames, "VideoTransformerBlock")
        if frames > ops.MAX_FRAMES:
            raise NotImplementedError(f"VideoTransformerBlock: {frames} frames (at most {ops.MAX_FRAMES})")
        x = x.contiguous()
        if self.ff_in:
            x = self.ff_in(x, residual=x if self.is_res else None, ln=self.norm_in)
        if self.disable_self_attn:
            x = self._video_attention(self.attn1, self.norm1, x, context, frames)
        else:
            x = self._frame_attention(self.attn1, self.norm1, x, frames)
        if self.attn2 is not None:
            if self.switch_temporal_ca_to_sa or context is None:
                x = self._frame_attention(self.attn2, self.norm2, x, frames)
            else:
                x = self._video_attention(self.attn2, self.norm2, x, context, frames)
        return self.ff(x, residual=x if self.is_res else None, ln=self.norm3)

    def get_last_layer(self):
        return self.ff.net[-1].weight


class SpatialVideoTransformer(SpatialTransformer):
    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0.0, use_linear=False, context_dim=None, use_spatial_context=False,
                 timesteps=None, merge_strategy: str = "fixed", merge_factor: float = 0.5, time_context_dim=None, ff_in=False,
                 checkpoint=False, time_depth=1, attn_mode="softmax", disable_self_attn=False, disable_temporal_crossattention=False,
                 max_time_embed_period: int = 10000):
        super().__init__(in_channels, n_heads, d_head, depth=depth, dropout=dropout, attn_type=attn_mode, use_checkpoint=checkpoint,
                         context_dim=context_dim, use_linear=use_linear, disable_self_attn=disable_self_attn)
        self.time_depth = time_depth
        self.depth = depth
        self.max_time_embed_period = max_time_embed_period
        inner_dim = n_heads * d_head
        if use_spatial_context:
            time_context_dim = context_dim
        self.time_stack = nn.ModuleList([
            VideoTransformerBlock(inner_dim, n_heads, d_head, dropout=dropout, context_dim=time_context_dim, timesteps=timesteps,
                                  checkpoint=checkpoint, ff_in=ff_in, inner_dim=inner_dim, attn_mode=attn_mode,
                                  disable_self_attn=disable_self_attn, disable_temporal_crossattention=disable_temporal_crossattention)
            for _ in range(self.depth)])
        assert len(self.time_stack) == len(self.transformer_blocks)
        self.use_spatial_context = use_spatial_context
        self.in_channels = in_channels
        self.time_pos_embed = nn.Sequential(linear(in_channels, in_channels * 4), SiLU(), linear(in_channels * 4, in_channels))
        self.time_mixer = AlphaBlender(alpha=merge_factor, merge_strategy=merge_strategy)

    @staticmethod
    def _first_frames(context: torch.Tensor, frames: int) -> torch.Tensor:
        """context[::frames], the same tensor object while the context is unchanged (the cross-attention K / V cache keys on it)"""
        c = getattr(context, "_crg_first_frames", None)
        if c is None or c[0] != (frames, context._version):
            c = context._crg_first_frames = ((frames, context._version), context[::frames].contiguous())
        return c[1]

    def forward(self, x, context=None, time_context=None, timesteps: Optional[int] = None, image_only_indicator=None):
        if isinstance(context, list):
            if len(context) != 1:
                raise NotImplementedError("per-block context lists are not used by the SVD configurations")
            context = context[0]
        x = ops.to_channels_last(x)
        F, _, h, w = x.shape
        _frames_of(x, timesteps, "SpatialVideoTransformer")
        if self.use_spatial_context:
            assert context.ndim == 3, f"n dims of spatial context should be 3 but are {context.ndim}"
            time_context = self._first_frames(context, timesteps)
        elif time_context is not None and time_context.ndim == 2:
            time_context = time_context[:, None, :]
        x_in = ops.tokens_of(x)
        # side channels as in the image SpatialTransformer: proj_in hands the first block's norm1 its row statistics, proj_out hands the
        # next ResBlock's GroupNorm its statistics - with every frame image-only the spatial layers then run the image network's launches
        t = ops.linear(ops.tokens_of(self.norm(x)), self.proj_in.weight, self.proj_in.bias,
                       row_stats=ops.ln_epi_wanted(self.proj_in.weight.shape[0]))
        # position of a frame inside its video -> one channel vector per frame
        pos = torch.arange(timesteps, device=x.device, dtype=torch.float32).repeat(F // timesteps)
        t_emb = timestep_embedding(pos, self.in_channels, max_period=self.max_time_embed_period, dtype=t.dtype)
        emb = self.time_pos_embed[2](self.time_pos_embed[0](t_emb, act="silu"))
        alpha = self.time_mixer.frame_alpha(image_only_indicator, F)
        for block, mix_block in zip(self.transformer_blocks, self.time_stack):
            block._crg_next_is_block = False
            t = block(t, context=context)
            t_mix = mix_block(ops.add_frames(t, emb), context=time_context, timesteps=timesteps)
            t = ops.blend_frames(alpha, t, t_mix)
        y = ops.linear(t, self.proj_out.weight, self.proj_out.bias, residual=x_in, gn_hw=h * w)
        return ops.image_of_stats(y, h, w)


class TimestepEmbedSequential(nn.Sequential, TimestepBlock):
    """sgm openaimodel.py:66-108: video blocks get the frame count and the image-only indicator, video transformers the time context too."""

    def forward(self, x, emb, context=None, image_only_indicator=None, time_context=None, num_video_frames=None):
        for layer in self:
            if isinstance(layer, VideoResBlock):
                x = layer(x, emb, num_video_frames, image_only_indicator)
            elif isinstance(layer, TimestepBlock):
                x = layer(x, emb)
            elif isinstance(layer, SpatialVideoTransformer):
                x = layer(x, context, time_context, num_video_frames, image_only_indicator)
            elif isinstance(layer, T.SpatialTransformer):
                x = layer(x, context)
            else:
                x = layer(x)
        return x


class VideoUNet(nn.Module):
    def __init__(self, in_channels: int, model_channels: int, out_channels: int, num_res_blocks: int, attention_resolutions: int,
                 dropout: float = 0.0, channel_mult: List[int] = (1, 2, 4, 8), conv_resample: bool = True, dims: int = 2,
                 num_classes: Optional[Union[int, str]] = None, use_checkpoint: bool = False, num_heads: int = -1, num_head_channels: int = -1,
                 num_heads_upsample: int = -1, use_scale_shift_norm: bool = False, resblock_updown: bool = False,
                 transformer_depth: Union[List[int], int] = 1, transformer_depth_middle: Optional[int] = None,
                 context_dim: Optional[int] = None, time_downup: bool = False, time_context_dim: Optional[int] = None,
                 extra_ff_mix_layer: bool = False, use_spatial_context: bool = False, merge_strategy: str = "fixed",
                 merge_factor: float = 0.5, spatial_transformer_attn_type: str = "softmax", video_kernel_size: Union[int, List[int]] = 3,
                 use_linear_in_transformer: bool = False, adm_in_channels: Optional[int] = None,
                 disable_temporal_crossattention: bool = False, max_ddpm_temb_period: int = 10000):
        super().__init__()
        assert context_dim is not None
        if not conv_resample or resblock_updown or dims != 2 or use_scale_shift_norm or time_downup or dropout:
            raise NotImplementedError("VideoUNet: unsupported structural option for the SVD path")
        if num_classes not in (None, "sequential"):
            raise NotImplementedError("VideoUNet: only num_classes None / 'sequential' (SVD) are restated")
        if max_ddpm_temb_period != 10000:
            raise NotImplementedError("VideoUNet: max_ddpm_temb_period other than 10000")
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads
        if num_heads == -1:
            assert num_head_channels != -1
        if num_head_channels == -1:
            assert num_heads != -1
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        if isinstance(transformer_depth, int):
            transformer_depth = len(channel_mult) * [transformer_depth]
        transformer_depth = list(transformer_depth)
        transformer_depth_middle = T.default(transformer_depth_middle, transformer_depth[-1])
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = attention_resolutions
        self.dropout = dropout
        self.channel_mult = channel_mult
        self.conv_resample = conv_resample
        self.num_classes = num_classes
        self.use_checkpoint = use_checkpoint
        self.num_heads = num_heads
        self.num_head_channels = num_head_channels
        self.num_heads_upsample = num_heads_upsample
        self.compute_dtype: Optional[torch.dtype] = None
        self._ctx_cast = None
        self._resblocks = None

        def heads_for(ch):
            if num_head_channels == -1:
                return num_heads, ch // num_heads
            return ch // num_head_channels, num_head_channels

        def attention_layer(ch, depth):
            nh, dh = heads_for(ch)
            return SpatialVideoTransformer(ch, nh, dh, depth=depth, context_dim=context_dim, time_context_dim=time_context_dim,
                                           dropout=dropout, ff_in=extra_ff_mix_layer, use_spatial_context=use_spatial_context,
                                           merge_strategy=merge_strategy, merge_factor=merge_factor, checkpoint=use_checkpoint,
                                           use_linear=use_linear_in_transformer, attn_mode=spatial_transformer_attn_type,
                                           disable_self_attn=False, disable_temporal_crossattention=disable_temporal_crossattention,
                                           max_time_embed_period=max_ddpm_temb_period)

        def resblock(ch, out_ch):
            return VideoResBlock(merge_factor=merge_factor, merge_strategy=merge_strategy, video_kernel_size=video_kernel_size, channels=ch,
                                 emb_channels=time_embed_dim, dropout=dropout, out_channels=out_ch, dims=dims, use_checkpoint=use_checkpoint,
                                 use_scale_shift_norm=use_scale_shift_norm)

        time_embed_dim = model_channels * 4
        self.time_embed = nn.Sequential(linear(model_channels, time_embed_dim), SiLU(), linear(time_embed_dim, time_embed_dim))
        if self.num_classes == "sequential":
            assert adm_in_channels is not None
            self.label_emb = nn.Sequential(nn.Sequential(linear(adm_in_channels, time_embed_dim), SiLU(),
                                                         linear(time_embed_dim, time_embed_dim)))
        self.input_blocks = nn.ModuleList([TimestepEmbedSequential(conv_nd(dims, in_channels, model_channels, 3, padding=1))])
        input_block_chans = [model_channels]
        ch = model_channels
        ds = 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [resblock(ch, mult * model_channels)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(attention_layer(ch, transformer_depth[level]))
                self.input_blocks.append(TimestepEmbedSequential(*layers))
                input_block_chans.append(ch)
            if level != len(channel_mult) - 1:
                ds *= 2
                self.input_blocks.append(TimestepEmbedSequential(Downsample(ch, conv_resample, dims=dims, out_channels=ch)))
                input_block_chans.append(ch)
        self.middle_block = TimestepEmbedSequential(resblock(ch, None), attention_layer(ch, transformer_depth_middle), resblock(ch, None))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = input_block_chans.pop()
                layers = [resblock(ch + ich, model_channels * mult)]
                ch = model_channels * mult
                if ds in attention_resolutions:
                    layers.append(attention_layer(ch, transformer_depth[level]))
                if level and i == num_res_blocks:
                    ds //= 2
                    layers.append(Upsample(ch, conv_resample, dims=dims, out_channels=ch))
                self.output_blocks.append(TimestepEmbedSequential(*layers))
        self.out = nn.Sequential(normalization(ch), SiLU(), zero_module(conv_nd(dims, model_channels, out_channels, 3, padding=1)))

    # the spatial ResBlocks' embedding projections as one GEMM per call, as in the image UNets (VideoResBlock is a ResBlock; the
    # time stacks project their own rows)
    _emb_projections = _SD15UNet._emb_projections
    _emb_rows = _SD15UNet._emb_rows
    _emb_table = _SD15UNet._emb_table
    resolve_compute_dtype = _SD15UNet.resolve_compute_dtype

    def forward(self, x, timesteps, context=None, y=None, time_context=None, num_video_frames: Optional[int] = None,
                image_only_indicator=None, c_concat=None, **kwargs):
        """x [(b t), C, h, w] NCHW (with `c_concat`: the result equals forward(cat([x, c_concat], 1)) without building the tensor),
        timesteps [(b t)], context [(b t), M, ctx], y [(b t), adm], image_only_indicator [b, t] -> [(b t), C_out, h, w] in x.dtype."""
        assert (y is not None) == (self.num_classes is not None), "must specify y if and only if the model is class-conditional"
        _frames_of(x, num_video_frames, "VideoUNet")
        cdt = self.resolve_compute_dtype()
        t_emb = timestep_embedding(timesteps, self.model_channels, dtype=cdt)
        emb = self.time_embed[2](self.time_embed[0](t_emb, act="silu"))
        if self.num_classes is not None:
            assert y.shape[0] == x.shape[0]
            le = self.label_emb[0]
            emb = le[2](le[0](y if y.dtype == cdt else y.to(cdt), act="silu"), residual=emb)
        emb._crg_emb_out = self._emb_projections(emb)
        if context is not None and context.dtype != cdt:
            c = self._ctx_cast
            if c is None or c[0] is not context or c[1] != context._version or c[2].dtype != cdt:
                self._ctx_cast = c = (context, context._version, context.to(cdt))
            context = c[2]
        if time_context is not None and time_context.dtype != cdt:
            time_context = time_context.to(cdt)
        kw = dict(context=context, image_only_indicator=image_only_indicator, time_context=time_context, num_video_frames=num_video_frames)
        hs = []
        h = ops.nchw_to_nhwc(x, cdt, c_concat)
        for module in self.input_blocks:
            h = module(h, emb, **kw)
            hs.append(h)
        h = self.middle_block(h, emb, **kw)
        for module in self.output_blocks:
            h = module((h, hs.pop()), emb, **kw)
        h = self.out[2](self.out[0](h, silu=True))
        return ops.nhwc_to_nchw(h, x.dtype if x.dtype in (torch.float32, ops.HALF) else torch.float32).to(x.dtype)
