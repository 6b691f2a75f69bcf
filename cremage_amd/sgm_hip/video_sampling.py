"""Sampling glue of the video (SVD) path - stays on PyTorch like sgm_hip/sampling.py, behaviour of
modules/sdxl/sgm/modules/diffusionmodules/{denoiser.py:11-39 (the continuous Denoiser: no sigma table), denoiser_scaling.py:51-59
(VScalingWithEDMcNoise), guiders.py:83-122 (LinearPredictionGuider), sampling.py (EulerEDMSampler on EDMDiscretization,
svd_xt_1_1.yaml's sampler_config)} and of the `additional_model_inputs` the Video Generator hands the network
(sdxl_pipeline/svd_video_generator.py: image_only_indicator, num_video_frames).  The guidance scale differs per frame, so the
update runs on the unfused torch loop: the fused step kernels take one scalar scale."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn as nn

from ..sampler_plan import EDMDiscretization
from ..samplers import append_dims
from .sampling import EulerEDMSampler, OpenAIWrapper


class VScalingWithEDMcNoise:
    """denoiser_scaling.py:51-59."""

    def __call__(self, sigma):
        c_skip = 1.0 / (sigma ** 2 + 1.0)
        c_out = -sigma / (sigma ** 2 + 1.0) ** 0.5
        c_in = 1.0 / (sigma ** 2 + 1.0) ** 0.5
        c_noise = 0.25 * sigma.log()
        return c_skip, c_out, c_in, c_noise


class Denoiser(nn.Module):
    """denoiser.py:11-39: sigma is used as it comes (no table), c_noise = log(sigma) / 4 is the network's `timesteps`."""

    def __init__(self, scaling=None):
        super().__init__()
        self.scaling = scaling or VScalingWithEDMcNoise()

    def forward(self, network, input, sigma, cond: Dict, **additional_model_inputs):
        sigma_shape = sigma.shape
        sigma = append_dims(sigma, input.ndim)
        c_skip, c_out, c_in, c_noise = self.scaling(sigma)
        c_noise = c_noise.reshape(sigma_shape)
        return network(input * c_in, c_noise, cond, **additional_model_inputs) * c_out + input * c_skip


class LinearPredictionGuider:
    """guiders.py:83-122: classifier-free guidance whose scale rises linearly over the frames of a video, linspace(min, max, T).  The
    doubled conditioning is built once per (c, uc) pair, as VanillaCFG does here."""

    def __init__(self, max_scale: float, num_frames: int, min_scale: float = 1.0, additional_cond_keys=None):
        self.min_scale, self.max_scale, self.num_frames = min_scale, max_scale, num_frames
        self.scale = torch.linspace(min_scale, max_scale, num_frames).unsqueeze(0)
        keys = additional_cond_keys or []
        self.additional_cond_keys = [keys] if isinstance(keys, str) else list(keys)
        self._cache = None

    def __call__(self, x, sigma):
        x_u, x_c = x.chunk(2)
        b = x_u.shape[0] // self.num_frames
        scale = append_dims(self.scale.expand(b, -1).reshape(-1), x_u.ndim).to(x_u.device)  # [(b t), 1, 1, 1]: the frame's own scale
        return x_u + scale * (x_c - x_u)

    def cat_cond(self, c, uc):
        k = self._cache
        if k is None or k[0] is not c or k[1] is not uc:
            c_out = dict()
            for key in c:
                if key in ["vector", "crossattn", "concat"] + self.additional_cond_keys:
                    c_out[key] = torch.cat((uc[key], c[key]), 0)
                else:
                    assert c[key] == uc[key]
                    c_out[key] = c[key]
            self._cache = k = (c, uc, c_out)
        return k[2]

    def prepare_inputs(self, x, s, c, uc):
        return torch.cat([x] * 2), torch.cat([s] * 2), self.cat_cond(c, uc)


class EulerEDMVideoSampler(EulerEDMSampler):
    """svd_xt_1_1.yaml sampler_config: Euler on the EDM ODE over EDMDiscretization(sigma_max = 700), with the network's additional inputs."""

    def __init__(self, num_steps: int, guider, device="cuda", sigma_min=0.002, sigma_max=700.0, rho=7.0, additional_model_inputs=None, **kw):
        super().__init__(num_steps, guider, device=device, **kw)
        self.discretization = EDMDiscretization(sigma_min=sigma_min, sigma_max=sigma_max, rho=rho)
        self.additional_model_inputs = additional_model_inputs or {}

    def denoise(self, x, denoiser, sigma, cond, uc):
        denoised = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc), **self.additional_model_inputs)
        return self.guider(denoised, sigma)


def video_model_inputs(num_frames: int, device, videos: int = 1) -> Dict:
    """What the Video Generator passes besides the conditioning: no frame is image-only; the batch is doubled for guidance."""
    return dict(image_only_indicator=torch.zeros(2 * videos, num_frames, device=device), num_video_frames=num_frames)


@torch.no_grad()
def sample_video_latents(unet, x, c: Dict, uc: Dict, *, num_frames: int, steps: int, min_scale: float = 1.0, max_scale: float = 2.5,
                         sigma_max: float = 700.0, network=None) -> torch.Tensor:
    """Euler-EDM over `steps` sigmas from unit-variance noise x [(b t), 4, h, w]; c / uc: dicts with "crossattn" [(b t), M, ctx],
    "vector" [(b t), adm] and "concat" [(b t), 4, h, w].  `network`: a callable in place of OpenAIWrapper(unet) (a GraphedModule adapter)."""
    guider = LinearPredictionGuider(max_scale, num_frames, min_scale)
    sampler = EulerEDMVideoSampler(steps, guider, device=x.device, sigma_max=sigma_max,
                                   additional_model_inputs=video_model_inputs(num_frames, x.device, x.shape[0] // num_frames))
    den, net = Denoiser(), network or OpenAIWrapper(unet)
    return sampler(lambda inp, sigma, cond, **kw: den(net, inp, sigma, cond, **kw), x, c, uc)
