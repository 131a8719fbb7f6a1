"""TEST INFRASTRUCTURE ONLY: torch-CPU stand-ins for what the FLUX img2img / inpainting pipelines call on top of
tests/inpaint_emulation.py -- ops.flux_prepare_latents (da_flux_prepare_latents) and the 32-channel route of
ops.conv_thin_out_moments -- with the C ABI's contract and the kernel's rounding points, and restatements of the reference semantics
the pipelines follow (the reference package is not importable on the build machine):

  FluxPipeline._pack_latents                       pipelines/flux/pipeline_flux.py
  FluxImg2ImgPipeline.get_timesteps / prepare_latents / _encode_vae_image
                                                   pipelines/flux/pipeline_flux_img2img.py
  FluxInpaintPipeline.prepare_mask_latents and the blend of its loop
                                                   pipelines/flux/pipeline_flux_inpaint.py
  FlowMatchEulerDiscreteScheduler.scale_noise      schedulers/scheduling_flow_match_euler_discrete.py

The kernels themselves are tested on the GPU (tests/test_flux_img2img_gpu.py)."""
from __future__ import annotations

import torch

import inpaint_emulation as I
import ops_emulation as E

bf16 = torch.bfloat16
MEAN, SAMPLE, NOISE = 1, 2, 3


# ---- restatements of the reference ------------------------------------------------------------------------------------------
def pack_latents(latents):
    """FluxPipeline._pack_latents: (B, C, H, W) -> (B, (H/2)(W/2), 4 C), column c * 4 + di * 2 + dj <- (c, 2 i + di, 2 j + dj)."""
    B, C, H, W = latents.shape
    x = latents.view(B, C, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5)
    return x.reshape(B, (H // 2) * (W // 2), C * 4)


def get_timesteps_ref(num_inference_steps, strength):
    """FluxImg2ImgPipeline.get_timesteps: ``(number of steps, begin index)`` -- no int() around the product."""
    init_timestep = min(num_inference_steps * strength, num_inference_steps)
    t_start = int(max(num_inference_steps - init_timestep, 0))
    return num_inference_steps - t_start, t_start


def scale_noise_ref(sample, sigma, noise):
    """FlowMatchEulerDiscreteScheduler.scale_noise on tensors of one dtype: ``sigma`` is the scheduler's fp32 sigma, cast to the
    sample's dtype first (``sigmas = self.sigmas.to(device=sample.device, dtype=sample.dtype)``), then the torch expression."""
    sigma = torch.as_tensor(sigma, dtype=torch.float32).to(device=sample.device, dtype=sample.dtype).flatten()
    while len(sigma.shape) < len(sample.shape):
        sigma = sigma.unsqueeze(-1)
    return sigma * noise + (1.0 - sigma) * sample


def blend_ref(mask, init_latents_proper, latents):
    """The reference loop's ``latents = (1 - init_mask) * init_latents_proper + init_mask * latents`` (bf16 torch ops)."""
    return (1 - mask) * init_latents_proper + mask * latents


# ---- stand-ins ----------------------------------------------------------------------------------------------------------------
def _r(t):
    return t.to(bf16).float()


def flux_prepare_latents(x, strides, *, batch, height, width, latent_channels, mode, noise, eps1=None, shift=None, scale=None,
                         a=0.0, b=1.0, want_image_latents=False, want_noise=False):
    Lc, hw = latent_channels, height * width
    assert mode in (MEAN, SAMPLE, NOISE) and height % 2 == 0 and width % 2 == 0 and (mode == SAMPLE) == (eps1 is not None)
    assert noise.dtype == bf16 and noise.numel() == batch * Lc * hw
    cin = Lc if mode == NOISE else 2 * Lc
    p = x.reshape(-1).as_strided((batch, cin, hw), tuple(int(s) for s in strides)).float()
    z = p[:, :Lc]
    if mode == SAMPLE:
        logvar = p[:, Lc:].clamp(-30.0, 20.0)
        std = _r(torch.exp(_r(0.5 * logvar)))
        z = _r(z + _r(std * eps1.reshape(batch, Lc, hw).float()))
    if shift is not None:
        z = _r(z - shift)
    if scale is not None:
        z = _r(z * scale)
    n = noise.reshape(batch, Lc, hw).float()
    xx = _r(_r(a * z) + _r(b * n))
    pk = lambda t: pack_latents(t.to(bf16).reshape(batch, Lc, height, width).contiguous()).contiguous()   # noqa: E731
    return pk(xx), pk(z) if want_image_latents else None, pk(n) if want_noise else None


def conv_thin_out_moments(x, w, bias):
    if w.shape[0] > 16:                                   # the implicit-GEMM conv as it is: NHWC, no padding
        y = E.conv2d_nhwc(x, w, bias, ksize=3)
        B, H, W_, C = y.shape
        return y, (H * W_ * C, 1, C)
    return I.conv_thin_out_moments(x, w, bias)


def install(monkeypatch, ops_module):
    """tests/inpaint_emulation.py's stand-ins plus the ones above."""
    I.install(monkeypatch, ops_module)
    for name in ("flux_prepare_latents", "conv_thin_out_moments"):
        monkeypatch.setattr(ops_module, name, globals()[name])
