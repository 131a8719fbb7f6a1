"""``torch.library`` registrations of the C-ABI kernels: ``torch.ops.mi355x.*``.

The reference binds its native attention kernels exactly this way (models/attention_dispatch.py:746-816: a
``torch.library.custom_op`` with ``device_types="cuda"`` around the native entry point plus a ``register_fake`` shape
function), which is what makes an op visible to ``torch.compile`` / ``torch.export`` (the fake implementation gives the
tracer output shapes and dtypes without running the kernel) and callable from inside any reference module's ``forward``.
Each op below is the ctypes call of :mod:`diffusers_amd.ops` -- device pointers, sizes and the CURRENT stream go to
``libdiffusers_amd.so`` -- behind a functional signature (tensors in, new tensor out; nothing mutated except where the
name ends in ``_``).  Registration happens on import of this module (``import diffusers_amd.torch_ops``);
``diffusers_amd.ops`` itself stays free of it so the eager engine path has no dispatcher overhead.

    y = torch.ops.mi355x.gemm(x, w, bias, 0)                   # F.linear + fused activation
    y = torch.ops.mi355x.conv2d_nhwc(x, w, bias, 3, 1, False)  # F.conv2d on channels-last activations
    o = torch.ops.mi355x.flash_attn(q, k, v, scale)            # F.scaled_dot_product_attention, (B, S, H, D) layout
    y = torch.ops.mi355x.groupnorm(x, gamma, beta, 32, 1e-5, True)
    y = torch.ops.mi355x.layernorm(x, gamma, beta, 1e-5)
    x_next = torch.ops.mi355x.euler_step(eps, x, table, step_idx, True, 5.0, 0)
    x_next = torch.ops.mi355x.euler_ancestral_step(eps, x, noise, table, step_idx, True, 5.0, 0, 0)
    x_next, m1 = torch.ops.mi355x.dpmpp_2m_step(eps, x, m1, table, step_idx, begin_idx, True, 5.0, 0)
    fin, moments = torch.ops.mi355x.vae_moments_tile_blend(raw, sB, sC, sP, wq, bq, up, left, moments, 4, h, w, E, y0, x0, kh, kw)
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops

NAMESPACE = "mi355x"
bf16 = torch.bfloat16


@torch.library.custom_op(f"{NAMESPACE}::gemm", mutates_args=(), device_types="cuda")
def gemm(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act: int) -> torch.Tensor:
    """out[M][N] = act(x[M][K] @ w[N][K]^T + bias) -- nn.Linear (da_gemm_bf16, conv == 0); act = DA_ACT_* (GEGLU expects the
    packed weight of ops.pack_geglu and returns N / 2 columns)."""
    return ops.linear(x, w, bias, act=act)


@gemm.register_fake
def _(x, w, bias, act):
    n = w.shape[0] // 2 if act in (1, 6) else w.shape[0]   # DA_ACT_GEGLU / DA_ACT_GEGLU_TANH
    return x.new_empty((x.shape[0], n))


@torch.library.custom_op(f"{NAMESPACE}::conv2d_nhwc", mutates_args=(), device_types="cuda")
def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], ksize: int, stride: int,
                upsample2x: bool) -> torch.Tensor:
    """Implicit-GEMM Conv2d on channels-last [B][H][W][C] activations, weight [Cout][k*k*Cin] (ops.pack_conv_weight);
    ``upsample2x`` fuses F.interpolate(scale_factor=2, mode="nearest") into the gather."""
    return ops.conv2d_nhwc(x, w, bias, ksize=ksize, stride=stride, up=upsample2x)


@conv2d_nhwc.register_fake
def _(x, w, bias, ksize, stride, upsample2x):
    B, H, W_, _ = x.shape
    pad = (ksize - 1) // 2
    hv, wv = (2 * H, 2 * W_) if upsample2x else (H, W_)
    return x.new_empty((B, (hv + 2 * pad - ksize) // stride + 1, (wv + 2 * pad - ksize) // stride + 1, w.shape[0]))


@torch.library.custom_op(f"{NAMESPACE}::flash_attn", mutates_args=(), device_types="cuda")
def flash_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: Optional[float]) -> torch.Tensor:
    """softmax(scale * q k^T) v on (B, S, H, D) tensors -- the layout of the reference's attention backends
    (attention_dispatch.py:257-283); no mask, no dropout, not causal."""
    from .attention_backend import mi355x_flash_attention
    return mi355x_flash_attention(q, k, v, scale=scale)


@flash_attn.register_fake
def _(q, k, v, scale):
    return q.new_empty(q.shape)


@torch.library.custom_op(f"{NAMESPACE}::groupnorm", mutates_args=(), device_types="cuda")
def groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
              silu: bool) -> torch.Tensor:
    """nn.GroupNorm (+ SiLU) on channels-last [B][H][W][C] / [B][HW][C] activations."""
    return ops.group_norm_nhwc(x, gamma, beta, groups, eps, silu=silu)


@groupnorm.register_fake
def _(x, gamma, beta, groups, eps, silu):
    return torch.empty_like(x)


@torch.library.custom_op(f"{NAMESPACE}::layernorm", mutates_args=(), device_types="cuda")
def layernorm(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    """nn.LayerNorm over the last dim of a token matrix [M][C]."""
    return ops.layer_norm(x, gamma, beta, eps)


@layernorm.register_fake
def _(x, gamma, beta, eps):
    return torch.empty_like(x)


@torch.library.custom_op(f"{NAMESPACE}::euler_step", mutates_args=(), device_types="cuda")
def euler_step(model_output: torch.Tensor, sample: torch.Tensor, table: torch.Tensor, step_idx: torch.Tensor, cfg: bool,
               guidance_scale: float, pred_type: int) -> torch.Tensor:
    """EulerDiscreteScheduler.step (+ the CFG combine when ``cfg``: model_output = [uncond ; cond]) from the scheduler's
    device table; returns the new sample."""
    return ops.euler_step(model_output, sample, table, step_idx, cfg=cfg, guidance=guidance_scale, pred_type=pred_type)


@euler_step.register_fake
def _(model_output, sample, table, step_idx, cfg, guidance_scale, pred_type):
    return torch.empty_like(sample)


@torch.library.custom_op(f"{NAMESPACE}::dpmpp_2m_step", mutates_args=(), device_types="cuda")
def dpmpp_2m_step(model_output: torch.Tensor, sample: torch.Tensor, history: torch.Tensor, table: torch.Tensor,
                  step_idx: torch.Tensor, begin_idx: torch.Tensor, cfg: bool, guidance_scale: float,
                  pred_type: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """DPMSolverMultistepScheduler.step (DPM-Solver++ 2M; + the CFG combine when ``cfg``) from the scheduler's device table:
    returns (new sample, new fp32 history = this step's x0 prediction).  Functional form of the in-place kernel."""
    x, m1 = sample.contiguous().clone(), history.contiguous().clone()
    ops.dpmpp_2m_step_(model_output, x, m1, table, step_idx, begin_idx, cfg=cfg, guidance=guidance_scale, pred_type=pred_type)
    return x, m1


@dpmpp_2m_step.register_fake
def _(model_output, sample, history, table, step_idx, begin_idx, cfg, guidance_scale, pred_type):
    return torch.empty_like(sample), torch.empty_like(history)


@torch.library.custom_op(f"{NAMESPACE}::euler_ancestral_step", mutates_args=(), device_types="cuda")
def euler_ancestral_step(model_output: torch.Tensor, sample: torch.Tensor, noise: torch.Tensor, table: torch.Tensor,
                         step_idx: torch.Tensor, cfg: bool, guidance_scale: float, pred_type: int,
                         noise_step_stride: int) -> torch.Tensor:
    """EulerAncestralDiscreteScheduler.step (+ the CFG combine when ``cfg``) from the scheduler's device table and the step's
    pre-drawn noise (row ``step_idx`` of a table ``noise_step_stride`` elements apart; 0: one block); returns the new sample."""
    return ops.euler_ancestral_step(model_output, sample, noise, table, step_idx, cfg=cfg, guidance=guidance_scale,
                                    pred_type=pred_type, noise_step_stride=noise_step_stride)


@euler_ancestral_step.register_fake
def _(model_output, sample, noise, table, step_idx, cfg, guidance_scale, pred_type, noise_step_stride):
    return torch.empty_like(sample)


@torch.library.custom_op(f"{NAMESPACE}::vae_moments_tile_blend", mutates_args=(), device_types="cuda")
def vae_moments_tile_blend(src: torch.Tensor, stride_b: int, stride_c: int, stride_p: int, wq: Optional[torch.Tensor],
                           bq: Optional[torch.Tensor], up: Optional[torch.Tensor], left: Optional[torch.Tensor], moments: torch.Tensor,
                           latent_channels: int, height: int, width: int, extent: int, y0: int, x0: int, keep_h: int,
                           keep_w: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """One tile of a tiled AutoencoderKL.encode (da_vae_moments_tile_blend): quant_conv, the blends with the finished upper / left
    tiles, and the kept rectangle placed at (y0, x0) of the moments.  Returns (blended tile [B][2L][height][width], new moments).
    Functional form of the in-place kernel: ``moments`` is copied."""
    out = moments.contiguous().clone()
    fin = ops.vae_moments_tile_blend(src, (stride_b, stride_c, stride_p), batch=moments.shape[0], latent_channels=latent_channels,
                                     height=height, width=width, moments=out, y0=y0, x0=x0, keep_h=keep_h, keep_w=keep_w, wq=wq, bq=bq,
                                     extent=extent, up=up, left=left, want_fin=True)
    return fin, out


@vae_moments_tile_blend.register_fake
def _(src, stride_b, stride_c, stride_p, wq, bq, up, left, moments, latent_channels, height, width, extent, y0, x0, keep_h, keep_w):
    return moments.new_empty((moments.shape[0], 2 * latent_channels, height, width)), torch.empty_like(moments)


OPS = ("gemm", "conv2d_nhwc", "flash_attn", "groupnorm", "layernorm", "euler_step", "dpmpp_2m_step", "euler_ancestral_step",
       "vae_moments_tile_blend")
