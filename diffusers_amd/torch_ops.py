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
    hidden, skip = torch.ops.mi355x.freeu(hidden, skip, 0.9, 1.3)  # apply_freeu, channels-last
    o = torch.ops.mi355x.temporal_attn(q, k, v, 16, 8, None)      # attention over the frame axis of [B, F, HW, C] tokens, in place
    torch.ops.mi355x.ip_attn(o, q, [k_ip], [v_ip], [4], [0.6], 20, None)      # IP-Adapter image branch, added onto `o` in place
    small = torch.ops.mi355x.resample_u8(img_u8_nhwc, 768, 1024, "lanczos")   # PIL.Image.resize, to the bit
    small = torch.ops.mi355x.gather_resize(img, 768, 1024, True)              # F.interpolate (nearest), NCHW
    q, s = torch.ops.mi355x.quantize_rows_fp8(x)                              # per-row e4m3 + fp32 scale
    y = torch.ops.mi355x.gemm_fp8(q, s, w_q, w_s, bias, 0)                    # F.linear on the fp8 MFMA
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

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


@torch.library.custom_op(f"{NAMESPACE}::freeu", mutates_args=(), device_types="cuda")
def freeu(hidden: torch.Tensor, skip: torch.Tensor, s: float, b: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's apply_freeu on channels-last [B][H][W][C] tensors (da_freeu_nhwc_bf16): returns (hidden with its first half of
    the channels scaled by ``b``, skip with its four lowest Fourier bins scaled by ``s``).  Functional form of the kernel, which
    scales ``hidden`` in place: ``hidden`` is copied."""
    h = hidden.contiguous().clone()
    return h, ops.freeu(h, skip.contiguous(), s=s, b=b)


@freeu.register_fake
def _(hidden, skip, s, b):
    return torch.empty_like(hidden), torch.empty_like(skip)


@torch.library.custom_op(f"{NAMESPACE}::temporal_attn", mutates_args=(), device_types="cuda")
def temporal_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_frames: int, heads: int, scale: Optional[float]) -> torch.Tensor:
    """Self-attention over the frame axis (da_attention_temporal_bf16): ``q`` / ``k`` / ``v`` are [B*F][HW][C] bf16, frame-major
    (row (b*F + f)*HW + p), last dim contiguous and the first two dims mergeable (stride(0) == HW * stride(1)) -- the column blocks of
    one fused projection output are taken as they are; nothing is copied.  Every (pixel, head) attends over its ``num_frames`` frames.
    A 2-D token matrix does not say what HW is and is refused; so is an operand that would need a copy.  Returns a contiguous tensor
    of q's shape."""
    if q.dim() != 3 or q.shape[0] % num_frames or q.shape[2] % heads:
        raise ValueError(f"temporal_attn: q must be [B*{num_frames}][HW][{heads}*D] (3-D: a 2-D token matrix does not carry HW), got "
                         f"{tuple(q.shape)}")
    BF, HW, C_ = q.shape

    def flat(t, name):
        if tuple(t.shape) != (BF, HW, C_) or t.stride(2) != 1 or (HW > 1 and BF > 1 and t.stride(0) != HW * t.stride(1)):
            raise ValueError(f"temporal_attn: {name} must be a [{BF}][{HW}][{C_}] view with a contiguous last dim and stride(0) == HW * "
                             f"stride(1) (it is not copied), got shape {tuple(t.shape)} strides {t.stride()}")
        ld = t.stride(1) if HW > 1 else (t.stride(0) if BF > 1 else C_)
        return t.as_strided((BF * HW, C_), (ld, 1), t.storage_offset())
    out = ops.temporal_attention(flat(q, "q"), flat(k, "k"), flat(v, "v"), B=BF // num_frames, F=num_frames, HW=HW, H=heads,
                                 D=C_ // heads, scale=scale)
    return out.view(q.shape)


@temporal_attn.register_fake
def _(q, k, v, num_frames, heads, scale):
    return q.new_empty(q.shape)


@torch.library.custom_op(f"{NAMESPACE}::ip_attn", mutates_args=("out",), device_types="cuda")
def ip_attn(out: torch.Tensor, q: torch.Tensor, ks: Sequence[torch.Tensor], vs: Sequence[torch.Tensor], num_tokens: Sequence[int],
            scales: Sequence[float], heads: int, scale: Optional[float]) -> None:
    """The image branch of IP-Adapter's decoupled cross-attention (da_attention_ip_bf16), added onto ``out`` IN PLACE:
    ``out += sum_a scales[a] * softmax(scale * q ks[a]^T) vs[a]``.  ``out`` / ``q``: [B][Sq][heads*D] bf16 with a contiguous last dim
    and mergeable leading dims; ``ks[a]`` / ``vs[a]``: [B][N_alloc_a][heads*D], token-major, the first ``num_tokens[a]`` tokens of a
    batch valid.  Nothing is copied: an operand that would need a copy is refused.  The one op of this module that mutates an
    argument (``IN_PLACE_OPS``); its schema says so."""
    if q.dim() != 3 or out.shape != q.shape or q.shape[2] % heads or not len(ks) == len(vs) == len(num_tokens) == len(scales):
        raise ValueError(f"ip_attn: out / q must be [B][Sq][{heads}*D] and ks / vs / num_tokens / scales of one length, got "
                         f"{tuple(out.shape)} / {tuple(q.shape)} and {len(ks)} / {len(vs)} / {len(num_tokens)} / {len(scales)}")
    B, Sq, C_ = q.shape

    def flat(t, name, rows):
        if tuple(t.shape) != (B, rows, C_) or t.stride(2) != 1 or (rows > 1 and B > 1 and t.stride(0) != rows * t.stride(1)):
            raise ValueError(f"ip_attn: {name} must be a [{B}][{rows}][{C_}] view with a contiguous last dim and stride(0) == rows * "
                             f"stride(1) (it is not copied), got shape {tuple(t.shape)} strides {t.stride()}")
        ld = t.stride(1) if rows > 1 else (t.stride(0) if B > 1 else C_)
        return t.as_strided((B * rows, C_), (ld, 1), t.storage_offset())
    adapters = [(flat(k, f"ks[{a}]", k.shape[1]), flat(v, f"vs[{a}]", k.shape[1]), int(n), k.shape[1], float(s))
                for a, (k, v, n, s) in enumerate(zip(ks, vs, num_tokens, scales))]
    ops.ip_attention_accumulate(flat(out, "out", Sq), flat(q, "q", Sq), adapters, B=B, H=heads, D=C_ // heads, Sq=Sq, scale=scale)


@ip_attn.register_fake
def _(out, q, ks, vs, num_tokens, scales, heads, scale):
    return None


@torch.library.custom_op(f"{NAMESPACE}::resample_u8", mutates_args=(), device_types="cuda")
def resample_u8(src: torch.Tensor, height: int, width: int, resample: str) -> torch.Tensor:
    """PIL.Image.resize((width, height), resample) of packed uint8 [B][H][W][C] images, C = 1 or 3, to the bit (da_resample_u8);
    ``resample``: 'lanczos', 'bicubic' or 'bilinear'."""
    return ops.resample_u8(src.contiguous(), (height, width), resample)


@resample_u8.register_fake
def _(src, height, width, resample):
    return src.new_empty((src.shape[0], height, width, src.shape[3]))


@torch.library.custom_op(f"{NAMESPACE}::gather_resize", mutates_args=(), device_types="cuda")
def gather_resize(src: torch.Tensor, height: int, width: int, nchw: bool) -> torch.Tensor:
    """F.interpolate(src, (height, width)) (nearest) of an fp32 or uint8 image batch, NCHW or NHWC (da_gather_resize)."""
    return ops.gather_resize(src.contiguous(), (height, width), nchw=nchw)


@gather_resize.register_fake
def _(src, height, width, nchw):
    B = src.shape[0]
    return src.new_empty((B, src.shape[1], height, width) if nchw else (B, height, width, src.shape[3]))


@torch.library.custom_op(f"{NAMESPACE}::quantize_rows_fp8", mutates_args=(), device_types="cuda")
def quantize_rows_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row e4m3 quantisation of a bf16 matrix [R][K] (da_quantize_rows_e4m3): returns (q float8_e4m3fn [R][K], scale fp32 [R])."""
    return ops.quantize_rows_fp8(x)


@quantize_rows_fp8.register_fake
def _(x):
    return x.new_empty(x.shape, dtype=torch.float8_e4m3fn), x.new_empty((x.shape[0],), dtype=torch.float32)


@torch.library.custom_op(f"{NAMESPACE}::gemm_fp8", mutates_args=(), device_types="cuda")
def gemm_fp8(a_q: torch.Tensor, a_scale: torch.Tensor, w_q: torch.Tensor, w_scale: torch.Tensor, bias: Optional[torch.Tensor],
             act: int) -> torch.Tensor:
    """out[M][N] = act(a_scale[m] w_scale[n] (a_q[M][K] @ w_q[N][K]^T) + bias), bf16, on the fp8 MFMA (da_gemm_fp8); act = DA_ACT_NONE
    or DA_ACT_GELU_TANH."""
    return ops.linear_fp8(a_q, a_scale, w_q, w_scale, bias, act=act)


@gemm_fp8.register_fake
def _(a_q, a_scale, w_q, w_scale, bias, act):
    return a_q.new_empty((a_q.shape[0], w_q.shape[0]), dtype=bf16)


OPS = ("gemm", "conv2d_nhwc", "flash_attn", "groupnorm", "layernorm", "euler_step", "dpmpp_2m_step", "euler_ancestral_step",
       "vae_moments_tile_blend", "freeu", "temporal_attn", "resample_u8", "gather_resize", "quantize_rows_fp8", "gemm_fp8")
IN_PLACE_OPS = ("ip_attn",)    # accumulate into their first argument; OPS above are the functional ones
