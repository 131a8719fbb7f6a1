"""TEST INFRASTRUCTURE ONLY: torch-CPU stand-ins for the ops entry points the inpainting pipelines call on top of those of
tests/ops_emulation.py -- the two inpainting kernels (da_inpaint_blend, da_conv_in_inpaint) and the ends of the VAE encoder
(da_vae_conv_in_image, da_vae_posterior_latents, ops.add_noise, ops.conv_thin_out_moments) -- each with the C ABI's contract and the
kernels' rounding points.  The kernels themselves are tested on the GPU (tests/test_inpaint_gpu.py)."""
from __future__ import annotations

import torch

import ops_emulation as E

bf16 = torch.bfloat16


def _r(t):
    return t.to(bf16).float()


def add_noise(x, noise, a, b):
    return (_r(a * x.float()) + _r(b * noise.float())).to(bf16)


def inpaint_blend_(latents, image_latents, noise, mask, coef, step_idx):
    assert latents.shape == image_latents.shape == noise.shape and mask.shape[0] in (1, latents.shape[0]) and mask.shape[1] == 1
    assert coef.dim() == 2 and coef.shape[1] == 2 and coef.dtype == torch.float32 and 0 <= int(step_idx) < coef.shape[0]
    a, b = (float(v) for v in coef[int(step_idx)])
    p = _r(_r(a * image_latents.float()) + _r(b * noise.float()))
    m = mask.float()
    latents.copy_((_r(_r(1.0 - m) * p) + _r(m * latents.float())).to(bf16))
    return latents


def conv_in_inpaint(x, mask, masked, w, bias, *, table=None, step_idx=None, rep=1):
    B = x.shape[0]
    assert x.shape[1] == 4 and mask.shape[0] in (1, B) and mask.shape[1] == 1 and masked.shape[1] == 4 and w.shape[1] == 81
    xs = E.euler_scale_model_input(x, table, step_idx) if table is not None else x
    cat = torch.cat([xs, mask.expand(B, -1, -1, -1), masked.expand(B, -1, -1, -1)], 1).contiguous()
    return torch.cat([E.conv_thin_in(cat, w, bias, ksize=3, in_nchw=True)] * rep, 0)


def vae_conv_in_image(img, w, bias, *, nchw, normalize):
    x = img.float() / 255.0 if img.dtype == torch.uint8 else img.float()
    if not nchw:
        x = x.permute(0, 3, 1, 2)
    if normalize:
        x = 2.0 * x - 1.0
    return E.conv_thin_in(x.to(bf16).contiguous(), w, bias, ksize=3, in_nchw=True)


def conv_thin_out_moments(x, w, bias):
    y = E.conv_thin_out(x, w, bias)
    B, C, H, W_ = y.shape
    return y, (C * H * W_, H * W_, 1)


def vae_posterior_latents(x, strides, *, batch, hw, latent_channels, mode, wq=None, bq=None, eps1=None, eps2=None, shift=None,
                          scale=None, a=1.0, b=0.0):
    Lc = latent_channels
    cin = Lc if mode == 3 else 2 * Lc
    p = x.reshape(-1).as_strided((batch, cin, hw), tuple(int(s) for s in strides)).float()
    if wq is not None:
        p = _r(torch.einsum("ok,bkp->bop", wq.float(), p) + bq.float()[None, :, None])
    if mode == 0:
        return p.to(bf16).contiguous()
    if mode == 3:
        z = p
    else:
        z, logvar = p[:, :Lc], p[:, Lc:].clamp(-30.0, 20.0)
        if mode == 2:
            std = _r(torch.exp(_r(0.5 * logvar)))
            z = _r(z + _r(std * eps1.reshape(batch, Lc, hw).float()))
    if shift is not None:
        z = _r(z - shift)
    if scale is not None:
        z = _r(z * scale)
    if eps2 is not None:
        z = _r(_r(a * z) + _r(b * eps2.reshape(batch, Lc, hw).float()))
    return z.to(bf16).contiguous()


def install(monkeypatch, ops_module):
    """tests/ops_emulation.py's stand-ins plus the ones above."""
    E.install(monkeypatch, ops_module)
    for name in ("add_noise", "inpaint_blend_", "conv_in_inpaint", "vae_conv_in_image", "conv_thin_out_moments",
                 "vae_posterior_latents"):
        monkeypatch.setattr(ops_module, name, globals()[name])
