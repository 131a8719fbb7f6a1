"""TEST INFRASTRUCTURE ONLY for the ControlNet tests.

1. torch-CPU stand-ins for the ``diffusers_amd.ops`` entry points ControlNet adds to the ones of tests/ops_emulation.py: the
   ``gate`` / ``gate_round`` keywords of ``conv2d_nhwc`` and ``linear`` (da_gemm_params.gate_f32 == 2) and ``vae_conv_in_image``.
2. A plain torch restatement of the reference ``ControlNetModel.forward`` (models/controlnets/controlnet.py) and of
   ``UNet2DConditionModel.forward`` WITH its ControlNet residuals (unet_2d_condition.py:979-1235), written here from the reference's
   definition: functional torch on a reference-format ``state_dict``, in whatever dtype the tensors have (fp32 = the oracle,
   bf16 on the CPU = the measured error floor of the number format), plus fp32 oracle loops of the two samplers the factory
   pipelines use.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import ops_emulation as E

bf16 = torch.bfloat16


# ----------------------------------------------------------------------------------------------------------------------
# 1. stand-ins
# ----------------------------------------------------------------------------------------------------------------------
def _gated(y, gate, gate_round, bidx_shape, residual, out, out_scale):
    """The epilogue after the bf16-rounded projection ``y``: gate (three rounding modes), residual, store."""
    g = gate.float().reshape(bidx_shape)
    y = y.float() * g
    if gate.dtype == bf16 or gate_round:
        assert gate.dtype == bf16 or gate.dtype == torch.float32
        y = y.to(bf16).float()
    if residual is not None:
        y = y + residual.float()
    return E._store(y * out_scale, out)


def conv2d_nhwc(x, w, bias=None, *, gate=None, gate_round=False, residual=None, out=None, out_scale=1.0, **kw):
    if gate is None:
        assert not gate_round
        return E.conv2d_nhwc(x, w, bias, residual=residual, out=out, out_scale=out_scale, **kw)
    assert not gate_round or (gate.dtype == torch.float32 and kw.get("ksize", 3) == 1), "C ABI: gate_f32 == 2 is conv 0 / 1"
    y = E.conv2d_nhwc(x, w, bias, **kw)
    assert tuple(gate.shape) == (y.shape[0], y.shape[3]) and gate.stride(1) == 1 and gate.stride(0) % 4 == 0
    if residual is not None:
        assert tuple(residual.shape) == tuple(y.shape) and residual.is_contiguous()
    return _gated(y, gate, gate_round, (y.shape[0], 1, 1, y.shape[3]), residual, out, out_scale)


def linear(x, w, bias=None, *, gate_round=False, **kw):
    if not gate_round:
        return E.linear(x, w, bias, **kw)
    gate, residual, out = kw.pop("gate"), kw.pop("residual", None), kw.pop("out", None)
    out_scale, rpb = kw.pop("out_scale", 1.0), kw.get("rows_per_batch", 0)
    assert gate.dtype == torch.float32 and rpb > 0
    y = E.linear(x, w, bias, **kw)
    bidx = torch.arange(y.shape[0]) // rpb
    return _gated(y, gate[bidx], True, y.shape, residual, out, out_scale)


def vae_conv_in_image(img, w, bias, *, nchw, normalize):
    """da_vae_conv_in_image: uint8 is x / 255, optional 2x - 1, the pipeline's bf16 cast, conv 3 -> Cout, NHWC bf16 out."""
    assert img.dtype in (torch.float32, torch.uint8) and img.is_contiguous() and (img.dtype != torch.uint8 or not nchw)
    x = img.float() / 255.0 if img.dtype == torch.uint8 else img
    x = x if nchw else x.permute(0, 3, 1, 2)
    if normalize:
        x = 2.0 * x - 1.0
    x = x.to(bf16).float()
    co = w.shape[0]
    assert x.shape[1] == 3 and w.shape[1] == 27
    y = F.conv2d(x, w.float().view(co, 3, 3, 3).permute(0, 3, 1, 2), None if bias is None else bias.float(), padding=1)
    return y.permute(0, 2, 3, 1).to(bf16).contiguous()


def install(monkeypatch, ops_module):
    E.install(monkeypatch, ops_module)
    for name in ("conv2d_nhwc", "linear", "vae_conv_in_image"):
        monkeypatch.setattr(ops_module, name, globals()[name])


# ----------------------------------------------------------------------------------------------------------------------
# 2. the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _tup(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


def _sinusoid(t, dim, flip, shift):
    half = dim // 2
    freq = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / (half - shift))
    a = t.float()[:, None] * freq[None]
    e = torch.cat([torch.sin(a), torch.cos(a)], -1)
    return torch.cat([e[:, half:], e[:, :half]], -1) if flip else e


def _mlp(sd, p, x):
    return F.linear(F.silu(F.linear(x, sd[p + ".linear_1.weight"], sd[p + ".linear_1.bias"])), sd[p + ".linear_2.weight"],
                    sd[p + ".linear_2.bias"])


def _resnet(sd, p, x, emb, groups, eps, scale=1.0):
    h = F.conv2d(F.silu(F.group_norm(x, groups, sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], eps)), sd[p + ".conv1.weight"],
                 sd[p + ".conv1.bias"], padding=1)
    h = h + F.linear(F.silu(emb), sd[p + ".time_emb_proj.weight"], sd[p + ".time_emb_proj.bias"])[:, :, None, None]
    h = F.conv2d(F.silu(F.group_norm(h, groups, sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], eps)), sd[p + ".conv2.weight"],
                 sd[p + ".conv2.bias"], padding=1)
    if p + ".conv_shortcut.weight" in sd:
        x = F.conv2d(x, sd[p + ".conv_shortcut.weight"], sd[p + ".conv_shortcut.bias"])
    return (x + h) / scale


def _attn(sd, p, x, ctx, heads):
    q, k, v = (F.linear(t, sd[f"{p}.to_{n}.weight"]) for n, t in (("q", x), ("k", ctx), ("v", ctx)))
    B, S, C = q.shape
    q, k, v = (t.view(B, -1, heads, C // heads).transpose(1, 2) for t in (q, k, v))
    o = torch.softmax(q @ k.transpose(-1, -2) * (C // heads) ** -0.5, dim=-1) @ v
    return F.linear(o.transpose(1, 2).reshape(B, S, C), sd[p + ".to_out.0.weight"], sd[p + ".to_out.0.bias"])


def _transformer(sd, p, x, ctx, heads, layers, groups, lin):
    B, C, H, W = x.shape
    h = F.group_norm(x, groups, sd[p + ".norm.weight"], sd[p + ".norm.bias"], 1e-6)
    if lin:
        h = F.linear(h.permute(0, 2, 3, 1).reshape(B, H * W, C), sd[p + ".proj_in.weight"], sd[p + ".proj_in.bias"])
    else:
        h = F.conv2d(h, sd[p + ".proj_in.weight"], sd[p + ".proj_in.bias"]).permute(0, 2, 3, 1).reshape(B, H * W, C)
    for k in range(layers):
        b = f"{p}.transformer_blocks.{k}"
        n = F.layer_norm(h, (C,), sd[b + ".norm1.weight"], sd[b + ".norm1.bias"])
        h = h + _attn(sd, b + ".attn1", n, n, heads)
        n = F.layer_norm(h, (C,), sd[b + ".norm2.weight"], sd[b + ".norm2.bias"])
        h = h + _attn(sd, b + ".attn2", n, ctx, heads)
        n = F.layer_norm(h, (C,), sd[b + ".norm3.weight"], sd[b + ".norm3.bias"])
        val, gate = F.linear(n, sd[b + ".ff.net.0.proj.weight"], sd[b + ".ff.net.0.proj.bias"]).chunk(2, dim=-1)
        h = h + F.linear(val * F.gelu(gate), sd[b + ".ff.net.2.weight"], sd[b + ".ff.net.2.bias"])
    if lin:
        h = F.linear(h, sd[p + ".proj_out.weight"], sd[p + ".proj_out.bias"]).reshape(B, H, W, C).permute(0, 3, 1, 2)
    else:
        h = F.conv2d(h.reshape(B, H, W, C).permute(0, 3, 1, 2), sd[p + ".proj_out.weight"], sd[p + ".proj_out.bias"])
    return h + x


def _embedding(sd, cfg, sample, timestep, added):
    dt, B = sample.dtype, sample.shape[0]
    t = torch.as_tensor(timestep, dtype=torch.float32).reshape(-1)
    t = t.expand(B) if t.numel() == 1 else t
    emb = _mlp(sd, "time_embedding", _sinusoid(t, cfg["block_out_channels"][0], cfg["flip_sin_to_cos"], cfg["freq_shift"]).to(dt))
    if cfg["addition_embed_type"] == "text_time":
        ids = _sinusoid(added["time_ids"].flatten(), cfg["addition_time_embed_dim"], cfg["flip_sin_to_cos"], cfg["freq_shift"])
        add = torch.cat([added["text_embeds"].float(), ids.reshape(B, -1)], -1).to(dt)
        emb = emb + _mlp(sd, "add_embedding", add)
    return emb


def _encoder(sd, cfg, x, emb, ctx):
    """down blocks + mid block on ``x`` (conv_in already applied): (skip list, mid output)."""
    boc = tuple(cfg["block_out_channels"])
    n = len(boc)
    groups, eps, lin = cfg["norm_num_groups"], cfg["norm_eps"], cfg["use_linear_projection"]
    heads = _tup(cfg.get("num_attention_heads") or cfg["attention_head_dim"], n)
    lpb, tlpb = _tup(cfg["layers_per_block"], n), _tup(cfg["transformer_layers_per_block"], n)
    skips = [x]
    for i, bt in enumerate(cfg["down_block_types"]):
        for j in range(lpb[i]):
            x = _resnet(sd, f"down_blocks.{i}.resnets.{j}", x, emb, groups, eps)
            if bt == "CrossAttnDownBlock2D":
                x = _transformer(sd, f"down_blocks.{i}.attentions.{j}", x, ctx, heads[i], tlpb[i], groups, lin)
            skips.append(x)
        if i != n - 1:
            x = F.conv2d(x, sd[f"down_blocks.{i}.downsamplers.0.conv.weight"], sd[f"down_blocks.{i}.downsamplers.0.conv.bias"],
                         stride=2, padding=1)
            skips.append(x)
    sc = cfg["mid_block_scale_factor"]
    x = _resnet(sd, "mid_block.resnets.0", x, emb, groups, eps, sc)
    x = _transformer(sd, "mid_block.attentions.0", x, ctx, heads[-1], tlpb[-1], groups, lin)
    return skips, _resnet(sd, "mid_block.resnets.1", x, emb, groups, eps, sc)


def controlnet_forward(sd, cfg, sample, timestep, ctx, cond_image, scale=1.0, added=None):
    """ControlNetModel.forward: ``(down residuals, mid residual)``, NCHW, multiplied by ``scale`` (a Python float)."""
    emb = _embedding(sd, cfg, sample, timestep, added)
    x = F.conv2d(sample, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    e = "controlnet_cond_embedding"
    c = F.silu(F.conv2d(cond_image, sd[e + ".conv_in.weight"], sd[e + ".conv_in.bias"], padding=1))
    for k in range(2 * (len(cfg["conditioning_embedding_out_channels"]) - 1)):
        c = F.silu(F.conv2d(c, sd[f"{e}.blocks.{k}.weight"], sd[f"{e}.blocks.{k}.bias"], padding=1, stride=1 + (k & 1)))
    x = x + F.conv2d(c, sd[e + ".conv_out.weight"], sd[e + ".conv_out.bias"], padding=1)
    skips, mid = _encoder(sd, cfg, x, emb, ctx)
    down = [F.conv2d(s, sd[f"controlnet_down_blocks.{k}.weight"], sd[f"controlnet_down_blocks.{k}.bias"]) * scale
            for k, s in enumerate(skips)]
    return down, F.conv2d(mid, sd["controlnet_mid_block.weight"], sd["controlnet_mid_block.bias"]) * scale


def unet_forward(sd, cfg, sample, timestep, ctx, added=None, down_res=None, mid_res=None):
    """UNet2DConditionModel.forward with ``down_block_additional_residuals`` / ``mid_block_additional_residual``."""
    boc = tuple(cfg["block_out_channels"])
    n = len(boc)
    groups, eps, lin = cfg["norm_num_groups"], cfg["norm_eps"], cfg["use_linear_projection"]
    heads = tuple(reversed(_tup(cfg.get("num_attention_heads") or cfg["attention_head_dim"], n)))
    lpb = tuple(reversed(_tup(cfg["layers_per_block"], n)))
    rt = cfg.get("reverse_transformer_layers_per_block")
    tlpb = tuple(reversed(_tup(cfg["transformer_layers_per_block"], n))) if rt is None else _tup(rt, n)
    emb = _embedding(sd, cfg, sample, timestep, added)
    skips, x = _encoder(sd, cfg, F.conv2d(sample, sd["conv_in.weight"], sd["conv_in.bias"], padding=1), emb, ctx)
    if down_res is not None:
        skips = [s + r for s, r in zip(skips, down_res)]
        x = x + mid_res
    for i, bt in enumerate(cfg["up_block_types"]):
        for j in range(lpb[i] + 1):
            x = _resnet(sd, f"up_blocks.{i}.resnets.{j}", torch.cat([x, skips.pop()], 1), emb, groups, eps)
            if bt == "CrossAttnUpBlock2D":
                x = _transformer(sd, f"up_blocks.{i}.attentions.{j}", x, ctx, heads[i], tlpb[i], groups, lin)
        if i != n - 1:
            x = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), sd[f"up_blocks.{i}.upsamplers.0.conv.weight"],
                         sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], padding=1)
    x = F.silu(F.group_norm(x, groups, sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], eps))
    return F.conv2d(x, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def rel_rms(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-30))


def psnr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float(10 * torch.log10((b.max() - b.min()) ** 2 / (a - b).pow(2).mean().clamp_min(1e-30)))


def oracle_loop(kind, scheduler_cfg, steps, guidance, latents, predict):
    """fp32 denoising loop of the factory pipelines' samplers -- ``kind`` "euler" (EulerDiscreteScheduler, leading spacing,
    epsilon) or "ddim" (eta 0, leading spacing, steps_offset, set_alpha_to_one False) -- around ``predict(x_in [2B], t)`` with
    the negative half in front; returns the final latents.  ``latents`` are unit-variance noise (scaled here by
    init_noise_sigma)."""
    T = 1000
    betas = torch.linspace(scheduler_cfg["beta_start"] ** 0.5, scheduler_cfg["beta_end"] ** 0.5, T, dtype=torch.float64) ** 2
    ac = torch.cumprod(1.0 - betas, 0)
    ratio = T // steps
    ts = (torch.arange(steps, dtype=torch.float64) * ratio).round().flip(0).long() + scheduler_cfg.get("steps_offset", 0)
    x = latents.double()
    if kind == "euler":
        sig_all = ((1 - ac) / ac) ** 0.5
        sig = torch.cat([sig_all[ts], torch.zeros(1, dtype=torch.float64)])
        x = x * (sig[0] ** 2 + 1) ** 0.5          # init_noise_sigma for "leading" spacing
        for i, t in enumerate(ts):
            xin = (x / (sig[i] ** 2 + 1) ** 0.5).float()
            u, c = predict(torch.cat([xin, xin]), float(t)).double().chunk(2)
            x = x + (u + guidance * (c - u)) * (sig[i + 1] - sig[i])
        return x.float()
    assert kind == "ddim"
    for t in ts:
        xin = x.float()
        u, c = predict(torch.cat([xin, xin]), float(t)).double().chunk(2)
        eps = u + guidance * (c - u)
        a_t = ac[t]
        prev = t - ratio
        a_p = ac[prev] if prev >= 0 else ac[0]
        x0 = (x - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
        x = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * eps
    return x.float()
