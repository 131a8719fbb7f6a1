"""IP-Adapter (https://arxiv.org/abs/2308.06721) on the engine: the checkpoint's key numbering, the image projection, loading into a
``UNet2DConditionModel`` and the image keys / values of a call.  The attention itself is ``layers.Attention`` (``attach_ip``,
``precompute_ip_kv``) on ``ops.ip_attention_accumulate`` (csrc/attention_ip.hip).  The plus checkpoints project with a perceiver
:class:`Resampler` (models/embeddings.py ``IPAdapterPlusImageProjection``) on ``ops.resampler_attention``
(csrc/attention_resampler.hip); the per-step half is the same.

Reference: loaders/unet.py ``_convert_ip_adapter_attn_to_diffusers`` / ``_load_ip_adapter_weights`` (a checkpoint is
``{"image_proj": {...}, "ip_adapter": {"1.to_k_ip.weight": ..., "1.to_v_ip.weight": ..., "3.to_k_ip.weight": ...}}``: the number
walks ``unet.attn_processors`` -- down blocks, up blocks, mid block, the order the reference registers its modules in -- two per
transformer block, and only the odd ones, the cross-attentions, carry weights), models/embeddings.py ``ImageProjection`` and
``MultiIPAdapterImageProjection``, loaders/ip_adapter.py ``IPAdapterMixin``."""
from __future__ import annotations

import itertools
from pathlib import Path
from typing import Dict, List

import torch

from . import _lib as L
from . import ops
from .layers import pad_encoder_states
from .unet_blocks import _tup

bf16 = torch.bfloat16
_GENERATION = itertools.count(1)
MAX_TOKENS = 32      # keys of one adapter in da_attention_ip_bf16
_RESAMPLER_KEYS = ("latents", "proj_in.weight", "perceiver_resampler.proj_in.weight", "norm.weight_face")


def cross_attention_widths(config) -> List[int]:
    """Hidden size of every cross-attention layer in checkpoint order (down, up, mid); layer ``i`` has key ``2 * i + 1``."""
    c = config
    n = len(c["block_out_channels"])
    boc, lpb, tlpb = tuple(c["block_out_channels"]), _tup(c["layers_per_block"], n), _tup(c.get("transformer_layers_per_block", 1), n)
    rt = c.get("reverse_transformer_layers_per_block")
    rtlpb = tuple(reversed(tlpb)) if rt is None else _tup(rt, n)
    down = [boc[i] for i, t in enumerate(c["down_block_types"]) if t == "CrossAttnDownBlock2D" for _ in range(lpb[i] * tlpb[i])]
    rboc, rlpb = tuple(reversed(boc)), tuple(reversed(lpb))
    up = [rboc[i] for i, t in enumerate(c["up_block_types"]) if t == "CrossAttnUpBlock2D" for _ in range((rlpb[i] + 1) * rtlpb[i])]
    return down + up + [boc[-1]] * tlpb[-1]


def ip_adapter_param_shapes(config, num_tokens: int = 4, image_embed_dim: int = 1024) -> Dict[str, tuple]:
    """Shapes of a plain (ImageProjection) IP-Adapter checkpoint for a U-Net config, flat with ``image_proj.`` / ``ip_adapter.``
    prefixes as the safetensors files store them."""
    cross = config["cross_attention_dim"]
    shapes = {"image_proj.proj.weight": (num_tokens * cross, image_embed_dim), "image_proj.proj.bias": (num_tokens * cross,),
              "image_proj.norm.weight": (cross,), "image_proj.norm.bias": (cross,)}
    for i, width in enumerate(cross_attention_widths(config)):
        shapes[f"ip_adapter.{2 * i + 1}.to_k_ip.weight"] = shapes[f"ip_adapter.{2 * i + 1}.to_v_ip.weight"] = (width, cross)
    return shapes


def nest(flat: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]:
    """``image_proj.*`` / ``ip_adapter.*`` keys -> the reference's two-level dict (a dict that has the two levels passes through)."""
    if "image_proj" in flat and "ip_adapter" in flat:
        return flat
    out = {"image_proj": {}, "ip_adapter": {}}
    for k, v in flat.items():
        head, _, rest = k.partition(".")
        if head not in out:
            raise ValueError(f"IP-Adapter checkpoint: unexpected key {k!r} (expected image_proj.* / ip_adapter.*)")
        out[head][rest] = v
    return out


def read_ip_adapter(source, subfolder=None, weight_name=None) -> Dict[str, Dict[str, torch.Tensor]]:
    """A checkpoint dict, or a local ``.safetensors`` file (``source[/subfolder]/weight_name``, or the file itself)."""
    if isinstance(source, dict):
        return nest(source)
    p = Path(source)
    if p.is_dir():
        if weight_name is None:
            raise ValueError("load_ip_adapter: `weight_name` is required with a directory")
        p = p / (subfolder or "") / weight_name
    if p.suffix != ".safetensors" or not p.is_file():
        raise OSError(f"load_ip_adapter: {p} is not a local .safetensors file (the engine neither downloads nor unpickles)")
    from safetensors.torch import load_file
    return nest(load_file(str(p)))


class ImageProjection:
    """models/embeddings.py ImageProjection: Linear(emb, num_tokens * cross_dim), reshape, LayerNorm -- the skinny linear and the
    LayerNorm kernel, once per call.  ``[B][n_img][emb]`` -> ``[B][n_img * num_tokens][cross_dim]`` (MultiIPAdapterImageProjection
    folds the images of a sample into the batch and back; their tokens end up adjacent)."""

    def __init__(self, sd: Dict[str, torch.Tensor], cross_dim: int, device):
        if any(k in sd for k in _RESAMPLER_KEYS) or "proj.weight" not in sd:
            raise NotImplementedError("IP-Adapter Resampler projections (the 'plus' / FaceID checkpoints) are not built: only the "
                                      "ImageProjection of the base checkpoints")
        self.weight, self.bias, self.gamma, self.beta = (sd[k].to(device=device, dtype=bf16).contiguous()
                                                         for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias"))
        self.cross_dim, self.num_tokens = cross_dim, self.weight.shape[0] // cross_dim
        if self.weight.shape[0] != self.num_tokens * cross_dim or self.num_tokens > MAX_TOKENS:
            raise NotImplementedError(f"IP-Adapter image projection of {self.weight.shape[0]} outputs for cross_attention_dim "
                                      f"{cross_dim}: 1 .. {MAX_TOKENS} image tokens are supported")

    def __call__(self, embeds: torch.Tensor) -> torch.Tensor:
        if embeds.dim() != 3 or embeds.shape[2] != self.weight.shape[1]:
            raise ValueError(f"image_embeds must be [batch][num_images][{self.weight.shape[1]}], got {tuple(embeds.shape)}")
        B, n_img, _ = embeds.shape
        if n_img * self.num_tokens > MAX_TOKENS:
            raise NotImplementedError(f"{n_img} images x {self.num_tokens} tokens: more than {MAX_TOKENS} image tokens per adapter")
        x = embeds.to(device=self.weight.device, dtype=bf16).reshape(B * n_img, -1).contiguous()
        y = ops.linear_small_m(x, self.weight, self.bias)
        y = ops.layer_norm(y.view(B * n_img * self.num_tokens, self.cross_dim), self.gamma, self.beta, 1e-5)
        return y.view(B, n_img * self.num_tokens, self.cross_dim)


_RESAMPLER_TOP = ("latents", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias", "norm_out.weight", "norm_out.bias")
_RESAMPLER_LAYER = ("0.norm1.weight", "0.norm1.bias", "0.norm2.weight", "0.norm2.bias", "0.to_q.weight", "0.to_kv.weight",
                    "0.to_out.weight", "1.0.weight", "1.0.bias", "1.1.weight", "1.3.weight")
RESAMPLER_HEAD_DIM = 64     # every published Resampler; the head size of da_attention_resampler_bf16
RESAMPLER_MAX_LATENTS = 16  # one query tile of da_attention_resampler_bf16


def ip_adapter_plus_param_shapes(config, num_tokens: int = 16, image_embed_dim: int = 1280, dim: int = 768, depth: int = 4,
                                 ff_mult: int = 4) -> Dict[str, tuple]:
    """Shapes of a plus (Resampler) IP-Adapter checkpoint for a U-Net config in the original key layout: ``image_proj.layers.i.0`` is
    the perceiver attention (``norm1`` the image side, ``norm2`` the latents, ``to_kv`` the K rows, then the V rows),
    ``image_proj.layers.i.1`` the feed-forward (``.0`` LayerNorm, ``.1`` up, ``.3`` down).  ``heads = dim / 64``."""
    cross = config["cross_attention_dim"]
    shapes = {"image_proj.latents": (1, num_tokens, dim), "image_proj.proj_in.weight": (dim, image_embed_dim),
              "image_proj.proj_in.bias": (dim,), "image_proj.proj_out.weight": (cross, dim), "image_proj.proj_out.bias": (cross,),
              "image_proj.norm_out.weight": (cross,), "image_proj.norm_out.bias": (cross,)}
    for i in range(depth):
        pre = f"image_proj.layers.{i}."
        for n in ("0.norm1", "0.norm2", "1.0"):
            shapes[pre + n + ".weight"] = shapes[pre + n + ".bias"] = (dim,)
        shapes[pre + "0.to_q.weight"] = shapes[pre + "0.to_out.weight"] = (dim, dim)
        shapes[pre + "0.to_kv.weight"] = (2 * dim, dim)
        shapes[pre + "1.1.weight"], shapes[pre + "1.3.weight"] = (ff_mult * dim, dim), (dim, ff_mult * dim)
    for i, width in enumerate(cross_attention_widths(config)):
        shapes[f"ip_adapter.{2 * i + 1}.to_k_ip.weight"] = shapes[f"ip_adapter.{2 * i + 1}.to_v_ip.weight"] = (width, cross)
    return shapes


def is_resampler(sd: Dict[str, torch.Tensor]) -> bool:
    """An ``image_proj`` dict that is not a plain ImageProjection: a plus Resampler, complete or not, or one of the FaceID kinds."""
    return any(k in sd for k in _RESAMPLER_KEYS) or "proj.0.weight" in sd


class Resampler:
    """models/embeddings.py IPAdapterPlusImageProjection, the projection of the plus checkpoints: ``depth`` perceiver layers in which
    ``num_tokens`` learned latents attend to the vision encoder's penultimate hidden states and to themselves, then a feed-forward.
    ``[B][n_img][S0][embed]`` -> ``[B][n_img * num_tokens][cross_dim]``, the call contract of :class:`ImageProjection` (the images of a
    sample are folded into the batch and back; their tokens end up adjacent).

    Per layer: two LayerNorm launches, the stacked ``to_k | to_v`` projection of the image rows, ONE stacked ``to_q | to_k | to_v``
    projection of the latent rows, ``ops.resampler_attention`` on the column blocks of those two outputs (no cat, no transpose),
    ``to_out`` with the residual epilogue, LayerNorm, FF up with the exact-GELU epilogue, FF down with the residual epilogue."""

    def __init__(self, sd: Dict[str, torch.Tensor], cross_dim: int, device):
        faceid = [k for k in sd if k in _RESAMPLER_KEYS[2:] or k == "proj.0.weight"]
        if faceid:
            raise NotImplementedError(f"IP-Adapter Resampler / FaceID projections with the key {faceid[0]!r} (FaceID, FaceID-plus, "
                                      "full-face) are not built: only the plus Resampler and the base ImageProjection")
        depth = 1 + max([int(k.split(".")[1]) for k in sd if k.startswith("layers.") and k.split(".")[1].isdigit()], default=-1)
        want = set(_RESAMPLER_TOP) | {f"layers.{i}.{n}" for i in range(depth) for n in _RESAMPLER_LAYER}
        if depth == 0 or set(sd) != want:
            odd = sorted(want - set(sd)) or sorted(set(sd) - want) or ["layers.0.0.to_q.weight"]
            raise NotImplementedError(f"IP-Adapter Resampler projection: the checkpoint is not a complete plus Resampler, key "
                                      f"{odd[0]!r} is {'missing' if odd[0] in want else 'unexpected'}")
        w = {k: v.to(device=device, dtype=bf16).contiguous() for k, v in sd.items()}
        self.latents = w["latents"][0].contiguous()                       # [Nq][dim]
        self.num_tokens, self.dim = self.latents.shape
        self.embed_dim, self.cross_dim, self.depth = w["proj_in.weight"].shape[1], cross_dim, depth
        inner = w["layers.0.0.to_q.weight"].shape[0]
        self.heads, self.inner = inner // RESAMPLER_HEAD_DIM, inner
        if inner % RESAMPLER_HEAD_DIM or not 1 <= self.num_tokens <= RESAMPLER_MAX_LATENTS:
            raise NotImplementedError(f"IP-Adapter Resampler with {self.num_tokens} latents and an attention width of {inner}: heads of "
                                      f"{RESAMPLER_HEAD_DIM} channels and 1 .. {RESAMPLER_MAX_LATENTS} latents are supported")
        if w["proj_out.weight"].shape[0] != cross_dim:
            raise ValueError(f"IP-Adapter Resampler projects to {w['proj_out.weight'].shape[0]} channels, the U-Net's "
                             f"cross_attention_dim is {cross_dim}")
        self.proj_in, self.proj_out = (w["proj_in.weight"], w["proj_in.bias"]), (w["proj_out.weight"], w["proj_out.bias"])
        self.norm_out = (w["norm_out.weight"], w["norm_out.bias"])
        self.layers = []
        for i in range(depth):
            g = lambda n: w[f"layers.{i}.{n}"]  # noqa: E731
            self.layers.append(dict(ln0=(g("0.norm1.weight"), g("0.norm1.bias")), ln1=(g("0.norm2.weight"), g("0.norm2.bias")),
                                    kv=g("0.to_kv.weight"), qkv=torch.cat([g("0.to_q.weight"), g("0.to_kv.weight")]).contiguous(),
                                    out=g("0.to_out.weight"), ff_ln=(g("1.0.weight"), g("1.0.bias")), up=g("1.1.weight"),
                                    down=g("1.3.weight")))

    def __call__(self, embeds: torch.Tensor) -> torch.Tensor:
        if embeds.dim() != 4 or embeds.shape[3] != self.embed_dim:
            raise ValueError(f"image_embeds of a plus (Resampler) adapter must be [batch][num_images][tokens][{self.embed_dim}] (the "
                             f"vision encoder's hidden_states[-2]), got {tuple(embeds.shape)}")
        B, n_img, S0, _ = embeds.shape
        Nq, inner = self.num_tokens, self.inner
        if n_img * Nq > MAX_TOKENS:
            raise NotImplementedError(f"{n_img} images x {Nq} tokens: more than {MAX_TOKENS} image tokens per adapter")
        Bf = B * n_img
        x = embeds.to(device=self.latents.device, dtype=bf16).reshape(Bf * S0, self.embed_dim).contiguous()
        x = ops.linear(x, *self.proj_in)
        lat = self.latents.repeat(Bf, 1)
        for ly in self.layers:
            e, l = ops.layer_norm(x, *ly["ln0"], 1e-5), ops.layer_norm(lat, *ly["ln1"], 1e-5)
            kv0, qkv1 = ops.linear(e, ly["kv"]), ops.linear(l, ly["qkv"])
            a = ops.resampler_attention(qkv1[:, :inner], kv0[:, :inner], kv0[:, inner:], qkv1[:, inner:2 * inner], qkv1[:, 2 * inner:],
                                        B=Bf, H=self.heads, Nq=Nq, S0=S0, S0_alloc=S0, S1=Nq, S1_alloc=Nq,
                                        scale=RESAMPLER_HEAD_DIM ** -0.5)
            lat = ops.linear(a, ly["out"], residual=lat)
            h = ops.linear(ops.layer_norm(lat, *ly["ff_ln"], 1e-5), ly["up"], act=L.ACT_GELU_ERF)
            lat = ops.linear(h, ly["down"], residual=lat)
        y = ops.layer_norm(ops.linear(lat, *self.proj_out), *self.norm_out, 1e-5)
        return y.view(B, n_img * Nq, self.cross_dim)


def cross_attention_layers(unet) -> list:
    """The cross-attention ``layers.Attention`` objects of a loaded U-Net in checkpoint order: down, up, mid."""
    trs = [t for st in unet.down for t in st["attns"]] + [t for st in unet.up for t in st["attns"]] + list(unet.mid["attns"])
    return [blk.attn2 for t in trs for blk in t.blocks]


def load_into_unet(unet, state_dicts) -> None:
    """``UNet2DConditionModel._load_ip_adapter_weights``: one image projection (a :class:`Resampler` for a plus checkpoint, an
    :class:`ImageProjection` otherwise; the two kinds mix freely) and one ``to_k_ip | to_v_ip`` pair per layer for each checkpoint; the
    scales start at 1.0."""
    if isinstance(state_dicts, dict):
        state_dicts = [state_dicts]
    sds = [nest(sd) for sd in state_dicts]
    if not 1 <= len(sds) <= L.IP_MAX_ADAPTERS:
        raise NotImplementedError(f"{len(sds)} IP-Adapters: 1 .. {L.IP_MAX_ADAPTERS} at once are supported")
    layers = cross_attention_layers(unet)
    proj = [(Resampler if is_resampler(sd["image_proj"]) else ImageProjection)(sd["image_proj"], unet.config.cross_attention_dim, unet.device)
            for sd in sds]
    for sd in sds:
        want = {f"{2 * i + 1}.to_{c}_ip.weight" for i in range(len(layers)) for c in "kv"}
        if set(sd["ip_adapter"]) != want:
            odd = sorted(set(sd["ip_adapter"]) ^ want)
            raise ValueError(f"IP-Adapter checkpoint does not match this U-Net's {len(layers)} cross-attention layers: {odd[:6]} ...")
    for i, layer in enumerate(layers):
        layer.attach_ip([(sd["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"], sd["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"]) for sd in sds])
    unet._ip, unet._ip_scales = proj, (1.0,) * len(sds)
    unet._ip_generation = next(_GENERATION)    # a captured step must not outlive the adapter weights it points into
    unet._cond_cache = None


def unload_from_unet(unet) -> None:
    for layer in cross_attention_layers(unet):
        layer.attach_ip(None)
    unet._ip, unet._ip_scales, unet._cond_cache = None, (), None


def set_scales(unet, scale) -> None:
    if unet._ip is None:
        raise ValueError("set_ip_adapter_scale: no IP-Adapter is loaded")
    scales = list(scale) if isinstance(scale, (list, tuple)) else [scale] * len(unet._ip)
    if any(isinstance(s, dict) for s in scales):
        raise NotImplementedError("per-block IP-Adapter scale dicts are not built: one float per adapter")
    if len(scales) != len(unet._ip):
        raise ValueError(f"set_ip_adapter_scale: {len(scales)} scales for {len(unet._ip)} adapters")
    unet._ip_scales = tuple(float(s) for s in scales)
    for layer in cross_attention_layers(unet):
        layer.ip_scales = unet._ip_scales


def image_kv(unet, added_cond_kwargs, batch: int, kvs) -> None:
    """The image half of ``precompute_conditioning``: project ``added_cond_kwargs["image_embeds"]`` (one tensor per adapter) once and
    give every cross-attention's ``CrossKV`` its image keys / values."""
    embeds = (added_cond_kwargs or {}).get("image_embeds")
    if embeds is None:
        raise ValueError("an IP-Adapter is loaded: `added_cond_kwargs['image_embeds']` (a list, one [batch][num_images][emb] tensor per "
                         "adapter, [batch][num_images][tokens][emb] for a plus adapter) is required")
    embeds = [embeds] if torch.is_tensor(embeds) else list(embeds)
    if len(embeds) != len(unet._ip) or any(e.shape[0] != batch for e in embeds):
        raise ValueError(f"image_embeds: expected {len(unet._ip)} tensors of batch {batch}, got {[tuple(e.shape) for e in embeds]}")
    tokens = [pad_encoder_states(p(e).contiguous()) for p, e in zip(unet._ip, embeds)]
    flat = [kv for per_transformer in kvs for kv in per_transformer]
    for layer, kv in zip(cross_attention_layers_in_walk_order(unet), flat):
        kv.ip = layer.precompute_ip_kv(tokens, batch)


def cross_attention_layers_in_walk_order(unet) -> list:
    """(the forward's order -- down, mid, up -- in which ``precompute_conditioning`` lists the CrossKVs)"""
    return [blk.attn2 for t in unet._transformers() for blk in t.blocks]
