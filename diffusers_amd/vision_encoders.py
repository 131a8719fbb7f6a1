"""The CLIP vision encoder on the engine's kernels: a drop-in for ``transformers.CLIPVisionModelWithProjection`` in the pipelines'
``image_encoder`` slot (IP-Adapter: pipelines/stable_diffusion/pipeline_stable_diffusion.py encode_image reads ``.image_embeds``).

Same config, ``state_dict`` keys and call signature as ``transformers`` (modeling_clip.py CLIPVisionTransformer.forward, version 5.x as
installed).  The front of the model -- centre crop, rescale, normalise, patch convolution, class token, position embedding,
``pre_layrnorm`` -- is ONE launch of csrc/clip_patch_embed.hip (``ops.clip_patch_embed``); the layers run as in
``text_encoders.CLIPTextModel``: LayerNorm, the Q|K + swapped V^T pair launch, unmasked flash attention over ``Skv = 1 + G G`` keys of
``S_alloc`` rows, fc1 with the activation in its epilogue, bias + residual in the GEMM epilogue; ``visual_projection`` is the skinny linear.
Head sizes that are no kernel size (ViT-H: 80 -> 96, bigG: 104 -> 128) are zero-padded once in the packed weights; the attention scale
stays that of the true head size.

``hidden_states`` follows the reference: entry 0 is the first layer's INPUT, i.e. the rows after ``pre_layrnorm`` (the kernel's
``x_out``), entry i the output of layer i; ``last_hidden_state`` is the last layer's output, ``image_embeds`` =
visual_projection(post_layernorm(its class row)).
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Optional

import torch

from . import ops
from .config_utils import check_to
from .layers import Weights, kernel_head_dim, pad_head_cols, pad_head_rows
from .text_encoders import _CLIP_ACT, ModelOutput, _SelfAttention, _cfg, _pad_rows

bf16 = torch.bfloat16

_VISION_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, projection_dim=512, num_hidden_layers=12, num_attention_heads=12,
                        num_channels=3, image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5)
CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)     # OPENAI_CLIP_MEAN / OPENAI_CLIP_STD, CLIPImageProcessor's defaults
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)


def resize_crop_geometry(height: int, width: int, size: int):
    """CLIPImageProcessor's geometry: the shortest side goes to ``size`` and the long one to ``int(size * long / short)``
    (image_transforms.get_resize_output_image_size, default_to_square=False), then the centre crop's origin (center_crop).
    Returns ``((new_h, new_w), (top, left))``."""
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = size, int(size * long / short)
    nh, nw = (new_long, new_short) if width <= height else (new_short, new_long)
    return (nh, nw), ((nh - size) // 2, (nw - size) // 2)


def clip_vision_param_shapes(config) -> dict:
    """``transformers.CLIPVisionModelWithProjection.state_dict()`` names -> shapes."""
    c = _cfg(config, _VISION_DEFAULTS)
    h, m, v = c.hidden_size, c.intermediate_size, "vision_model."
    sh = {v + "embeddings.class_embedding": (h,), v + "embeddings.patch_embedding.weight": (h, 3, c.patch_size, c.patch_size),
          v + "embeddings.position_embedding.weight": (1 + (c.image_size // c.patch_size) ** 2, h)}
    for n in ("pre_layrnorm", "post_layernorm"):
        sh[f"{v}{n}.weight"], sh[f"{v}{n}.bias"] = (h,), (h,)
    for i in range(c.num_hidden_layers):
        q = f"{v}encoder.layers.{i}."
        for n in ("q", "k", "v", "out"):
            sh[q + f"self_attn.{n}_proj.weight"], sh[q + f"self_attn.{n}_proj.bias"] = (h, h), (h,)
        for n in ("layer_norm1", "layer_norm2"):
            sh[q + n + ".weight"], sh[q + n + ".bias"] = (h,), (h,)
        sh[q + "mlp.fc1.weight"], sh[q + "mlp.fc1.bias"] = (m, h), (m,)
        sh[q + "mlp.fc2.weight"], sh[q + "mlp.fc2.bias"] = (h, m), (h,)
    sh["visual_projection.weight"] = (c.projection_dim, h)
    return sh


class _PaddedSelfAttention(_SelfAttention):
    """``_SelfAttention`` at head sizes 64 / 96 / 128: q / k / v rows and out_proj columns zero-padded per head to the kernel's size."""

    def __init__(self, wq, wk, wv, wo, bq, bk, bv, bo, heads: int):
        d = wq.shape[0] // heads
        dp = kernel_head_dim(d)
        if dp > 128:
            raise ValueError(f"CLIP vision attention: head size {d} exceeds 128")
        rows = lambda t: pad_head_rows(t, heads, d, dp)
        self.heads, self.inner, self.head = heads, heads * dp, dp
        self.wqk = torch.cat([rows(wq), rows(wk)], 0).contiguous()
        self.bqk = torch.cat([rows(bq), rows(bk)], 0).contiguous()
        self.wv, self.bv, self.wo, self.bo = rows(wv), rows(bv), pad_head_cols(wo, heads, d, dp), bo
        self.scale = d ** -0.5


class CLIPVisionModelWithProjection:
    """``transformers.CLIPVisionModelWithProjection``: ``forward(pixel_values)`` takes normalised float32 / bf16 [B][3][S][S] images;
    :meth:`encode_image` takes the images themselves (CLIPImageProcessor's route)."""

    def __init__(self, config):
        self.config = _cfg(config, _VISION_DEFAULTS)
        c = self.config
        if c.hidden_act not in _CLIP_ACT:
            raise ValueError(f"CLIP hidden_act {c.hidden_act!r} is not supported")
        if c.num_channels != 3 or c.image_size % c.patch_size or c.hidden_size % 128 or c.hidden_size > 1664 or \
                c.hidden_size % c.num_attention_heads or 3 * c.patch_size ** 2 > 3072:
            raise ValueError("diffusers_amd CLIP vision encoder: 3 channels, image_size a multiple of patch_size <= 32, hidden_size a "
                             "multiple of 128 and of the head count, at most 1664")
        self.image_mean, self.image_std = CLIP_IMAGE_MEAN, CLIP_IMAGE_STD
        self.dtype, self.device, self._built = bf16, None, False

    @classmethod
    def from_pretrained(cls, path, subfolder: Optional[str] = None, variant: Optional[str] = None, device="cuda"):
        """A local ``transformers`` directory: config.json, model.safetensors (or its shards) and, where present,
        preprocessor_config.json for ``image_mean`` / ``image_std``."""
        from .loading import LazyCheckpoint, _weight_files
        d = Path(path) / subfolder if subfolder else Path(path)
        model = cls(json.loads((d / "config.json").read_text()))
        model.load_state_dict(LazyCheckpoint(_weight_files(d, variant, stem="model")), device=device)
        pre = d / "preprocessor_config.json"
        if pre.is_file():
            pc = json.loads(pre.read_text())
            model.image_mean = tuple(pc.get("image_mean", CLIP_IMAGE_MEAN))
            model.image_std = tuple(pc.get("image_std", CLIP_IMAGE_STD))
        return model

    def load_state_dict(self, state_dict, device="cuda", strict: bool = True):
        c = self.config
        w = Weights(state_dict, device)
        self.device = torch.device(device)
        p = "vision_model." if w.has("vision_model.embeddings.class_embedding") else ""
        self.patch_w = ops.pack_clip_patch_weight(w.get(p + "embeddings.patch_embedding.weight"))
        self.cls = w.get(p + "embeddings.class_embedding")
        self.pos = w.get(p + "embeddings.position_embedding.weight")
        self.pre_ln = (w.get(p + "pre_layrnorm.weight"), w.get(p + "pre_layrnorm.bias"))
        self.layers = []
        for i in range(c.num_hidden_layers):
            q = f"{p}encoder.layers.{i}."
            a = _PaddedSelfAttention(*(w.get(q + f"self_attn.{n}_proj.weight") for n in ("q", "k", "v", "out")),
                                     *(w.get(q + f"self_attn.{n}_proj.bias") for n in ("q", "k", "v", "out")),
                                     heads=c.num_attention_heads)
            self.layers.append({"ln1": (w.get(q + "layer_norm1.weight"), w.get(q + "layer_norm1.bias")), "attn": a,
                                "ln2": (w.get(q + "layer_norm2.weight"), w.get(q + "layer_norm2.bias")),
                                "fc1": (w.get(q + "mlp.fc1.weight"), w.get(q + "mlp.fc1.bias")),
                                "fc2": (w.get(q + "mlp.fc2.weight"), w.get(q + "mlp.fc2.bias"))})
        self.post_ln = (w.get(p + "post_layernorm.weight"), w.get(p + "post_layernorm.bias"))
        self.visual_projection = w.get("visual_projection.weight")
        if strict and [k for k in w.unused() if not k.endswith("position_ids")]:
            raise RuntimeError(f"unexpected keys in state_dict: {w.unused()[:8]} ...")
        self._built = True
        return self

    def to(self, *args, **kwargs):
        return check_to(self, args, kwargs)

    def eval(self):
        return self

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    def _tokens(self) -> int:
        return 1 + (self.config.image_size // self.config.patch_size) ** 2

    def _front(self, image: torch.Tensor, out=None, **kw):
        c = self.config
        return ops.clip_patch_embed(image, self.patch_w, self.cls, self.pos, *self.pre_ln, c.layer_norm_eps, patch=c.patch_size,
                                    out=out, **kw)[0]

    def _encode(self, x: torch.Tensor, B: int, output_hidden_states, return_dict: bool):
        """x: [B * S_alloc][hidden], the first layer's input."""
        c = self.config
        S = self._tokens()
        S_alloc = _pad_rows(S)
        unpad = lambda h: h.view(B, S_alloc, -1)[:, :S]
        act = _CLIP_ACT[c.hidden_act]
        hidden = [unpad(x)] if output_hidden_states else None
        for ly in self.layers:
            h = ops.layer_norm(x, *ly["ln1"], c.layer_norm_eps)
            x = ly["attn"](h, B, S, S_alloc, residual=x)
            h = ops.layer_norm(x, *ly["ln2"], c.layer_norm_eps)
            h = ops.linear(h, *ly["fc1"], act=act)
            x = ops.linear(h, *ly["fc2"], residual=x)
            if output_hidden_states:
                hidden.append(unpad(x))
        last = unpad(x)
        pooled = ops.layer_norm(last[:, 0].contiguous(), *self.post_ln, c.layer_norm_eps)
        embeds = ops.linear_small_m(pooled, self.visual_projection) if B <= 8 else ops.linear(pooled, self.visual_projection)
        out = ModelOutput(image_embeds=embeds, last_hidden_state=last, hidden_states=tuple(hidden) if output_hidden_states else None)
        return out if return_dict else out.to_tuple()

    @torch.no_grad()
    def forward(self, pixel_values: Optional[torch.Tensor] = None, output_hidden_states: Optional[bool] = None,
                return_dict: bool = True, **kwargs):
        if not self._built:
            raise RuntimeError(f"{type(self).__name__}: call load_state_dict() first")
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        S = self.config.image_size
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S):
            raise ValueError(f"pixel_values must be [B][3][{S}][{S}], got {tuple(pixel_values.shape)}")
        pv = pixel_values.to(device=self.device, dtype=torch.float32).contiguous()
        return self._encode(self._front(pv), pv.shape[0], output_hidden_states, return_dict)

    @torch.no_grad()
    def encode_image(self, images, output_hidden_states: Optional[bool] = None, return_embeds: bool = True):
        """CLIPImageProcessor + forward for PIL images, uint8 HWC arrays / tensors or a list of them: each is uploaded as it is, its
        shortest side resized to ``image_size`` (bicubic, Pillow's to the bit: ops.resample_u8) and the centre crop, rescale and
        normalise happen inside the patch kernel -- no cropped copy, no float image.  Returns ``image_embeds`` [B][projection_dim], or
        the whole output with ``return_embeds=False``."""
        import numpy as np
        if not self._built:
            raise RuntimeError(f"{type(self).__name__}: call load_state_dict() first")
        images = list(images) if isinstance(images, (list, tuple)) else [images]
        S, S_alloc = self.config.image_size, _pad_rows(self._tokens())
        x = torch.empty((len(images) * S_alloc, self.config.hidden_size), device=self.device, dtype=bf16)
        for b, img in enumerate(images):
            if hasattr(img, "convert"):
                img = np.array(img.convert("RGB"))
            t = torch.as_tensor(np.ascontiguousarray(img) if isinstance(img, np.ndarray) else img)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError(f"encode_image: PIL images or uint8 [H][W][3] arrays / tensors are required, got {t.dtype} "
                                 f"{tuple(t.shape)}")
            size, crop = resize_crop_geometry(t.shape[0], t.shape[1], S)
            small = ops.resample_u8(t.to(self.device).contiguous()[None], size, "bicubic")
            self._front(small, out=x[b * S_alloc:(b + 1) * S_alloc], size=S, crop=crop, mean=self.image_mean, std=self.image_std)
        out = self._encode(x, len(images), output_hidden_states, True)
        return out.image_embeds if return_embeds else out
