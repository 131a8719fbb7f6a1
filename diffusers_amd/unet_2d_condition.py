"""UNet2DConditionModel on the gfx950 kernels.

Mirrors the reference class (models/unets/unet_2d_condition.py:979-1235) for the configurations the BASELINE names
(SD1.5 and SDXL): same constructor kwargs, same ``state_dict`` key names / shapes, same ``forward`` arguments and
NCHW in/out tensors, same ``ValueError``s for unsupported arguments.  Inside, activations are channels-last bf16 and every op is
a hand-written HIP kernel (see layers.py / csrc/).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import torch

from . import ops
from .config_utils import check_to
from .loading import PretrainedMixin
from .layers import (GroupNorm, ResnetBlock2D, TimeProjections, TimestepEmbedding, Transformer2DModel, Upsample2D, Weights,
                     encoder_mask_bias, pad_encoder_states)
from .unet_blocks import build_down_blocks, build_mid_block, walk_down, walk_mid

bf16 = torch.bfloat16


@dataclass
class UNet2DConditionOutput:
    sample: torch.Tensor


class FrozenConfig(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


_DEFAULTS = dict(
    sample_size=None, in_channels=4, out_channels=4, center_input_sample=False, flip_sin_to_cos=True, freq_shift=0,
    down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
    mid_block_type="UNetMidBlock2DCrossAttn",
    up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
    only_cross_attention=False, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, downsample_padding=1,
    mid_block_scale_factor=1, dropout=0.0, act_fn="silu", norm_num_groups=32, norm_eps=1e-5,
    cross_attention_dim=1280, transformer_layers_per_block=1, reverse_transformer_layers_per_block=None,
    encoder_hid_dim=None, encoder_hid_dim_type=None, attention_head_dim=8, num_attention_heads=None,
    dual_cross_attention=False, use_linear_projection=False, class_embed_type=None, addition_embed_type=None,
    addition_time_embed_dim=None, num_class_embeds=None, upcast_attention=False, resnet_time_scale_shift="default",
    resnet_skip_time_act=False, resnet_out_scale_factor=1.0, time_embedding_type="positional",
    time_embedding_dim=None, time_embedding_act_fn=None, timestep_post_act=None, time_cond_proj_dim=None,
    conv_in_kernel=3, conv_out_kernel=3, projection_class_embeddings_input_dim=None, attention_type="default",
    class_embeddings_concat=False, mid_block_only_cross_attention=None, cross_attention_norm=None,
    addition_embed_type_num_heads=64,
)


def _tup(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


class UNet2DConditionModel(PretrainedMixin):
    """Drop-in for the reference ``UNet2DConditionModel`` (inference, bf16, HIP device only)."""

    def __init__(self, **kwargs):
        unknown = set(kwargs) - set(_DEFAULTS)
        if unknown:
            raise TypeError(f"UNet2DConditionModel: unexpected config keys {sorted(unknown)}")
        cfg = dict(_DEFAULTS)
        cfg.update(kwargs)
        self.config = FrozenConfig(cfg)
        c = self.config
        # -- what the engine implements; everything else is refused loudly rather than silently approximated --
        if c.act_fn != "silu" or c.resnet_time_scale_shift != "default" or c.time_embedding_type != "positional":
            raise ValueError("diffusers_amd UNet2DConditionModel supports act_fn='silu', default time scale shift")
        if c.class_embed_type is not None or c.num_class_embeds is not None or c.encoder_hid_dim_type is not None:
            raise ValueError("class / encoder_hid embeddings are not on the BASELINE hot path")
        if c.addition_embed_type not in (None, "text_time"):
            raise ValueError(f"addition_embed_type={c.addition_embed_type!r} is not supported")
        if c.dual_cross_attention or c.only_cross_attention or c.attention_type != "default" or c.upcast_attention:
            raise ValueError("unsupported attention variant")
        if c.conv_in_kernel != 3 or c.conv_out_kernel != 3:
            raise ValueError("unsupported conv_in/out kernel")
        tcd = c.time_cond_proj_dim
        if tcd is not None and (isinstance(tcd, bool) or not isinstance(tcd, int) or tcd <= 0 or tcd % 8):
            # (the skinny linear reads its K in 16-byte chunks; the distilled LCM checkpoints use 256)
            raise ValueError(f"time_cond_proj_dim={tcd!r}: None or a positive multiple of 8")
        # options the engine has no code for must sit at their reference defaults: a non-default value would change the
        # reference's arithmetic, so it is refused rather than ignored
        for k in ("center_input_sample", "dropout", "resnet_skip_time_act", "resnet_out_scale_factor",
                  "time_embedding_dim", "time_embedding_act_fn", "timestep_post_act", "encoder_hid_dim",
                  "class_embeddings_concat", "mid_block_only_cross_attention", "cross_attention_norm",
                  "projection_class_embeddings_input_dim" if c.addition_embed_type is None else "dropout"):
            if c[k] != _DEFAULTS[k]:
                raise ValueError(f"diffusers_amd UNet2DConditionModel: config option {k}={c[k]!r} is not implemented on "
                                 f"the HIP path (only the default {_DEFAULTS[k]!r})")
        if len(c.down_block_types) != len(c.up_block_types) or len(c.block_out_channels) != len(c.down_block_types):
            raise ValueError("Must provide the same number of `down_block_types`, `up_block_types`, `block_out_channels`.")
        for t in c.down_block_types:
            if t not in ("CrossAttnDownBlock2D", "DownBlock2D"):
                raise ValueError(f"{t} does not exist.")
        for t in c.up_block_types:
            if t not in ("CrossAttnUpBlock2D", "UpBlock2D"):
                raise ValueError(f"{t} does not exist.")
        if c.mid_block_type != "UNetMidBlock2DCrossAttn":
            raise ValueError(f"unknown mid_block_type : {c.mid_block_type}")
        self.dtype = bf16
        self.device = None
        self._built = False

    # ------------------------------------------------------------------------------------------------------------
    # weights
    # ------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], device="cuda", strict: bool = True):
        """Pack a reference-format state_dict (keys as ``reference_unet.state_dict()``) onto ``device``."""
        c = self.config
        w = Weights(state_dict, device)
        self.device = torch.device(device)
        self._new_weights_generation()
        self._cond_cache = None   # hoisted K / V^T of the previous weights must not outlive them
        n = len(c.block_out_channels)
        boc = tuple(c.block_out_channels)
        groups, eps = c.norm_num_groups, c.norm_eps
        heads = _tup(c.num_attention_heads or c.attention_head_dim, n)
        lpb = _tup(c.layers_per_block, n)
        tlpb = _tup(c.transformer_layers_per_block, n)
        temb_dim = boc[0] * 4

        # conv_in stays in torch layout [Cout][Cin][3][3] -> [Cout][9*Cin] for the thin-input kernel
        self.conv_in_w = ops.pack_conv_weight(w.get("conv_in.weight"))
        self.conv_in_b = w.get("conv_in.bias")
        self.time_embedding = TimestepEmbedding(w, "time_embedding")
        # TimestepEmbedding.cond_proj (models/embeddings.py:1276-1279, bias-free): the guidance-scale embedding of the distilled LCM
        # checkpoints, projected onto the sinusoidal timestep embedding in front of linear_1
        self.time_cond_proj = None
        if c.time_cond_proj_dim is not None:
            self.time_cond_proj = w.get("time_embedding.cond_proj.weight")
            if tuple(self.time_cond_proj.shape) != (boc[0], c.time_cond_proj_dim):
                raise ValueError(f"time_embedding.cond_proj.weight has shape {tuple(self.time_cond_proj.shape)}, the config asks for "
                                 f"{(boc[0], c.time_cond_proj_dim)}")
        self.add_embedding = TimestepEmbedding(w, "add_embedding") if c.addition_embed_type == "text_time" else None

        self.down = build_down_blocks(w, c)
        self.mid = build_mid_block(w, c)

        rheads = tuple(reversed(heads))
        rlpb = tuple(reversed(lpb))
        rtlpb = tuple(reversed(tlpb)) if c.reverse_transformer_layers_per_block is None \
            else _tup(c.reverse_transformer_layers_per_block, n)
        self.up = []
        for i, btype in enumerate(c.up_block_types):
            pre = f"up_blocks.{i}"
            stage = {"resnets": [], "attns": [], "up": None}
            for j in range(rlpb[i] + 1):
                stage["resnets"].append(ResnetBlock2D(w, f"{pre}.resnets.{j}", groups, eps))
                if btype == "CrossAttnUpBlock2D":
                    stage["attns"].append(Transformer2DModel(w, f"{pre}.attentions.{j}", rheads[i], rtlpb[i], groups))
            if i != n - 1:
                stage["up"] = Upsample2D(w, f"{pre}.upsamplers.0")
            self.up.append(stage)
        # every block's time_emb_proj in one launch per forward (layers.TimeProjections), blocks in forward order
        self.time_proj = TimeProjections([r for st in self.down for r in st["resnets"]] + self.mid["resnets"] +
                                         [r for st in self.up for r in st["resnets"]])

        self.conv_norm_out = GroupNorm(w, "conv_norm_out", groups, eps)
        self.conv_out_w = ops.pack_conv_weight(w.get("conv_out.weight"))
        self.conv_out_b = w.get("conv_out.bias")
        if strict and w.unused():
            raise RuntimeError(f"unexpected keys in state_dict: {w.unused()[:8]} ...")
        self._temb_dim = temb_dim
        self._built = True
        return self

    def to(self, *args, **kwargs):
        return check_to(self, args, kwargs)

    def eval(self):
        return self

    # ------------------------------------------------------------------------------------------------------------
    # step-invariant work (hoisted): cross-attention K / V^T of every transformer block, SDXL text_time embedding
    # ------------------------------------------------------------------------------------------------------------
    def _transformers(self) -> List[Transformer2DModel]:
        out = []
        for st in self.down:
            out += st["attns"]
        out += self.mid["attns"]
        for st in self.up:
            out += st["attns"]
        return out

    def precompute_conditioning(self, encoder_hidden_states: torch.Tensor,
                                added_cond_kwargs: Optional[Dict[str, torch.Tensor]] = None,
                                encoder_attention_mask: Optional[torch.Tensor] = None,
                                timestep_cond: Optional[torch.Tensor] = None) -> Dict[str, Any]:
        """Everything in forward() that does not depend on the timestep or the latents.  ``timestep_cond`` (a U-Net with
        ``time_cond_proj_dim``): kept as a static bf16 buffer the step reads by address."""
        ops.require_hip(encoder_hidden_states, "encoder_hidden_states")
        B = encoder_hidden_states.shape[0]
        tc = self._check_timestep_cond(timestep_cond, B)
        ehs_pad, skv, skv_alloc = pad_encoder_states(encoder_hidden_states.contiguous())
        bias = None
        if encoder_attention_mask is not None:
            bias = encoder_mask_bias(encoder_attention_mask.to(encoder_hidden_states.device), B, skv)
        kvs = [tr.precompute_kv(ehs_pad, B, skv, skv_alloc, bias) for tr in self._transformers()]
        aug = None
        if self.config.addition_embed_type == "text_time":
            aug = self._text_time_embedding(added_cond_kwargs, B)
        cond = {"kvs": kvs, "aug_emb": aug, "batch": B, "ehs_ptr": encoder_hidden_states.data_ptr()}
        if tc is not None:
            cond["timestep_cond"] = tc
        return cond

    def _check_timestep_cond(self, timestep_cond, B: int):
        """``timestep_cond`` as the step reads it: None for a U-Net without ``time_cond_proj_dim`` (which refuses the argument),
        else a fresh contiguous bf16 [B][time_cond_proj_dim] tensor on the device."""
        dim = self.config.time_cond_proj_dim
        if dim is None:
            if timestep_cond is not None:
                raise ValueError("diffusers_amd UNet2DConditionModel.forward: `timestep_cond` is not supported on the HIP path "
                                 "(this U-Net's config has no `time_cond_proj_dim`)")
            return None
        if timestep_cond is None:
            raise ValueError(f"this U-Net has time_cond_proj_dim={dim}: `timestep_cond` [batch][{dim}] is required")
        if not torch.is_tensor(timestep_cond) or timestep_cond.dim() != 2 or tuple(timestep_cond.shape) != (B, dim):
            got = tuple(timestep_cond.shape) if torch.is_tensor(timestep_cond) else type(timestep_cond).__name__
            raise ValueError(f"`timestep_cond` must be [{B}][{dim}] (batch, time_cond_proj_dim), got {got}")
        return timestep_cond.to(device=self.device, dtype=bf16).contiguous().clone()

    def _cached_conditioning(self, encoder_hidden_states, added_cond_kwargs, encoder_attention_mask=None, timestep_cond=None):
        """The drop-in path: an unchanged reference pipeline calls forward(sample, t, encoder_hidden_states=prompt_embeds,
        added_cond_kwargs=...) with the SAME tensors on every step (pipeline_stable_diffusion_xl.py:1208-1217), so the
        step-invariant work (140 K / V^T GEMMs + the text_time MLP for SDXL) is computed for the first call and reused
        while those tensors are the same objects with the same in-place version counters."""
        def ident(t):
            if t is None:
                return None
            if t.is_inference():
                # tensors made under torch.inference_mode() have no version counter (reading it raises): an in-place edit
                # could not be seen, so such a call is never served from the cache
                return False
            return (t.data_ptr(), t._version, tuple(t.shape), t.dtype)
        added = added_cond_kwargs or {}
        key = (ident(encoder_hidden_states), ident(added.get("text_embeds")), ident(added.get("time_ids")),
               ident(encoder_attention_mask), ident(timestep_cond))
        cacheable = not any(k is False for k in key)
        hit = getattr(self, "_cond_cache", None)
        if cacheable and hit is not None and hit[0] == key:
            return hit[1]
        ehs = encoder_hidden_states
        if ehs is not None and (ehs.dtype != bf16 or not ehs.is_cuda):
            ehs = ehs.to(device=self.device, dtype=bf16)
        cond = self.precompute_conditioning(ehs, added_cond_kwargs, encoder_attention_mask, timestep_cond)
        if not cacheable:
            self._cond_cache = None
            return cond
        # the cache holds references to the keyed tensors, so their storage (and data_ptr) cannot be recycled under it
        self._cond_cache = (key, cond, (encoder_hidden_states, added.get("text_embeds"), added.get("time_ids"),
                                        encoder_attention_mask, timestep_cond))
        return cond

    @staticmethod
    def _nhwc(r: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
        """A reference-layout (NCHW) residual as a channels-last bf16 tensor shaped like ``like``."""
        ops.require_hip(r, "additional residual", (bf16, torch.float16, torch.float32))
        if r.dim() != 4 or tuple(r.shape) != (like.shape[0], like.shape[3], like.shape[1], like.shape[2]):
            raise ValueError(f"additional residual of shape {tuple(r.shape)} does not match the activation "
                             f"{(like.shape[0], like.shape[3], like.shape[1], like.shape[2])} (NCHW)")
        return r.to(bf16).permute(0, 2, 3, 1).contiguous()

    def _text_time_embedding(self, added_cond_kwargs, B):
        # unet_2d_condition.py:906-922
        if added_cond_kwargs is None or "text_embeds" not in added_cond_kwargs:
            raise ValueError(f"{self.__class__} has the config param `addition_embed_type` set to 'text_time' which "
                             "requires the keyword argument `text_embeds` to be passed in `added_cond_kwargs`")
        if "time_ids" not in added_cond_kwargs:
            raise ValueError(f"{self.__class__} has the config param `addition_embed_type` set to 'text_time' which "
                             "requires the keyword argument `time_ids` to be passed in `added_cond_kwargs`")
        text_embeds = added_cond_kwargs["text_embeds"].to(device=self.device, dtype=bf16).contiguous()
        time_ids = added_cond_kwargs["time_ids"].to(device=self.device, dtype=torch.float32).contiguous()
        c = self.config
        n_ids = time_ids.shape[1]
        te = ops.timestep_embedding(time_ids.reshape(-1), c.addition_time_embed_dim, batch=B * n_ids,
                                    flip_sin_to_cos=c.flip_sin_to_cos, shift=float(c.freq_shift))
        te = te.view(B, n_ids * c.addition_time_embed_dim)
        add = torch.cat([text_embeds, te], dim=-1).contiguous()  # tiny host-side glue: (B, 2816)
        return self.add_embedding(add)

    # ------------------------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------------------------
    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    def forward(self, sample: torch.Tensor, timestep, encoder_hidden_states: torch.Tensor, class_labels=None,
                timestep_cond=None, attention_mask=None, cross_attention_kwargs=None, added_cond_kwargs=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None,
                down_intrablock_additional_residuals=None, encoder_attention_mask=None, return_dict: bool = True,
                conditioning: Optional[Dict[str, Any]] = None, sampler_table=None, step_idx=None, inpaint_cond=None,
                scale_model_input: bool = False, controlnet_handoff=None, image_cond=None):
        """Same signature as the reference forward (unet_2d_condition.py:979-994) plus engine extensions:
        ``conditioning`` (result of :meth:`precompute_conditioning`), ``sampler_table``/``step_idx`` (read the
        timestep from the device-resident sampler table so the call is HIP-graph replayable) and, for a 9-channel inpainting
        U-Net, ``inpaint_cond=(mask, masked_image_latents)``: ``sample`` is then the 4-channel, un-doubled latents, and conv_in reads
        its nine input channels from the three tensors (ops.conv_in_inpaint; the CFG halves are stored from one computation, their
        count taken from the conditioning batch).  ``scale_model_input`` (with ``inpaint_cond`` and ``sampler_table``) applies the
        Euler scheduler's ``scale_model_input`` to the latents inside that conv.  Without ``inpaint_cond`` a 9-channel ``sample``
        goes through the ordinary conv_in.  ``image_cond=image_latents`` is the same for an 8-channel InstructPix2Pix U-Net
        (ops.conv_in_pix2pix): ``sample`` is the 4-channel latents, channels 4-7 come from the image latents, and a conditioning batch
        of three times the latents' selects the (text, image, uncond) rows, the last with a zero image, as the reference's
        ``cat([image_latents, image_latents, zeros_like(image_latents)])`` builds them; it honours ``scale_model_input`` and is not
        combined with ``inpaint_cond``.  An 8-channel ``sample`` without it goes through the ordinary conv_in.  ``controlnet_handoff``: a callable ``f(skips, mid)`` that adds a ControlNet's residuals
        with the engine's own launches (``ControlNetModel.handoff_``): called once, after the mid block, with the channels-last skip
        list of the down blocks and the mid block's output, it updates those tensors IN PLACE -- no torch op, so the step stays
        recordable as a strict launch plan.  Not together with the two reference residual arguments.

        Handled like the reference: ``encoder_attention_mask`` (key-padding mask of the text tokens, :1071-1073, through the
        masked flash kernel), ``down_block_additional_residuals`` / ``mid_block_additional_residual`` (ControlNet, :1178-1222:
        added to the skip connections / the mid-block output), ``cross_attention_kwargs`` that change nothing
        (``None``, ``{}``, ``{"scale": 1.0}``).  Refused loudly: what has no engine path (self-attention ``attention_mask``,
        ``class_labels``, T2I-Adapter intra-block residuals, GLIGEN, a LoRA ``scale`` != 1 -- fuse the
        adapter with ``fuse_lora(scale)`` instead)."""
        if not self._built:
            raise RuntimeError("UNet2DConditionModel: call load_state_dict() first")
        for name, v in (("class_labels", class_labels), ("attention_mask", attention_mask),
                        ("down_intrablock_additional_residuals", down_intrablock_additional_residuals)):
            if v is not None:
                raise ValueError(f"diffusers_amd UNet2DConditionModel.forward: `{name}` is not supported on the HIP path")
        if timestep_cond is not None and self.config.time_cond_proj_dim is None:
            self._check_timestep_cond(timestep_cond, 0)      # refused by name
        if cross_attention_kwargs:
            extra = {k: v for k, v in cross_attention_kwargs.items() if not (k == "scale" and float(v) == 1.0)}
            if extra:
                raise ValueError(f"diffusers_amd UNet2DConditionModel.forward: cross_attention_kwargs {sorted(extra)} are not "
                                 "supported on the HIP path (LoRA scales: fuse_lora(scale) packs them into the weights)")
        if (down_block_additional_residuals is None) != (mid_block_additional_residual is None):
            raise ValueError("ControlNet residuals: pass both down_block_additional_residuals and "
                             "mid_block_additional_residual (unet_2d_condition.py:1104)")
        if controlnet_handoff is not None and down_block_additional_residuals is not None:
            raise ValueError("`controlnet_handoff` and down_block_additional_residuals / mid_block_additional_residual are two "
                             "ways to add the same residuals: pass one")
        ops.require_hip(sample, "sample")
        c = self.config
        B, Cin, H, W_ = sample.shape
        n_up = len(c.block_out_channels) - 1
        if H % (2 ** n_up) or W_ % (2 ** n_up):
            raise ValueError("sample height/width must be divisible by 2**(num_upsamplers)")
        if conditioning is None:
            conditioning = self._cached_conditioning(encoder_hidden_states, added_cond_kwargs, encoder_attention_mask, timestep_cond)
        elif encoder_attention_mask is not None:
            raise ValueError("pass encoder_attention_mask to precompute_conditioning() when `conditioning` is given")
        elif timestep_cond is not None:
            raise ValueError("pass timestep_cond to precompute_conditioning() when `conditioning` is given")
        if c.time_cond_proj_dim is not None and conditioning.get("timestep_cond") is None:
            raise ValueError(f"this U-Net has time_cond_proj_dim={c.time_cond_proj_dim}: `timestep_cond` is required "
                             "(forward(timestep_cond=) or precompute_conditioning(timestep_cond=))")
        if image_cond is not None:
            if inpaint_cond is not None:
                raise ValueError("`image_cond` (InstructPix2Pix, 8 input channels) and `inpaint_cond` (inpainting, 9) exclude each other")
            if c.in_channels != 8 or Cin != 4:
                raise ValueError(f"`image_cond` is for a U-Net with 8 input channels fed 4-channel latents (this one has "
                                 f"{c.in_channels}, `sample` has {Cin})")
            if scale_model_input and sampler_table is None:
                raise ValueError("`scale_model_input` reads the sampler table: pass `sampler_table` / `step_idx`")
            rep = conditioning["batch"] // B
            if rep not in (1, 3) or rep * B != conditioning["batch"]:
                raise ValueError("conditioning batch must be the latents' batch, or three times it (text, image, unconditional)")
            B = rep * B
        elif inpaint_cond is not None:
            if c.in_channels != 9 or Cin != 4:
                raise ValueError(f"`inpaint_cond` is for a U-Net with 9 input channels fed 4-channel latents (this one has "
                                 f"{c.in_channels}, `sample` has {Cin})")
            if scale_model_input and sampler_table is None:
                raise ValueError("`scale_model_input` reads the sampler table: pass `sampler_table` / `step_idx`")
            rep = conditioning["batch"] // B
            if rep not in (1, 2) or rep * B != conditioning["batch"]:
                raise ValueError("conditioning batch must be the latents' batch, or twice it (classifier-free guidance)")
            B = rep * B
        elif scale_model_input:
            raise ValueError("`scale_model_input` is an option of `inpaint_cond` / `image_cond`")
        if conditioning["batch"] != B:
            raise ValueError("conditioning batch does not match sample batch")
        kvs = conditioning["kvs"]

        # 1. time embedding (unet_2d_condition.py:852-872, :1081-1098)
        if sampler_table is not None:
            t_emb = ops.timestep_embedding(None, c.block_out_channels[0], batch=B, flip_sin_to_cos=c.flip_sin_to_cos,
                                           shift=float(c.freq_shift), table=sampler_table, step_idx=step_idx)
        else:
            if not torch.is_tensor(timestep):
                timestep = torch.tensor([float(timestep)], dtype=torch.float32)
            t = timestep.to(device=self.device, dtype=torch.float32).reshape(-1)
            if t.numel() == 1:
                t = t.expand(B)
            t_emb = ops.timestep_embedding(t.contiguous(), c.block_out_channels[0], batch=B,
                                           flip_sin_to_cos=c.flip_sin_to_cos, shift=float(c.freq_shift))
        if self.time_cond_proj is not None:
            # embeddings.py:1296-1297: sample + cond_proj(condition) = bf16(t_emb + bf16(cond_proj(c))), the skinny linear's epilogue
            t_emb = ops.linear_small_m(conditioning["timestep_cond"], self.time_cond_proj, None, residual=t_emb)
        emb = self.time_embedding(t_emb, residual=conditioning["aug_emb"])  # emb + aug_emb fused as residual
        emb = self.time_proj(emb)                    # the resnets below take their columns of this

        # 2. conv_in: NCHW -> channels-last
        if image_cond is not None:
            x = ops.conv_in_pix2pix(sample.contiguous(), image_cond, self.conv_in_w, self.conv_in_b,
                                    table=sampler_table if scale_model_input else None,
                                    step_idx=step_idx if scale_model_input else None, rep=rep)
        elif inpaint_cond is not None:
            x = ops.conv_in_inpaint(sample.contiguous(), inpaint_cond[0], inpaint_cond[1], self.conv_in_w, self.conv_in_b,
                                    table=sampler_table if scale_model_input else None,
                                    step_idx=step_idx if scale_model_input else None, rep=rep)
        else:
            x = ops.conv_thin_in(sample.contiguous(), self.conv_in_w, self.conv_in_b, ksize=3, in_nchw=True)

        # 3. down
        x, skips, ki = walk_down(self.down, x, emb, kvs)

        if down_block_additional_residuals is not None:
            # ControlNet (:1191-1200): one residual per skip connection, NCHW like every reference activation; the sum is a
            # bf16 add as in the reference (torch glue on the device: not part of the captured hot loop)
            if len(down_block_additional_residuals) != len(skips):
                raise ValueError(f"down_block_additional_residuals: expected {len(skips)} tensors, got "
                                 f"{len(down_block_additional_residuals)}")
            skips = [s_ + self._nhwc(r, s_) for s_, r in zip(skips, down_block_additional_residuals)]

        # 4. mid
        x, ki = walk_mid(self.mid, x, emb, kvs, ki)
        if mid_block_additional_residual is not None:
            x = x + self._nhwc(mid_block_additional_residual, x)             # :1220-1222
        if controlnet_handoff is not None:
            # after the mid block, not in front of it: the last skip IS the mid block's input, which the reference leaves without
            # a residual (:1191-1200 build new tensors for the skip list only)
            controlnet_handoff(skips, x)

        # 5. up (skip concat fused into the resnets)
        for st in self.up:
            for j, rn in enumerate(st["resnets"]):
                skip = skips.pop()
                x = rn(x, emb, skip=skip)
                if st["attns"]:
                    x = st["attns"][j](x, kvs[ki])
                    ki += 1
            if st["up"] is not None:
                x = st["up"](x)

        # 6. out: GroupNorm + SiLU + conv_out, channels-last -> NCHW
        x = self.conv_norm_out(x, silu=True)
        out = ops.conv_thin_out(x, self.conv_out_w, self.conv_out_b)
        if not return_dict:
            return (out,)
        return UNet2DConditionOutput(sample=out)
