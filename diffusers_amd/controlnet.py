"""ControlNetModel on the gfx950 kernels.

Mirrors the reference class (models/controlnets/controlnet.py) for the SD1.5 and SDXL flavours: same constructor kwargs, same
``state_dict`` names / shapes, same ``forward`` arguments and NCHW residuals.  The encoder half is the U-Net's own (unet_blocks.py:
the same blocks under the same names); on top of it sit the conditioning embedding of the control image and the 1x1 "zero convs".

The engine splits ``forward`` where the denoising loop needs it split:

  precompute_conditioning   once per call: cross-attention K / V^T, the SDXL text_time embedding, and the conditioning embedding of
                            the control image up to (not including) its ``conv_out``
  features                  once per step: conv_in(latents) + conv_out(embedding) in one tensor, time embedding, down + mid walk
  handoff_                  once per step, from inside the U-Net forward: every zero conv as ONE launch that scales its output by
                            ``conditioning_scale`` and accumulates it into the U-Net's skip / mid tensor in place

Rounding of the hand-off (the reference: ``sample * conditioning_scale`` on a bf16 tensor with a Python float, then the U-Net's
bf16 add): ``skip' = bf16(skip + bf16(bf16(zero_conv(h)) * s))`` with ``s`` in fp32 -- da_gemm_params.gate_f32 == 2.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import _lib as L
from . import ops
from .config_utils import check_to
from .layers import TimeProjections, TimestepEmbedding, Weights, pad_encoder_states
from .loading import PretrainedMixin
from .unet_2d_condition import FrozenConfig, UNet2DConditionModel
from .unet_blocks import build_down_blocks, build_mid_block, walk_down, walk_mid

bf16 = torch.bfloat16


@dataclass
class ControlNetOutput:
    down_block_res_samples: Tuple[torch.Tensor, ...]
    mid_block_res_sample: torch.Tensor


_DEFAULTS = dict(
    in_channels=4, conditioning_channels=3, flip_sin_to_cos=True, freq_shift=0,
    down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
    mid_block_type="UNetMidBlock2DCrossAttn", only_cross_attention=False, block_out_channels=(320, 640, 1280, 1280),
    layers_per_block=2, downsample_padding=1, mid_block_scale_factor=1, act_fn="silu", norm_num_groups=32, norm_eps=1e-5,
    cross_attention_dim=1280, transformer_layers_per_block=1, encoder_hid_dim=None, encoder_hid_dim_type=None,
    attention_head_dim=8, num_attention_heads=None, use_linear_projection=False, class_embed_type=None,
    addition_embed_type=None, addition_time_embed_dim=None, num_class_embeds=None, upcast_attention=False,
    resnet_time_scale_shift="default", projection_class_embeddings_input_dim=None,
    controlnet_conditioning_channel_order="rgb", conditioning_embedding_out_channels=(16, 32, 96, 256),
    global_pool_conditions=False, addition_embed_type_num_heads=64,
)


def _pad64(c: int) -> int:
    return (c + 63) // 64 * 64


def _pad_conv(w: torch.Tensor, b: torch.Tensor):
    """[Cout][Cin][3][3] / [Cout] -> both channel counts zero-padded to the implicit-GEMM kernel's 64-wide granule, packed.  The
    padded output channels have zero weights AND zero bias, so they are 0 after the conv and stay 0 through SiLU; the padded
    input channels are the next conv's ``k_valid`` tail."""
    co, ci = w.shape[0], w.shape[1]
    cop, cip = _pad64(co), _pad64(ci)
    if (cop, cip) != (co, ci):
        wp = torch.zeros((cop, cip, 3, 3), device=w.device, dtype=w.dtype)
        wp[:co, :ci] = w
        bp = torch.zeros((cop,), device=b.device, dtype=b.dtype)
        bp[:co] = b
        w, b = wp, bp
    return ops.pack_conv_weight(w), b.contiguous()


class ConditioningEmbedding:
    """ControlNetConditioningEmbedding (controlnet.py:50-95): conv_in, SiLU, then per stage a 3x3 conv and a stride-2 3x3 conv with
    SiLU after each, then conv_out.  conv_in reads the 3-channel image through the thin-input kernels; every later conv is an
    implicit GEMM on channels zero-padded to 64 (``k_valid`` = the real count).  ``conv_out`` is NOT run here: it is the per-step
    launch that also adds conv_in(latents) (ControlNetModel.features)."""

    def __init__(self, w: Weights, prefix: str, channels: Tuple[int, ...], out_channels: int):
        wi, bi = w.get(prefix + ".conv_in.weight"), w.get(prefix + ".conv_in.bias")
        c0, c0p = channels[0], _pad64(channels[0])
        wp = torch.zeros((c0p,) + tuple(wi.shape[1:]), device=wi.device, dtype=wi.dtype)
        wp[:c0] = wi
        bp = torch.zeros((c0p,), device=bi.device, dtype=bi.dtype)
        bp[:c0] = bi
        self.conv_in_w, self.conv_in_b = ops.pack_conv_weight(wp), bp
        # SiLU of conv_in's output: the thin-input kernels have no activation, so it rides the epilogue of an identity 1x1 GEMM
        # (x . 1 accumulates exactly; the epilogue rounds to bf16 and applies SiLU like every other launch)
        self.eye = torch.eye(c0p, device=wi.device, dtype=wi.dtype).contiguous()
        self.convs: List[dict] = []
        for i in range(len(channels) - 1):
            for j, (stride, ci) in enumerate(((1, channels[i]), (2, channels[i]))):
                cw, cb = _pad_conv(w.get(f"{prefix}.blocks.{2 * i + j}.weight"), w.get(f"{prefix}.blocks.{2 * i + j}.bias"))
                self.convs.append({"w": cw, "b": cb, "stride": stride, "k_valid": ci})
        self.out_w, self.out_b = _pad_conv(w.get(prefix + ".conv_out.weight"), w.get(prefix + ".conv_out.bias"))
        self.out_k_valid = channels[-1]
        self.scale = 2 ** (len(channels) - 1)
        if self.out_w.shape[0] != out_channels:
            raise ValueError(f"{prefix}.conv_out: {out_channels} output channels must be a multiple of 64")

    def embed(self, image: torch.Tensor, nchw: bool) -> torch.Tensor:
        """The embedding in front of conv_out: NHWC bf16 [B][H / scale][W / scale][pad64(channels[-1])]."""
        if image.dtype == bf16:
            h = ops.conv_thin_in(image.contiguous(), self.conv_in_w, self.conv_in_b, ksize=3, in_nchw=nchw)
        else:
            h = ops.vae_conv_in_image(image.contiguous(), self.conv_in_w, self.conv_in_b, nchw=nchw, normalize=False)
        B, H, W_, C = h.shape
        h = ops.linear(h.view(B * H * W_, C), self.eye, act=L.ACT_SILU).view(B, H, W_, C)
        for cv in self.convs:
            h = ops.conv2d_nhwc(h, cv["w"], cv["b"], ksize=3, stride=cv["stride"], act=L.ACT_SILU, k_valid=cv["k_valid"])
        return h


class ControlNetModel(PretrainedMixin):
    """Drop-in for the reference ``ControlNetModel`` (inference, bf16, HIP device only; SD1.5 and SDXL flavours)."""

    def __init__(self, **kwargs):
        unknown = set(kwargs) - set(_DEFAULTS)
        if unknown:
            raise TypeError(f"ControlNetModel: unexpected config keys {sorted(unknown)}")
        cfg = dict(_DEFAULTS)
        cfg.update(kwargs)
        self.config = FrozenConfig(cfg)
        c = self.config
        if c.class_embed_type is not None or c.num_class_embeds is not None:
            raise ValueError("diffusers_amd ControlNetModel: `class_embed_type` / `num_class_embeds` are not implemented")
        if c.global_pool_conditions:
            raise NotImplementedError("diffusers_amd ControlNetModel: `global_pool_conditions=True` is not implemented")
        if c.addition_embed_type not in (None, "text_time"):
            raise ValueError(f"diffusers_amd ControlNetModel: addition_embed_type={c.addition_embed_type!r} is not supported "
                             "(None or 'text_time')")
        if c.conditioning_channels != 3:
            raise ValueError(f"diffusers_amd ControlNetModel: conditioning_channels={c.conditioning_channels} -- the control image "
                             "has 3 channels")
        if c.act_fn != "silu" or c.resnet_time_scale_shift != "default":
            raise ValueError("diffusers_amd ControlNetModel supports act_fn='silu', default time scale shift")
        if c.only_cross_attention or c.upcast_attention or c.encoder_hid_dim is not None or c.encoder_hid_dim_type is not None:
            raise ValueError("diffusers_amd ControlNetModel: unsupported attention variant / encoder_hid projection")
        if c.controlnet_conditioning_channel_order != "rgb":
            raise ValueError(f"unknown `controlnet_conditioning_channel_order`: {c.controlnet_conditioning_channel_order} "
                             "(the engine reads rgb)")
        if len(c.block_out_channels) != len(c.down_block_types):
            raise ValueError("Must provide the same number of `block_out_channels` as `down_block_types`.")
        for t in c.down_block_types:
            if t not in ("CrossAttnDownBlock2D", "DownBlock2D"):
                raise ValueError(f"{t} does not exist.")
        if c.mid_block_type != "UNetMidBlock2DCrossAttn":
            raise ValueError(f"unknown mid_block_type : {c.mid_block_type}")
        if len(c.conditioning_embedding_out_channels) < 1:
            raise ValueError("conditioning_embedding_out_channels must name at least one channel count")
        self.dtype = bf16
        self.device = None
        self._built = False

    # ------------------------------------------------------------------------------------------------------------
    # weights
    # ------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], device="cuda", strict: bool = True):
        """Pack a reference-format state_dict (keys as ``reference_controlnet.state_dict()``) onto ``device``."""
        c = self.config
        w = Weights(state_dict, device)
        self.device = torch.device(device)
        self._new_weights_generation()
        self._cond_cache = None
        boc = tuple(c.block_out_channels)
        self.conv_in_w = ops.pack_conv_weight(w.get("conv_in.weight"))
        self.conv_in_b = w.get("conv_in.bias")
        self.time_embedding = TimestepEmbedding(w, "time_embedding")
        self.add_embedding = TimestepEmbedding(w, "add_embedding") if c.addition_embed_type == "text_time" else None
        self.cond_embedding = ConditioningEmbedding(w, "controlnet_cond_embedding", tuple(c.conditioning_embedding_out_channels),
                                                    boc[0])
        self.down = build_down_blocks(w, c)
        self.mid = build_mid_block(w, c)
        self.time_proj = TimeProjections([r for st in self.down for r in st["resnets"]] + self.mid["resnets"])
        # the zero convs: [C][C] 1x1 weights, one per skip connection (walk_down's list order), then the mid block's
        n_skips = 1 + sum(len(st["resnets"]) + (st["down"] is not None) for st in self.down)
        self.zero_w, self.zero_b = [], []
        for k in range(n_skips):
            zw = w.get(f"controlnet_down_blocks.{k}.weight")
            self.zero_w.append(zw.reshape(zw.shape[0], -1).contiguous())
            self.zero_b.append(w.get(f"controlnet_down_blocks.{k}.bias"))
        zw = w.get("controlnet_mid_block.weight")
        self.zero_w.append(zw.reshape(zw.shape[0], -1).contiguous())
        self.zero_b.append(w.get("controlnet_mid_block.bias"))
        if strict and w.unused():
            raise RuntimeError(f"unexpected keys in state_dict: {w.unused()[:8]} ...")
        self._built = True
        return self

    def to(self, *args, **kwargs):
        return check_to(self, args, kwargs)

    def eval(self):
        return self

    @property
    def conditioning_scale_factor(self) -> int:
        """Control-image pixels per latent pixel (8 for the shipped checkpoints: three stride-2 stages)."""
        return 2 ** (len(self.config.conditioning_embedding_out_channels) - 1)

    # ------------------------------------------------------------------------------------------------------------
    # once per call
    # ------------------------------------------------------------------------------------------------------------
    def _transformers(self):
        out = []
        for st in self.down:
            out += st["attns"]
        return out + self.mid["attns"]

    def _image(self, image: torch.Tensor, nchw: Optional[bool], batch: int) -> Tuple[torch.Tensor, bool]:
        """The control image on the device, in one of the layouts the thin-input kernels read, repeated to ``batch``."""
        if not torch.is_tensor(image) or image.dim() != 4:
            raise ValueError("ControlNetModel: the control image must be a 4-D tensor (NCHW, or NHWC for uint8 / fp32 pixels)")
        if nchw is None:
            nchw = not (image.dtype == torch.uint8 or (image.shape[1] != 3 and image.shape[3] == 3))
        if image.dtype == torch.uint8 and nchw:
            raise ValueError("ControlNetModel: uint8 control images are NHWC")
        if image.dtype not in (torch.uint8, torch.float32, bf16):
            image = image.to(torch.float32)
        if image.dtype == bf16 and not nchw:
            raise ValueError("ControlNetModel: bf16 control images are NCHW")
        ch = image.shape[1] if nchw else image.shape[3]
        if ch != 3:
            raise ValueError(f"ControlNetModel: the control image has {ch} channels, 3 expected")
        image = image.to(self.device)
        if image.shape[0] != batch:
            if batch % image.shape[0]:
                raise ValueError(f"ControlNetModel: {image.shape[0]} control images for a batch of {batch}")
            image = image.repeat(batch // image.shape[0], 1, 1, 1)
        return image.contiguous(), nchw

    def precompute_conditioning(self, encoder_hidden_states: torch.Tensor,
                                added_cond_kwargs: Optional[Dict[str, torch.Tensor]] = None, image: torch.Tensor = None,
                                image_nchw: Optional[bool] = None, conditioning_scale: float = 1.0) -> Dict[str, Any]:
        """Everything in forward() that depends neither on the timestep nor on the latents: the K / V^T of this model's own
        cross-attention layers, ``aug_emb``, the conditioning embedding of ``image`` up to its conv_out (``embed``) and the fp32
        ``[batch][max channels]`` vector of ``conditioning_scale`` the zero convs take as their gate.  ``image``: pixels in [0, 1],
        NCHW bf16 / fp32 or NHWC uint8 / fp32, one per sample or a divisor of the batch."""
        ops.require_hip(encoder_hidden_states, "encoder_hidden_states")
        if image is None:
            raise ValueError("ControlNetModel.precompute_conditioning: `image` (the control image) is required")
        B = encoder_hidden_states.shape[0]
        ehs_pad, skv, skv_alloc = pad_encoder_states(encoder_hidden_states.contiguous())
        kvs = [tr.precompute_kv(ehs_pad, B, skv, skv_alloc, None) for tr in self._transformers()]
        aug = None
        if self.config.addition_embed_type == "text_time":
            aug = self._text_time_embedding(added_cond_kwargs, B)
        img, nchw = self._image(image, image_nchw, B)
        embed = self.cond_embedding.embed(img, nchw)
        gate = torch.full((B, max(self.config.block_out_channels)), float(conditioning_scale), device=self.device,
                          dtype=torch.float32)
        return {"kvs": kvs, "aug_emb": aug, "batch": B, "embed": embed, "gate": gate}

    def _text_time_embedding(self, added_cond_kwargs, B):
        # (the U-Net's, config names included: controlnet.py:760-785 is unet_2d_condition.py:906-922)
        return UNet2DConditionModel._text_time_embedding(self, added_cond_kwargs, B)

    # ------------------------------------------------------------------------------------------------------------
    # once per step
    # ------------------------------------------------------------------------------------------------------------
    def features(self, x_in: torch.Tensor, conditioning: Dict[str, Any], sampler_table=None, step_idx=None,
                 timestep=None) -> List[torch.Tensor]:
        """The down-block skips and the mid-block output (channels-last, BEFORE their zero convs; the mid output last) for the
        NCHW latents ``x_in``.  The timestep comes from the device-resident sampler table (``sampler_table`` / ``step_idx``,
        graph-replayable) or from ``timestep``."""
        if not self._built:
            raise RuntimeError("ControlNetModel: call load_state_dict() first")
        ops.require_hip(x_in, "sample")
        c = self.config
        B, _, H, W_ = x_in.shape
        if conditioning["batch"] != B:
            raise ValueError("conditioning batch does not match sample batch")
        embed, ce = conditioning["embed"], self.cond_embedding
        if tuple(embed.shape[:3]) != (B, H, W_):
            raise ValueError(f"the control image embeds to {tuple(embed.shape[1:3])}, the latents are {(H, W_)}: the image must be "
                             f"{ce.scale} x the latents' size")
        n_down = len(c.block_out_channels) - 1
        if H % (2 ** n_down) or W_ % (2 ** n_down):
            raise ValueError("sample height/width must be divisible by 2**(num_downsamplers)")
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
        emb = self.time_embedding(t_emb, residual=conditioning["aug_emb"])
        emb = self.time_proj(emb)
        # conv_in(x) + controlnet_cond_embedding(image) (controlnet.py:795-797) as ONE tensor: the embedding's conv_out takes
        # conv_in's output as its residual (no launch entry point adds two tensors)
        x = ops.conv_thin_in(x_in.contiguous(), self.conv_in_w, self.conv_in_b, ksize=3, in_nchw=True)
        x = ops.conv2d_nhwc(embed, ce.out_w, ce.out_b, ksize=3, residual=x, k_valid=ce.out_k_valid)
        x, skips, ki = walk_down(self.down, x, emb, conditioning["kvs"])
        x, _ = walk_mid(self.mid, x, emb, conditioning["kvs"], ki)
        return skips + [x]

    def handoff_(self, skips: List[torch.Tensor], mid: torch.Tensor, features: List[torch.Tensor], gate: torch.Tensor) -> None:
        """``skips[k] += bf16(zero_conv_k(features[k]) * scale)`` and the same for ``mid`` with the last feature, in place: one
        1x1-conv launch each (gate_f32 == 2: see the module docstring).  ``gate``: fp32 [batch][>= channels] holding the scale."""
        targets = list(skips) + [mid]
        if len(targets) != len(features) or len(features) != len(self.zero_w):
            raise ValueError(f"ControlNetModel.handoff_: {len(targets)} targets, {len(features)} features, "
                             f"{len(self.zero_w)} zero convs")
        for tgt, f, zw, zb in zip(targets, features, self.zero_w, self.zero_b):
            if tuple(tgt.shape) != tuple(f.shape):
                raise ValueError(f"ControlNetModel.handoff_: feature {tuple(f.shape)} does not match the U-Net's {tuple(tgt.shape)}")
            ops.conv2d_nhwc(f, zw, zb, ksize=1, gate=gate[:, :zw.shape[0]], gate_round=True, residual=tgt, out=tgt)

    def handoff(self, features: List[torch.Tensor], gate: torch.Tensor):
        """The callable ``UNet2DConditionModel.forward(controlnet_handoff=)`` takes."""
        return lambda skips, mid: self.handoff_(skips, mid, features, gate)

    # ------------------------------------------------------------------------------------------------------------
    # the reference's forward
    # ------------------------------------------------------------------------------------------------------------
    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    def forward(self, sample: torch.Tensor, timestep, encoder_hidden_states: torch.Tensor, controlnet_cond: torch.Tensor,
                conditioning_scale: float = 1.0, class_labels=None, timestep_cond=None, attention_mask=None,
                added_cond_kwargs=None, cross_attention_kwargs=None, guess_mode: bool = False, return_dict: bool = True):
        """controlnet.py:676-870: the residuals ``(down_block_res_samples, mid_block_res_sample)`` as NCHW bf16 tensors, already
        multiplied by ``conditioning_scale``.  Built from the engine methods above: the features handed off into zero tensors."""
        if not self._built:
            raise RuntimeError("ControlNetModel: call load_state_dict() first")
        for name, v in (("class_labels", class_labels), ("timestep_cond", timestep_cond), ("attention_mask", attention_mask)):
            if v is not None:
                raise ValueError(f"diffusers_amd ControlNetModel.forward: `{name}` is not supported on the HIP path")
        if cross_attention_kwargs:
            extra = {k: v for k, v in cross_attention_kwargs.items() if not (k == "scale" and float(v) == 1.0)}
            if extra:
                raise ValueError(f"diffusers_amd ControlNetModel.forward: cross_attention_kwargs {sorted(extra)} are not supported")
        if guess_mode:
            raise NotImplementedError("diffusers_amd ControlNetModel.forward: `guess_mode=True` is not implemented")
        if isinstance(conditioning_scale, (list, tuple)) or torch.is_tensor(conditioning_scale):
            raise NotImplementedError("diffusers_amd ControlNetModel.forward: one float `conditioning_scale`")
        ehs = encoder_hidden_states
        if ehs.dtype != bf16 or not ehs.is_cuda:
            ehs = ehs.to(device=self.device, dtype=bf16)
        cond = self.precompute_conditioning(ehs, added_cond_kwargs, controlnet_cond, conditioning_scale=conditioning_scale)
        feats = self.features(sample, cond, timestep=timestep)
        outs = [torch.zeros_like(f) for f in feats]
        self.handoff_(outs[:-1], outs[-1], feats, cond["gate"])
        outs = [o.permute(0, 3, 1, 2).contiguous() for o in outs]
        if not return_dict:
            return tuple(outs[:-1]), outs[-1]
        return ControlNetOutput(down_block_res_samples=tuple(outs[:-1]), mid_block_res_sample=outs[-1])
