"""AnimateDiff motion modules (models/unets/unet_motion_model.py: MotionAdapter, MotionModules, AnimateDiffTransformer3D -- older name
TransformerTemporalModel) on the engine's kernels.

Activations stay what the SD 1.5 U-Net with frames folded into its batch keeps: a frame-major channels-last token matrix
``x[(b F + f) HW + p][C]``.  The reference permutes to (B HW, F, C) around every module; here the only layer that looks along the
frame axis, the attention, reads that layout in place (csrc/attention_temporal.hip).  The position embedding in front of each
attention is added inside the fused Q | K | V projection: (LN(x) + pe[f]) W^T = LN(x) W^T + (pe W^T)[f], and ``pe W^T`` is a per-frame
row vector of the GEMM epilogue (``ops.linear(rowvec=, rows_per_batch=HW)``), made once per (batch, frames) on the host, outside the
step.  No torch arithmetic runs in a forward.

``MotionAdapter`` loads like every other model (``from_pretrained`` with the pack-once cache, ``from_state_dict``, seeded through
``factory.build_motion_adapter``); ``UNetMotionModel.from_unet2d`` puts its modules between the layers of a loaded SD 1.5
``UNet2DConditionModel`` (sharing that model's packed weights), and ``pipelines.AnimateDiffPipeline`` runs it.  Refused by name: motion
LoRA, more than 32 frames (context windows / FreeNoise), FreeU and ControlNet next to the motion modules, SDXL adapters."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch

from . import ops
from .layers import FeedForwardGEGLU, GroupNorm, LayerNorm, Linear, Weights
from .loading import PretrainedMixin
from .unet_2d_condition import FrozenConfig, UNet2DConditionModel, UNet2DConditionOutput

bf16 = torch.bfloat16
MAX_FRAMES = 32      # da_attention_temporal_bf16: all keys of a sequence fit one MFMA tile


def sinusoidal_pe(channels: int, max_len: int = MAX_FRAMES) -> torch.Tensor:
    """embeddings.py SinusoidalPositionalEmbedding: pe[pos, 0::2] = sin(pos w), pe[pos, 1::2] = cos(pos w), fp32 as the reference."""
    pos = torch.arange(max_len).unsqueeze(1)
    w = torch.exp(torch.arange(0, channels, 2) * (-math.log(10000.0) / channels))
    pe = torch.zeros(max_len, channels)
    pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * w), torch.cos(pos * w)
    return pe


class _TemporalSelfAttention:
    """attn1 / attn2 of the module's block: to_q / to_k / to_v (no bias) as ONE projection with the position row vector, the temporal
    kernel on its three column blocks, to_out.0 (bias) with the residual in its epilogue."""

    def __init__(self, w: Weights, prefix: str, heads: int, pe: torch.Tensor):
        self.wqkv = torch.cat([w.get(f"{prefix}.to_{n}.weight") for n in "qkv"], dim=0).contiguous()
        self.to_out = Linear(w, prefix + ".to_out.0")
        self.heads, self.channels = heads, self.wqkv.shape[1]
        # (pe W^T)[f]: fp32 product of the bf16 weights the GEMM reads, rounded once
        self.pe_w = (pe.to(self.wqkv.device, torch.float32) @ self.wqkv.float().t()).to(bf16).contiguous()
        self._rowvec: Dict[Tuple[int, int], torch.Tensor] = {}

    def rowvec(self, batch: int, frames: int) -> torch.Tensor:
        rv = self._rowvec.get((batch, frames))
        if rv is None:
            rv = self._rowvec[(batch, frames)] = self.pe_w[:frames].repeat(batch, 1).contiguous()     # row b F + f
        return rv

    def __call__(self, normed, residual, batch: int, frames: int, hw: int):
        Cc = self.channels
        qkv = ops.linear(normed, self.wqkv, rowvec=self.rowvec(batch, frames), rows_per_batch=hw)
        o = ops.temporal_attention(qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], B=batch, F=frames, HW=hw, H=self.heads,
                                   D=Cc // self.heads)
        return self.to_out(o, residual=residual)


class MotionModule:
    """AnimateDiffTransformer3D with one BasicTransformerBlock (double_self_attention, sinusoidal positions, GEGLU):
    GroupNorm over ALL frames of a sample -> proj_in -> x += attn1(LN1 x + pe) -> x += attn2(LN2 x + pe) -> x += FF(LN3 x) ->
    proj_out -> + input."""

    def __init__(self, w: Weights, prefix: str, heads: int = 8, groups: int = 32, max_seq_length: int = MAX_FRAMES):
        tb = prefix + ".transformer_blocks.0"
        self.norm = GroupNorm(w, prefix + ".norm", groups, 1e-6)
        self.proj_in = Linear(w, prefix + ".proj_in")
        self.channels = self.proj_in.weight.shape[0]
        if (self.channels // heads) not in (40, 80, 160) or self.channels % heads:
            raise NotImplementedError(f"MotionModule: {self.channels} channels over {heads} heads: the temporal attention kernel has head "
                                      "sizes 40 / 80 / 160")
        # a checkpoint's ``pos_embed.pe`` is a buffer holding this same table: it is computed, and the key counts as consumed
        pe = sinusoidal_pe(self.channels, max_seq_length)
        w.used.add(tb + ".pos_embed.pe")
        self.max_frames = min(int(pe.shape[0]), MAX_FRAMES)
        self.norm1, self.norm2, self.norm3 = (LayerNorm(w, f"{tb}.norm{i}") for i in (1, 2, 3))
        self.attn1 = _TemporalSelfAttention(w, tb + ".attn1", heads, pe[:MAX_FRAMES])
        self.attn2 = _TemporalSelfAttention(w, tb + ".attn2", heads, pe[:MAX_FRAMES])
        self.ff = FeedForwardGEGLU(w, tb + ".ff")
        self.proj_out = Linear(w, prefix + ".proj_out")

    def __call__(self, x: torch.Tensor, num_frames: int) -> torch.Tensor:
        """x: [B*F][H][W][C] (or [B*F][HW][C]) bf16, frames of a sample adjacent; returns the same shape."""
        ops.require_hip(x, "MotionModule input")
        if not 1 <= num_frames <= self.max_frames:
            raise NotImplementedError(f"MotionModule: num_frames must be in 1 .. {self.max_frames} (longer videos need context windows, "
                                      f"which are not built), got {num_frames}")
        if x.shape[0] % num_frames or x.shape[-1] != self.channels or not x.is_contiguous():
            raise ValueError(f"MotionModule: expected contiguous [B*{num_frames}][...][{self.channels}], got {tuple(x.shape)}")
        Cc, batch = self.channels, x.shape[0] // num_frames
        rows = x.numel() // Cc
        hw = rows // x.shape[0]
        res = x.view(rows, Cc)
        h = self.norm(x.view(batch, num_frames * hw, Cc)).view(rows, Cc)       # one slab = the F HW rows of a sample
        h = self.proj_in(h)
        h = self.attn1(self.norm1(h), h, batch, num_frames, hw)
        h = self.attn2(self.norm2(h), h, batch, num_frames, hw)
        h = self.ff(self.norm3(h), residual=h)
        return self.proj_out(h, residual=res).view(x.shape)


def motion_adapter_param_shapes(cfg: dict) -> Dict[str, Tuple[int, ...]]:
    """Reference state_dict keys and shapes of a MotionAdapter (the ``pos_embed.pe`` buffers are not parameters: computed at load)."""
    boc = tuple(cfg["block_out_channels"])
    n, mid = cfg["motion_layers_per_block"], cfg["motion_mid_block_layers_per_block"]
    mods = [(f"down_blocks.{i}.motion_modules.{j}", c) for i, c in enumerate(boc) for j in range(n)]
    mods += [(f"up_blocks.{i}.motion_modules.{j}", c) for i, c in enumerate(reversed(boc)) for j in range(n + 1)]
    if cfg["use_motion_mid_block"]:
        mods += [(f"mid_block.motion_modules.{j}", boc[-1]) for j in range(mid)]
    shapes: Dict[str, Tuple[int, ...]] = {}
    for p, c in mods:
        tb = p + ".transformer_blocks.0"
        shapes.update({f"{p}.norm.weight": (c,), f"{p}.norm.bias": (c,), f"{p}.proj_in.weight": (c, c), f"{p}.proj_in.bias": (c,),
                       f"{p}.proj_out.weight": (c, c), f"{p}.proj_out.bias": (c,)})
        for i in (1, 2, 3):
            shapes.update({f"{tb}.norm{i}.weight": (c,), f"{tb}.norm{i}.bias": (c,)})
        for a in ("attn1", "attn2"):
            shapes.update({f"{tb}.{a}.to_{n_}.weight": (c, c) for n_ in "qkv"})
            shapes.update({f"{tb}.{a}.to_out.0.weight": (c, c), f"{tb}.{a}.to_out.0.bias": (c,)})
        shapes.update({f"{tb}.ff.net.0.proj.weight": (8 * c, c), f"{tb}.ff.net.0.proj.bias": (8 * c,),
                       f"{tb}.ff.net.2.weight": (c, 4 * c), f"{tb}.ff.net.2.bias": (c,)})
    return shapes




class MotionAdapter(PretrainedMixin):
    """The reference's MotionAdapter: the motion modules of an SD 1.5 U-Net, by block.  ``down[i]`` / ``up[i]`` / ``mid`` are lists of
    :class:`MotionModule`.  ``from_pretrained(local_dir)`` reads ``config.json`` + safetensors and keeps the packed weights (the fused
    Q | K | V rows, the ``pe W^T`` row vectors, the interleaved GEGLU rows) in the pack-once cache next to the checkpoint."""

    DEFAULTS = dict(block_out_channels=(320, 640, 1280, 1280), motion_layers_per_block=2, motion_mid_block_layers_per_block=1,
                    motion_num_attention_heads=8, motion_norm_num_groups=32, motion_max_seq_length=32, use_motion_mid_block=True)

    def __init__(self, **config):
        unknown = set(config) - set(self.DEFAULTS)
        if unknown:
            raise TypeError(f"MotionAdapter: unknown config keys {sorted(unknown)}")
        self.config = FrozenConfig(dict(self.DEFAULTS, **config))
        if self.config["motion_max_seq_length"] > MAX_FRAMES:
            raise NotImplementedError(f"MotionAdapter: motion_max_seq_length > {MAX_FRAMES} is not built (the temporal attention kernel "
                                      "holds a sequence in one MFMA tile)")
        self.device = None
        self.down = self.up = self.mid = None

    def load_lora_weights(self, *args, **kwargs):
        raise NotImplementedError("motion LoRA is not built")

    fuse_lora = load_lora_adapter = load_lora_weights

    def load_state_dict(self, state_dict, device="cuda", strict: bool = True):
        c, w = self.config, Weights(state_dict, device)
        self.device = torch.device(device)
        self._new_weights_generation()
        n = c["motion_layers_per_block"]
        mk = lambda p: MotionModule(w, p, c["motion_num_attention_heads"], c["motion_norm_num_groups"], c["motion_max_seq_length"])  # noqa: E731
        nb = len(c["block_out_channels"])
        self.down = [[mk(f"down_blocks.{i}.motion_modules.{j}") for j in range(n)] for i in range(nb)]
        self.up = [[mk(f"up_blocks.{i}.motion_modules.{j}") for j in range(n + 1)] for i in range(nb)]
        self.mid = [mk(f"mid_block.motion_modules.{j}") for j in range(c["motion_mid_block_layers_per_block"])] \
            if c["use_motion_mid_block"] else []
        if strict and w.unused():
            raise ValueError(f"MotionAdapter: {len(w.unused())} unexpected keys in the state_dict, e.g. {w.unused()[:3]}")
        return self

    @classmethod
    def from_state_dict(cls, state_dict, device="cuda", **config) -> "MotionAdapter":
        return cls(**config).load_state_dict(state_dict, device)


class UNetMotionModel(UNet2DConditionModel):
    """The reference's UNetMotionModel for SD 1.5: a loaded ``UNet2DConditionModel`` with a ``MotionAdapter``'s modules after every
    (resnet, attention) pair of the down and up blocks and after the mid block's attention.  Frames are folded into the batch
    (``sample`` [B F][4][h][w], the frames of a sample adjacent; the reference's [B][4][F][h][w] is folded here with one copy each way);
    the spatial layers are the U-Net's own packed weights, shared, not copied.  Text K / V^T and every other per-sample conditioning are
    repeated per frame once, in ``precompute_conditioning(..., num_frames=)``, outside the step."""

    @classmethod
    def from_unet2d(cls, unet: UNet2DConditionModel, motion_adapter: MotionAdapter, **unsupported) -> "UNetMotionModel":
        if unsupported:
            raise NotImplementedError(f"UNetMotionModel.from_unet2d: {sorted(unsupported)} (loading motion weights apart from the "
                                      "adapter) is not built: pass a loaded MotionAdapter")
        if not getattr(unet, "_built", False) or motion_adapter is None or motion_adapter.down is None:
            raise ValueError("UNetMotionModel.from_unet2d needs a loaded UNet2DConditionModel and a loaded MotionAdapter")
        c, m = unet.config, motion_adapter.config
        if c.addition_embed_type is not None:
            raise NotImplementedError("SDXL motion adapters are not built: AnimateDiff here is the SD 1.5 U-Net")
        lpb = c.layers_per_block if isinstance(c.layers_per_block, int) else None
        if tuple(c.block_out_channels) != tuple(m.block_out_channels) or lpb != m.motion_layers_per_block or not m.use_motion_mid_block:
            raise ValueError(f"the MotionAdapter (block_out_channels {tuple(m.block_out_channels)}, {m.motion_layers_per_block} layers per "
                             f"block) does not fit the U-Net ({tuple(c.block_out_channels)}, {c.layers_per_block})")
        if unet._freeu is not None:
            raise NotImplementedError("FreeU with AnimateDiff is not built: disable_freeu() first")
        self = object.__new__(cls)
        self.__dict__.update(unet.__dict__)        # the same packed tensors and weights generation as `unet`
        self.motion_adapter, self._cond_cache, self._frames = motion_adapter, None, 1
        return self

    def load_state_dict(self, *args, **kwargs):
        raise NotImplementedError("UNetMotionModel is built by from_unet2d(unet, motion_adapter) from two loaded models")

    def enable_freeu(self, *args, **kwargs):
        raise NotImplementedError("FreeU with AnimateDiff is not built")

    def graph_token(self) -> tuple:
        return ("motion", self.motion_adapter._weights_generation)

    def _load_ip_adapter_weights(self, state_dicts):
        raise NotImplementedError("IP-Adapter with AnimateDiff is not built (image keys / values are made per sample, not per frame)")

    def precompute_conditioning(self, encoder_hidden_states, added_cond_kwargs=None, encoder_attention_mask=None, timestep_cond=None,
                                num_frames=None):
        """As the U-Net's, for per-SAMPLE inputs: each row is repeated ``num_frames`` times (the frames of a sample adjacent)."""
        F = self._frames if num_frames is None else int(num_frames)
        rep = lambda t: None if t is None else t.repeat_interleave(F, dim=0)      # noqa: E731
        cond = super().precompute_conditioning(rep(encoder_hidden_states), added_cond_kwargs, rep(encoder_attention_mask),
                                               rep(timestep_cond))
        cond["num_frames"] = F
        return cond

    def forward(self, sample, timestep, encoder_hidden_states, *args, num_frames=None, conditioning=None, controlnet_handoff=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None, return_dict: bool = True, **kw):
        if controlnet_handoff is not None or down_block_additional_residuals is not None or mid_block_additional_residual is not None:
            raise NotImplementedError("ControlNet / SparseCtrl with AnimateDiff is not built")
        video = sample.dim() == 5
        if video:
            B, Cin, F, h, w_ = sample.shape
            if num_frames not in (None, F):
                raise ValueError(f"`sample` holds {F} frames, num_frames={num_frames}")
            num_frames, sample = F, sample.permute(0, 2, 1, 3, 4).reshape(B * F, Cin, h, w_)
        if num_frames is None:
            raise ValueError("UNetMotionModel.forward: pass `sample` as [B][C][F][h][w], or folded [B F][C][h][w] with num_frames=")
        F = int(num_frames)
        if not 1 <= F <= MAX_FRAMES:
            raise NotImplementedError(f"num_frames must be in 1 .. {MAX_FRAMES}: longer videos need context windows / FreeNoise, which are "
                                      f"not built (got {F})")
        if sample.shape[0] % F:
            raise ValueError(f"the folded batch {sample.shape[0]} is no multiple of num_frames={F}")
        if conditioning is not None and conditioning.get("num_frames") != F:
            raise ValueError(f"`conditioning` was made for num_frames={conditioning.get('num_frames')}, this call has {F}")
        if F != self._frames:
            self._frames, self._cond_cache = F, None       # the cached conditioning of a drop-in call was repeated for another F
        self._motion = (self.motion_adapter, F)
        try:
            out = super().forward(sample, timestep, encoder_hidden_states, *args, conditioning=conditioning, return_dict=False, **kw)[0]
        finally:
            self._motion = None
        if video:
            out = out.view(B, F, *out.shape[1:]).permute(0, 2, 1, 3, 4).contiguous()
        return UNet2DConditionOutput(sample=out) if return_dict else (out,)
