"""The encoder half of the SD / SDXL U-Net -- down blocks and mid block -- as ``UNet2DConditionModel`` and ``ControlNetModel`` both
build and walk it (unet_2d_condition.py:430-560 / :1128-1222 and controlnets/controlnet.py:330-420 / :800-830 construct and run
the same ``get_down_block`` / ``UNetMidBlock2DCrossAttn`` modules under the same ``state_dict`` names)."""
from __future__ import annotations

from typing import List, Tuple

from .layers import Downsample2D, ResnetBlock2D, Transformer2DModel, Weights


def _tup(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


def block_heads(c) -> tuple:
    """Attention heads per level (the reference's ``num_attention_heads or attention_head_dim`` naming quirk)."""
    return _tup(c.num_attention_heads or c.attention_head_dim, len(c.block_out_channels))


def build_down_blocks(w: Weights, c) -> List[dict]:
    """``down_blocks.*`` of config ``c``: per level ``{"resnets", "attns", "down"}``."""
    n = len(c.block_out_channels)
    groups, eps = c.norm_num_groups, c.norm_eps
    heads, lpb, tlpb = block_heads(c), _tup(c.layers_per_block, n), _tup(c.transformer_layers_per_block, n)
    down = []
    for i, btype in enumerate(c.down_block_types):
        pre = f"down_blocks.{i}"
        stage = {"resnets": [], "attns": [], "down": None}
        for j in range(lpb[i]):
            stage["resnets"].append(ResnetBlock2D(w, f"{pre}.resnets.{j}", groups, eps))
            if btype == "CrossAttnDownBlock2D":
                stage["attns"].append(Transformer2DModel(w, f"{pre}.attentions.{j}", heads[i], tlpb[i], groups))
        if i != n - 1:
            stage["down"] = Downsample2D(w, f"{pre}.downsamplers.0", padding=c.downsample_padding)
        down.append(stage)
    return down


def build_mid_block(w: Weights, c) -> dict:
    """``mid_block.*`` (UNetMidBlock2DCrossAttn): resnet, transformer, resnet."""
    n = len(c.block_out_channels)
    groups, eps = c.norm_num_groups, c.norm_eps
    heads, tlpb = block_heads(c), _tup(c.transformer_layers_per_block, n)
    return {
        "resnets": [ResnetBlock2D(w, "mid_block.resnets.0", groups, eps, c.mid_block_scale_factor),
                    ResnetBlock2D(w, "mid_block.resnets.1", groups, eps, c.mid_block_scale_factor)],
        "attns": [Transformer2DModel(w, "mid_block.attentions.0", heads[-1], tlpb[-1], groups)],
    }


def walk_down(down: List[dict], x, emb, kvs, ki: int = 0) -> Tuple[object, list, int]:
    """The down blocks on ``x`` (channels-last): returns the output, the skip list (``x`` itself first, then one entry per
    resnet / attention pair and per downsampler) and the index of the next unused cross-attention K / V^T of ``kvs``."""
    skips = [x]
    for st in down:
        for j, rn in enumerate(st["resnets"]):
            x = rn(x, emb)
            if st["attns"]:
                x = st["attns"][j](x, kvs[ki])
                ki += 1
            skips.append(x)
        if st["down"] is not None:
            x = st["down"](x)
            skips.append(x)
    return x, skips, ki


def walk_mid(mid: dict, x, emb, kvs, ki: int) -> Tuple[object, int]:
    x = mid["resnets"][0](x, emb)
    x = mid["attns"][0](x, kvs[ki])
    x = mid["resnets"][1](x, emb)
    return x, ki + 1
