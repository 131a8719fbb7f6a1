"""The CLIP vision front (csrc/clip_patch_embed.hip) and the whole ViT-H encode, timed on one MI355X.

    python tools/bench_clip_vision.py [--reps 5] [--inner 20] > profiles/clip_vision_numbers.md

Front: ONE da_clip_patch_embed launch (uint8 image in, first layer's input out) against the same front as torch ops on the GPU (crop,
rescale, normalise, bf16 conv2d with stride 14, class token, position embedding, layer_norm, zero-padded token matrix), ViT-H
(hidden 1280, 224 x 224, patch 14) at B = 1 and 4.  Encode: the engine's CLIPVisionModelWithProjection against ``transformers``' module in
bf16 on the GPU, same seeded weights, B = 1.  Legs alternate inside one process; a timed call is ``--inner`` back-to-back runs between
two device events, a figure is the median of ``--reps`` such calls with the range.  Seeded data.  Needs a HIP device: no fallback."""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diffusers_amd import factory, ops                                                  # noqa: E402
from diffusers_amd.vision_encoders import CLIP_IMAGE_MEAN as MEAN, CLIP_IMAGE_STD as STD  # noqa: E402
from bench_temporal_attention import measure                                            # noqa: E402

bf16 = torch.bfloat16
DEV = "cuda"
VIT_H = dict(hidden_size=1280, intermediate_size=5120, projection_dim=1024, num_hidden_layers=32, num_attention_heads=16, image_size=224,
             patch_size=14, hidden_act="gelu")


def front_legs(enc, sd, B: int):
    c = enc.config
    S, P, h = c.image_size, c.patch_size, c.hidden_size
    n = 1 + (S // P) ** 2
    S_alloc = (n + 15) // 16 * 16
    img = torch.randint(0, 256, (B, S + 32, S, 3), generator=torch.Generator("cpu").manual_seed(B), dtype=torch.uint8).to(DEV)
    w4 = sd["vision_model.embeddings.patch_embedding.weight"].to(DEV)
    mean, std = (torch.tensor(v, device=DEV).view(1, 3, 1, 1) for v in (MEAN, STD))
    out = torch.zeros((B, S_alloc, h), dtype=bf16, device=DEV)

    def kernel():
        return enc._front(img, size=S, crop=(16, 0), mean=MEAN, std=STD)

    def torch_ops():
        x = ((img[:, 16:16 + S].permute(0, 3, 1, 2).float() / 255.0 - mean) / std).to(bf16)
        e = F.conv2d(x, w4, stride=P).flatten(2).transpose(1, 2)
        e = torch.cat([enc.cls.expand(B, 1, h), e], 1) + enc.pos
        out[:, :n] = F.layer_norm(e, (h,), *enc.pre_ln, c.layer_norm_eps)
        return out
    a, b = kernel().view(B, S_alloc, h).float(), torch_ops().float()
    return {"kernel": kernel, "torch": torch_ops}, float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_vision: needs a HIP device")
    enc, sd = factory.build_clip_vision(VIT_H, seed=8)
    print("# CLIP vision encoder (ViT-H / 14, 224 x 224): measured on one MI355X\n")
    print(f"Per run, median of {args.reps} x {args.inner} runs (range); launched from Python.\n")
    print("| what | B | one launch (da_clip_patch_embed) | torch ops on the GPU | torch / kernel | legs differ by (rel-rms) |")
    print("|---|---|---|---|---|---|")
    for B in (1, 4):
        legs, rr = front_legs(enc, sd, B)
        res = measure(legs, args.reps, args.inner)
        (k, klo, khi), (t, tlo, thi) = res["kernel"], res["torch"]
        print(f"| front: image -> first layer input | {B} | {k:.1f} ({klo:.1f} .. {khi:.1f}) us | {t:.1f} ({tlo:.1f} .. {thi:.1f}) us | "
              f"{t / k:.2f}x | {rr:.2e} |", flush=True)
    import transformers
    theirs = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**VIT_H)).eval()
    theirs.load_state_dict({k: v.float() for k, v in sd.items()})
    theirs = theirs.to(DEV, bf16)
    pv = torch.randn((1, 3, 224, 224), generator=torch.Generator("cpu").manual_seed(0)).to(DEV)
    with torch.no_grad():
        legs = {"engine": lambda: enc(pixel_values=pv).image_embeds, "transformers": lambda: theirs(pixel_values=pv.to(bf16)).image_embeds}
        a, b = legs["engine"]().float(), legs["transformers"]().float()
        res = measure(legs, args.reps, max(1, args.inner // 10))
    (k, klo, khi), (t, tlo, thi) = res["engine"], res["transformers"]
    print(f"\nWhole encode, pixel_values -> image_embeds, B = 1 (32 layers), image_embeds differ by rel-rms "
          f"{float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()):.2e}:\n")
    print(f"- engine: {k / 1e3:.2f} ({klo / 1e3:.2f} .. {khi / 1e3:.2f}) ms", flush=True)
    print(f"- transformers, bf16: {t / 1e3:.2f} ({tlo / 1e3:.2f} .. {thi / 1e3:.2f}) ms", flush=True)
