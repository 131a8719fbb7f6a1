"""Timing of the ControlNet pipelines per denoising step (HIP-graph replay, CFG 5, seeded random weights: timings only), both legs in
one process on one GPU, alternating, median of the repetitions:

  (a) the text-to-image pipeline
  (b) the ControlNet pipeline over the SAME U-Net, VAE and scheduler objects: (a) + ControlNetModel.features + the hand-off launches

for the tiny SDXL config (16 x 16 latents) and, unless ``--tiny-only``, for SDXL at 1024 x 1024; and the per-step launch of the
conditioning embedding's conv_out (the 3x3 conv that also adds conv_in(latents)) in isolation, as a share of (b) - (a).  Per-step
times are the latent-output call time divided by the step count.  Prints one JSON line.

    python tools/bench_controlnet.py [--steps 30] [--reps 5] [--tiny-only]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _kernel_us(fn, iters=100):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def measure(tiny: bool, steps: int, reps: int) -> dict:
    from diffusers_amd import factory, ops
    from diffusers_amd.pipelines import StableDiffusionXLPipeline
    dev, bf16 = torch.device("cuda", 0), torch.bfloat16
    cn = factory.build_sdxl_pipeline(device=dev, tiny=tiny, controlnet=True)
    base = StableDiffusionXLPipeline(vae=cn.vae, unet=cn.unet, scheduler=cn.scheduler)
    c = cn.unet.config
    side = c.sample_size * cn.vae_scale_factor
    seq, cross, pooled = (7, 64, 64) if tiny else (77, 2048, 1280)
    g = torch.Generator().manual_seed(0)
    pe, te = torch.randn(1, seq, cross, generator=g).to(bf16).to(dev), torch.randn(1, pooled, generator=g).to(bf16).to(dev)
    img = torch.rand(1, 3, side, side, generator=g)
    kw = dict(num_inference_steps=steps, guidance_scale=5.0, prompt_embeds=pe, negative_prompt_embeds=pe, pooled_prompt_embeds=te,
              negative_pooled_prompt_embeds=te, output_type="latent")
    legs = {"base": lambda: base(height=side, width=side, generator=torch.Generator().manual_seed(1), **kw).images,
            "controlnet": lambda: cn(image=img, generator=torch.Generator().manual_seed(1), **kw).images}
    for fn in legs.values():          # warm-up: tuning, capture
        fn()
        fn()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(_timed(fn))
    res = {"latents": side // cn.vae_scale_factor, "image": side}
    for k, v in times.items():
        v.sort()
        res[f"{k}_ms_per_step"] = round(v[len(v) // 2] / steps, 4)
        res[f"{k}_ms_per_step_min_max"] = [round(v[0] / steps, 4), round(v[-1] / steps, 4)]
    # the embedding's conv_out alone, on the shapes of a CFG step
    m = cn.controlnet
    ce = m.cond_embedding
    h = side // cn.vae_scale_factor
    embed = torch.randn(2, h, h, ce.out_w.shape[1] // 9, generator=g).to(bf16).to(dev)
    x = torch.randn(2, h, h, ce.out_w.shape[0], generator=g).to(bf16).to(dev)
    us = _kernel_us(lambda: ops.conv2d_nhwc(embed, ce.out_w, ce.out_b, ksize=3, residual=x, k_valid=ce.out_k_valid))
    res["embedding_conv_out_us"] = round(us, 2)
    extra = res["controlnet_ms_per_step"] - res["base_ms_per_step"]
    res["controlnet_extra_ms_per_step"] = round(extra, 4)
    res["embedding_conv_out_share_of_extra"] = round(us / 1e3 / extra, 4) if extra > 0 else None
    res["embedding_conv_out_share_of_step"] = round(us / 1e3 / res["controlnet_ms_per_step"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiny-only", action="store_true")
    args = ap.parse_args()
    out = {"tool": "bench_controlnet", "steps": args.steps, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "tiny_sdxl": measure(True, args.steps, args.reps)}
    if not args.tiny_only:
        out["sdxl_1024"] = measure(False, args.steps, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
