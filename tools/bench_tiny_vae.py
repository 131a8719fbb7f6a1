"""Timing of AutoencoderTiny against AutoencoderKL (seeded random weights: timings only), every comparison with both legs in one
process on one GPU, alternating, median of the repetitions with min .. max:

  (a) decode      AutoencoderTiny.decode (TAESDXL) vs AutoencoderKL.decode (the SDXL VAE) of 128 x 128 latents, postprocess="uint8"
  (b) per launch  the 64 -> 64 ReLU conv (csrc/conv_c64.hip) at 1024 x 1024 x 64 vs ops.conv2d_nhwc on the same shape with
                  act=NONE (the existing kernel that can run it), and its arithmetic rate
  (c) end to end  the 4-step LCM SDXL image (guidance_scale 1.0, HIP-graph replay, output_type="pt") with either VAE, unless --no-e2e

Prints one JSON line.

    python tools/bench_tiny_vae.py [--reps 5] [--no-e2e] [--latents 128]
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


def _alternate(legs: dict, reps: int, warm: int = 2) -> dict:
    for fn in legs.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(_timed(fn))
    out = {}
    for k, v in times.items():
        v.sort()
        out[k] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    return out


def _event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def decode(reps: int, lat: int) -> dict:
    from diffusers_amd import factory, init as dinit
    dev, bf16 = torch.device("cuda", 0), torch.bfloat16
    tiny, _ = factory.build_tiny_vae(dinit.TAESDXL, seed=1, device=dev, init_device=str(dev), with_encoder=False)
    kl, _ = factory.build_vae(dinit.SDXL_VAE, seed=1, device=dev, init_device=str(dev))
    z = torch.randn(1, 4, lat, lat, generator=torch.Generator().manual_seed(0)).to(bf16).to(dev)
    res = _alternate({"tiny": lambda: tiny.decode(z, latents_div=0.13025, postprocess="uint8"),
                      "kl": lambda: kl.decode(z, latents_div=0.13025, postprocess="uint8")}, reps)
    res["latents"], res["image"] = lat, lat * 8
    res["kl_over_tiny"] = round(res["kl"]["median_ms"] / res["tiny"]["median_ms"], 2)
    return res


def per_launch(reps: int, side: int = 1024) -> dict:
    from diffusers_amd import _lib as L, ops
    dev, bf16 = torch.device("cuda", 0), torch.bfloat16
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, side, side, 64, generator=g).to(bf16).to(dev)
    r = torch.randn(1, side, side, 64, generator=g).to(bf16).to(dev)
    w = (torch.randn(64, 576, generator=g) * 576 ** -0.5).to(bf16).to(dev)
    b = torch.randn(64, generator=g).to(bf16).to(dev)
    out = torch.empty_like(x)
    legs = {"relu_conv": lambda: ops.conv2d_nhwc(x, w, b, act=L.ACT_RELU, out=out),
            "relu_conv_residual": lambda: ops.conv2d_nhwc(x, w, b, residual=r, act=L.ACT_RELU, out=out),
            "existing_conv_act_none": lambda: ops.conv2d_nhwc(x, w, b, out=out)}
    for fn in legs.values():            # warm-up (the existing kernel tunes its variant here)
        for _ in range(3):
            fn()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(_event_ms(fn, 20))
    res = {"shape": [1, side, side, 64]}
    flop = 2.0 * side * side * 64 * 576
    for k, v in times.items():
        v.sort()
        med = v[len(v) // 2]
        res[k] = {"median_us": round(med * 1e3, 1), "min_us": round(v[0] * 1e3, 1), "max_us": round(v[-1] * 1e3, 1),
                  "tflops": round(flop / med / 1e9, 1)}
    return res


def end_to_end(reps: int) -> dict:
    from diffusers_amd import factory, init as dinit
    from diffusers_amd.pipelines import StableDiffusionXLPipeline
    dev, bf16 = torch.device("cuda", 0), torch.bfloat16
    kl = factory.build_sdxl_pipeline(device=dev, scheduler="lcm")
    tv, _ = factory.build_tiny_vae(dinit.TAESDXL, seed=1, device=dev, init_device=str(dev), with_encoder=False)
    tiny = StableDiffusionXLPipeline(vae=tv, unet=kl.unet, scheduler=kl.scheduler)
    g = torch.Generator().manual_seed(0)
    pe, te = torch.randn(1, 77, 2048, generator=g).to(bf16).to(dev), torch.randn(1, 1280, generator=g).to(bf16).to(dev)
    kw = dict(num_inference_steps=4, guidance_scale=1.0, prompt_embeds=pe, pooled_prompt_embeds=te, output_type="pt", height=1024,
              width=1024)
    res = _alternate({"tiny": lambda: tiny(generator=torch.Generator().manual_seed(1), **kw).images,
                      "kl": lambda: kl(generator=torch.Generator().manual_seed(1), **kw).images}, reps)
    res["steps"] = 4
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--latents", type=int, default=128)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    out = {"tool": "bench_tiny_vae", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "decode": decode(args.reps, args.latents), "per_launch": per_launch(args.reps)}
    if not args.no_e2e:
        out["lcm_sdxl_4_step"] = end_to_end(args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
