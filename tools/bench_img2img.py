"""Timing of the encoder side: AutoencoderKL.encode next to decode at 512 x 512 and 1024 x 1024 (SDXL VAE), and a full SDXL
img2img call at 1024 x 1024 with strength 0.3 / 0.6 (30 scheduled steps, CFG 5.0, HIP-graph replay).  Seeded random weights, so
the numbers are timings only.  Prints one JSON line.

    python tools/bench_img2img.py [--steps 30] [--reps 5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from diffusers_amd import factory
    dev = torch.device("cuda", 0)
    bf16 = torch.bfloat16
    pipe = factory.build_sdxl_pipeline(device=dev, img2img=True)
    vae = pipe.vae
    res = {}
    g = torch.Generator().manual_seed(0)
    for hw in (512, 1024):
        img = torch.rand(1, 3, hw, hw, generator=g).to(dev)
        lat = torch.randn(1, 4, hw // 8, hw // 8, generator=g).to(bf16).to(dev)
        res[f"encode_ms_{hw}"] = _ms(lambda: vae.encode_image(img, nchw=True, normalize=True).latents(None, scale=0.13025), args.reps)
        res[f"decode_ms_{hw}"] = _ms(lambda: vae.decode(lat, return_dict=False, latents_div=0.13025, postprocess="pt"), args.reps)
    pe = torch.randn(1, 77, 2048, generator=g).to(bf16).to(dev)
    te = torch.randn(1, 1280, generator=g).to(bf16).to(dev)
    img = torch.rand(1, 3, 1024, 1024, generator=g)
    for strength in (0.3, 0.6):
        def call():
            return pipe(image=img, strength=strength, num_inference_steps=args.steps, guidance_scale=5.0, prompt_embeds=pe,
                        negative_prompt_embeds=pe, pooled_prompt_embeds=te, negative_pooled_prompt_embeds=te,
                        generator=torch.Generator().manual_seed(1), output_type="pt").images
        res[f"img2img_1024_strength{strength}_ms"] = _ms(call, max(2, args.reps // 2))
        res[f"img2img_1024_strength{strength}_unet_steps"] = min(int(args.steps * strength), args.steps)
    print(json.dumps({"tool": "bench_img2img", "steps": args.steps, **{k: round(v, 3) if isinstance(v, float) else v
                                                                        for k, v in res.items()}}))


if __name__ == "__main__":
    main()
