"""Numbers for DPMSolverMultistepScheduler (recorded in profiles/, not gated anywhere).

  python tools/bench_dpmpp.py --kernels     the fused DPM-Solver++ 2M step next to the Euler step at SDXL's latent size; for
                                              kernel times run it as the program of
                                              `timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -- python ...`
  python tools/bench_dpmpp.py --images      wall time of one SDXL 1024^2 image, 25 DPM++ 2M Karras steps next to 50 Euler steps,
                                              same process, seeded factory weights, HIP-graph replay, VAE decode included
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from diffusers_amd import factory  # noqa: E402
from diffusers_amd.schedulers import DPMSolverMultistepScheduler, EulerDiscreteScheduler  # noqa: E402

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16


def kernels(iters: int):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 4, 128, 128, generator=g).to(bf16).to(DEV)
    eps = torch.randn(2, 4, 128, 128, generator=g).to(bf16).to(DEV)
    dpm = DPMSolverMultistepScheduler(**factory.SDXL_DPM_SCHEDULER)
    dpm.set_timesteps(25, device=DEV)
    eul = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    eul.set_timesteps(50, device=DEV)
    for _ in range(iters):
        dpm.reset(0)
        xd = x.clone()
        dpm.step_cfg(eps, xd, 5.0, out=xd)        # first order (first step of the loop)
        dpm.step_cfg(eps, xd, 5.0, out=xd)        # second order
        eul.reset(0)
        xe = x.clone()
        eul.step_cfg(eps, xe, 5.0, out=xe)
        eul.step_cfg(eps, xe, 5.0, out=xe)
    torch.cuda.synchronize()
    print(json.dumps({"leg": "kernels", "elements": x.numel(), "launches_each": 2 * iters}))


def images():
    pipe = factory.build_sdxl_pipeline(device=DEV)
    g = torch.Generator().manual_seed(1)
    kw = dict(prompt_embeds=torch.randn(1, 77, 2048, generator=g).to(bf16).to(DEV),
              negative_prompt_embeds=torch.randn(1, 77, 2048, generator=g).to(bf16).to(DEV),
              pooled_prompt_embeds=torch.randn(1, 1280, generator=g).to(bf16).to(DEV),
              negative_pooled_prompt_embeds=torch.randn(1, 1280, generator=g).to(bf16).to(DEV),
              guidance_scale=5.0, output_type="pt")
    lat = torch.randn(1, 4, 128, 128, generator=g).to(bf16)
    out = {"leg": "images", "size": 1024}
    for name, sch, steps in (("euler_50", pipe.scheduler, 50),
                             ("dpmpp_2m_karras_25", DPMSolverMultistepScheduler(**factory.SDXL_DPM_SCHEDULER), 25)):
        pipe.scheduler = sch
        pipe(latents=lat.clone(), num_inference_steps=steps, **kw)        # capture + tuning
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            img = pipe(latents=lat.clone(), num_inference_steps=steps, **kw).images
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        assert torch.isfinite(img.float()).all()
        out[name + "_ms"] = [round(1e3 * t, 1) for t in times]
    out["ratio_best"] = round(min(out["euler_50_ms"]) / min(out["dpmpp_2m_karras_25_ms"]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--images", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if a.kernels:
        kernels(a.iters)
    if a.images:
        images()
