"""Numbers for HeunDiscreteScheduler / KDPM2DiscreteScheduler (recorded in profiles/second_order_numbers.md, not gated anywhere).
One MI355X, the legs of a comparison alternating in one process, the median of 5 windows per leg after a warm-up of every leg.

  python tools/bench_second_order.py --step     the fused two-phase step (a predictor and a corrector entry per iteration, CFG, bf16,
                                                 n = 4 x 128 x 128: SDXL's latents) against the same update written as torch ops on
                                                 the same tensors; host clock around a window that ends in a device synchronise
  python tools/bench_second_order.py --images   wall time of one SDXL 1024^2 image: 25 Heun steps and 25 DPM2 steps (49 model calls
                                                 each) against 49 Euler steps, seeded factory weights, HIP-graph replay, VAE decode
                                                 included
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from diffusers_amd import factory, ops  # noqa: E402
from diffusers_amd.schedulers import EulerDiscreteScheduler, HeunDiscreteScheduler, KDPM2DiscreteScheduler  # noqa: E402

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16
WINDOWS = 5


def _torch_entry(eps, x, m1, row, g):
    """One entry with torch ops, the roundings of the fused step: the reference's style of scheduler step (epsilon prediction)."""
    sigma, c_hist, dt_x, phase = row
    u, c = eps[0], eps[1]
    e = u + g * (c - u)
    s = x.float()
    x0 = s - (sigma * e.float()).to(bf16).float()
    d = (s - x0) / sigma
    if phase == 1:
        m1.copy_(s + c_hist * d)
    base = m1 if phase == 2 else s
    x.copy_((base + dt_x * d).to(bf16))


def step(iters: int):
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(1, 4, 128, 128, generator=g).to(bf16).to(DEV)
    eps = torch.randn(2, 1, 4, 128, 128, generator=g).to(bf16).to(DEV)
    sch = HeunDiscreteScheduler(**factory.SECOND_ORDER_SCHEDULER)
    sch.set_timesteps(25, device=DEV)
    table = sch.device_table
    rows = [(float(r[0]), float(r[1]), float(r[2]), int(r[6])) for r in table[2:4].cpu()]       # a predictor and its corrector
    steps = [torch.full((), j, dtype=torch.int32, device=DEV) for j in (2, 3)]
    m1 = torch.zeros(x0.shape, dtype=torch.float32, device=DEV)
    x = x0.clone()

    def fused():
        for st in steps:
            ops.second_order_step_(eps, x, m1, table, st, st, cfg=True, guidance=5.0)

    def eager():
        for row in rows:
            _torch_entry(eps, x, m1, row, 5.0)

    # the two legs compute the same thing
    fused()
    a = x.clone()
    x.copy_(x0)
    eager()
    assert float((a.float() - x.float()).abs().max()) <= 2.0 ** -7 * float(a.float().abs().max()), "the two legs disagree"
    legs = {"fused": fused, "torch_ops": eager}
    times = {k: [] for k in legs}
    for w in range(WINDOWS + 1):                      # window 0 warms both legs up
        for name, fn in legs.items():
            x.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            if w:
                times[name].append((time.perf_counter() - t0) / (2 * iters))
    out = {"leg": "step", "elements": x.numel(), "entries_per_window": 2 * iters, "windows": WINDOWS}
    for name, t in times.items():
        out[name + "_us_per_entry"] = [round(1e6 * v, 2) for v in t]
        out[name + "_median_us"] = round(1e6 * statistics.median(t), 2)
    out["ratio_of_medians"] = round(out["torch_ops_median_us"] / out["fused_median_us"], 2)
    print(json.dumps(out))


def images():
    pipe = factory.build_sdxl_pipeline(device=DEV)
    g = torch.Generator().manual_seed(1)
    kw = dict(prompt_embeds=torch.randn(1, 77, 2048, generator=g).to(bf16).to(DEV),
              negative_prompt_embeds=torch.randn(1, 77, 2048, generator=g).to(bf16).to(DEV),
              pooled_prompt_embeds=torch.randn(1, 1280, generator=g).to(bf16).to(DEV),
              negative_pooled_prompt_embeds=torch.randn(1, 1280, generator=g).to(bf16).to(DEV),
              guidance_scale=5.0, output_type="pt")
    lat = torch.randn(1, 4, 128, 128, generator=g).to(bf16)
    legs = (("euler_49", EulerDiscreteScheduler(**factory.SDXL_SCHEDULER), 49),
            ("heun_25", HeunDiscreteScheduler(**factory.SECOND_ORDER_SCHEDULER), 25),
            ("kdpm2_25", KDPM2DiscreteScheduler(**factory.SECOND_ORDER_SCHEDULER), 25))
    # one pipeline object per leg on the same U-Net and VAE: each keeps its captured step, so no timed call captures
    pipes = {name: type(pipe)(vae=pipe.vae, unet=pipe.unet, scheduler=sch) for name, sch, _ in legs}
    times = {name: [] for name, _, _ in legs}
    for w in range(WINDOWS + 1):                      # round 0: capture + tuning of every leg
        for name, sch, steps in legs:
            pipe = pipes[name]
            graph = pipe._graph
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            img = pipe(latents=lat.clone(), num_inference_steps=steps, **kw).images
            torch.cuda.synchronize()
            if w:
                times[name].append(time.perf_counter() - t0)
            assert torch.isfinite(img.float()).all() and len(sch.timesteps) == 49 and (w == 0 or pipe._graph is graph)
    out = {"leg": "images", "size": 1024, "model_calls": 49, "windows": WINDOWS}
    for name, t in times.items():
        out[name + "_ms"] = [round(1e3 * v, 1) for v in t]
        out[name + "_median_ms"] = round(1e3 * statistics.median(t), 1)
    out["heun_over_euler"] = round(out["heun_25_median_ms"] / out["euler_49_median_ms"], 4)
    out["kdpm2_over_euler"] = round(out["kdpm2_25_median_ms"] / out["euler_49_median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--images", action="store_true")
    ap.add_argument("--iters", type=int, default=5000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_second_order.py measures on a HIP device; none found")
    if a.step:
        step(a.iters)
    if a.images:
        images()
