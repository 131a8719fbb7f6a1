"""Numbers for EulerAncestralDiscreteScheduler (recorded in profiles/, not gated anywhere).

  python tools/bench_euler_ancestral.py --kernels    the fused Euler-ancestral step next to the Euler step at SDXL's latent size
                                                     (1 x 4 x 128 x 128 bf16, CFG, epsilon); for kernel times run it as the program of
                                                     `timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -- python ...`
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from diffusers_amd import factory  # noqa: E402
from diffusers_amd.schedulers import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler  # noqa: E402

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16


def kernels(iters: int):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 4, 128, 128, generator=g).to(bf16).to(DEV)
    eps = torch.randn(2, 4, 128, 128, generator=g).to(bf16).to(DEV)
    anc = EulerAncestralDiscreteScheduler(**factory.SDXL_EULER_A_SCHEDULER)
    anc.set_timesteps(50, device=DEV)
    noise = torch.randn(50, 1, 4, 128, 128, generator=g).to(bf16).to(DEV)
    eul = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    eul.set_timesteps(50, device=DEV)
    for _ in range(iters):
        anc.reset(0)
        xa = x.clone()
        anc.step_cfg(eps, xa, 5.0, out=xa, noise_table=noise)
        anc.step_cfg(eps, xa, 5.0, out=xa, noise_table=noise)
        eul.reset(0)
        xe = x.clone()
        eul.step_cfg(eps, xe, 5.0, out=xe)
        eul.step_cfg(eps, xe, 5.0, out=xe)
    torch.cuda.synchronize()
    print(json.dumps({"leg": "kernels", "elements": x.numel(), "launches_each": 2 * iters}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if a.kernels:
        kernels(a.iters)
