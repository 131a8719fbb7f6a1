"""Timing of FreeU (seeded random tensors and weights: timings only), every comparison with its legs in one process on one GPU,
alternating, median of the repetitions with min .. max:

  (a) kernel   ops.freeu on SDXL's six (hidden, skip) shapes at CFG batch 2 -- the library's own path, and the two-launch path where
               the library chose the LDS-resident one -- against the reference's route with torch ops on the GPU (NCHW, fp32:
               fftn, fftshift, ones-mask, multiply, ifftshift, ifftn, .real, the casts and the half-channel slice-assign).  One
               timed sample is `--inner` back-to-back calls between two synchronisations, divided by their number.
  (b) step     one SDXL 1024 x 1024 denoising step (captured HIP graph, CFG batch 2) with FreeU on against off: two pipelines of
               the same weights, one with enable_freeu(0.9, 0.2, 1.3, 1.4); a sample is a `--steps`-step call over its step count.

Prints one JSON line; --markdown PATH also writes the tables.

    python tools/bench_freeu.py [--reps 5] [--inner 50] [--steps 10] [--skip-step] [--markdown profiles/freeu_numbers.md]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
bf16 = torch.bfloat16
# (H = W, hidden channels, skip channels): up block 0's three resnets, up block 1's three
SDXL_SHAPES = [(32, 1280, 1280), (32, 1280, 1280), (32, 1280, 640), (64, 1280, 640), (64, 640, 640), (64, 640, 320)]


def _timed(fn, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def _alternate(legs: dict, reps: int, inner: int = 1, warm: int = 2) -> dict:
    for fn in legs.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(_timed(fn, inner))
    return {k: _stats(v) for k, v in times.items()}


def torch_route(hidden_nchw, skip_nchw, s, b):
    """apply_freeu / fourier_filter as the reference runs them."""
    half = hidden_nchw.shape[1] // 2
    hidden_nchw[:, :half] = hidden_nchw[:, :half] * b
    x = skip_nchw.to(torch.float32)
    B, C, H, W = x.shape
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), device=x.device)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    f = torch.fft.ifftshift(f * mask, dim=(-2, -1))
    return torch.fft.ifftn(f, dim=(-2, -1)).real.to(skip_nchw.dtype)


def kernel_legs(reps: int, inner: int) -> list:
    from diffusers_amd import _lib as L, ops
    lib, dev, rows = L.load(), torch.device("cuda", 0), []
    g = torch.Generator().manual_seed(0)
    for i, (hw, cx, cs) in enumerate(SDXL_SHAPES):
        s, b = (0.9, 1.3) if i < 3 else (0.2, 1.4)
        hidden = torch.randn(2, hw, hw, cx, generator=g).to(bf16).to(dev)
        skip = torch.randn(2, hw, hw, cs, generator=g).to(bf16).to(dev)
        hn, sn = hidden.permute(0, 3, 1, 2).contiguous(), skip.permute(0, 3, 1, 2).contiguous()
        resident = lib.da_freeu_workspace_bytes(2, hw, hw, cs, L.FREEU_AUTO) == 0
        legs = {"kernel": lambda: ops.freeu(hidden, skip, s=s, b=b), "torch_route": lambda: torch_route(hn, sn, s, b)}
        if resident:
            legs["kernel_two_launch"] = lambda: ops.freeu(hidden, skip, s=s, b=b, path=L.FREEU_TWO_LAUNCH)
        res = _alternate(legs, reps, inner)
        res.update(shape=[2, hw, hw], hidden=cx, skip=cs, path="resident" if resident else "two-launch",
                   torch_over_kernel=round(res["torch_route"]["median_ms"] / res["kernel"]["median_ms"], 1))
        rows.append(res)
    return rows


def step_legs(reps: int, steps: int) -> dict:
    from diffusers_amd import factory
    dev = torch.device("cuda", 0)
    pipes = {k: factory.build_sdxl_pipeline(device=dev, seed=0) for k in ("off", "on")}
    pipes["on"].enable_freeu(s1=0.9, s2=0.2, b1=1.3, b2=1.4)
    g = torch.Generator().manual_seed(1)
    kw = dict(prompt_embeds=torch.randn(1, 77, 2048, generator=g).to(bf16).to(dev), negative_prompt_embeds=torch.randn(1, 77, 2048, generator=g).to(bf16).to(dev),
              pooled_prompt_embeds=torch.randn(1, 1280, generator=g).to(bf16).to(dev), negative_pooled_prompt_embeds=torch.randn(1, 1280, generator=g).to(bf16).to(dev),
              guidance_scale=5.0, height=1024, width=1024, num_inference_steps=steps, output_type="latent", use_graph=True)
    lat = torch.randn(1, 4, 128, 128, generator=g).to(bf16).to(dev)
    res = _alternate({k: (lambda p=p: p(latents=lat.clone(), **kw)) for k, p in pipes.items()}, reps, warm=1)
    out = {k: {n: round(v / steps, 3) for n, v in r.items()} for k, r in res.items()}
    out["freeu_ms_per_step"] = round(out["on"]["median_ms"] - out["off"]["median_ms"], 3)
    out["steps_per_call"] = steps
    return out


def markdown(out: dict) -> str:
    lines = ["# FreeU: measurements", "", f"`tools/bench_freeu.py`, {out['device']}, legs alternating in one process, median of {out['reps']} "
             f"(min .. max); a kernel sample is {out['inner']} back-to-back calls over their number (launch overhead of the host included).", "",
             "## (a) `ops.freeu` against the reference's torch route, SDXL's six shapes, CFG batch 2", "",
             "| plane | hidden ch | skip ch | path | kernel ms | two-launch ms | torch route ms | torch / kernel |", "|---|---|---|---|---|---|---|---|"]
    fmt = lambda r: f"{r['median_ms']} ({r['min_ms']} .. {r['max_ms']})"  # noqa: E731
    for r in out["kernel"]:
        two = fmt(r["kernel_two_launch"]) if "kernel_two_launch" in r else "-"
        lines.append(f"| {r['shape'][1]} x {r['shape'][2]} | {r['hidden']} | {r['skip']} | {r['path']} | {fmt(r['kernel'])} | {two} | "
                     f"{fmt(r['torch_route'])} | {r['torch_over_kernel']} x |")
    if "step" in out:
        s = out["step"]
        lines += ["", "## (b) One SDXL 1024 x 1024 step (captured graph, CFG batch 2), ms per step", "", "| FreeU | median | min | max |", "|---|---|---|---|",
                  f"| off | {s['off']['median_ms']} | {s['off']['min_ms']} | {s['off']['max_ms']} |",
                  f"| on (0.9, 0.2, 1.3, 1.4) | {s['on']['median_ms']} | {s['on']['min_ms']} | {s['on']['max_ms']} |", "",
                  f"FreeU costs {s['freeu_ms_per_step']} ms per step (up block 0: three resident launches; up block 1: three reduce / apply pairs)."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_freeu: no HIP device (timings are taken on the GPU only)")
    out = {"tool": "bench_freeu", "reps": args.reps, "inner": args.inner, "device": torch.cuda.get_device_name(0),
           "kernel": kernel_legs(args.reps, args.inner)}
    if not args.skip_step:
        out["step"] = step_legs(args.reps, args.steps)
    if args.markdown:
        Path(args.markdown).write_text(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
