"""FP8 flash attention (csrc/attention_fp8.hip) against the bf16 kernel, at Wan2.1-1.3B's and FLUX.1's own shapes and on captured steps.

    python tools/bench_fp8_attention.py [--reps 5] [--inner 5] [--no-step] > profiles/fp8_attention_numbers.md

Part one, per shape (B, H, S) with heads of 128: ``ops.attention`` (bf16) against ``ops.attention_fp8`` on prepared operands (the
kernel alone) and against ``ops.attention_fp8_prepare`` + ``ops.attention_fp8`` (what a step pays), with the rel-rms of the fp8 result
against the bf16 one.  Part two: WanPipeline (480 x 832, 81 frames, 2 steps with CFG, latents out) and FluxPipeline (1024 x 1024, 4
steps + decode), seeded factory weights, captured, fp8 attention off against on -- ms per call and the PSNR of the fp8-attention output
against the bf16 output on the same seed.  Legs alternate inside one process; a figure is the median of ``--reps`` timed windows with
the range.  The operations of an attention are 4 B H S^2 D.  Needs a HIP device: there is no fallback."""
from __future__ import annotations

import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diffusers_amd import factory, ops                # noqa: E402
from bench_temporal_attention import measure          # noqa: E402

bf16 = torch.bfloat16
DEV = "cuda"
SHAPES = (("Wan2.1-1.3B self-attention", 1, 12, 32760), ("FLUX.1 joint attention", 1, 24, 4608))


def attention_legs(B: int, H: int, S: int):
    g = torch.Generator("cpu").manual_seed(S)
    C = 128 * H
    qk = torch.randn((B * S, 2 * C), generator=g).to(bf16).to(DEV)
    vt = torch.randn((C, B * S), generator=g).to(bf16).to(DEV)
    prepared = ops.attention_fp8_prepare(qk, vt, B=B, S=S, H=H)
    kw = dict(B=B, H=H, Sq=S, Skv=S, scale=128 ** -0.5)
    legs = {"bf16": lambda: ops.attention(qk, qk[:, C:], vt, D=128, Skv_alloc=S, q_row_stride=2 * C, k_row_stride=2 * C,
                                          q_batch_stride=S * 2 * C, k_batch_stride=S * 2 * C, vt_ld=B * S, vt_batch_stride=S, **kw),
            "fp8 kernel": lambda: ops.attention_fp8(*prepared, **kw),
            "prepare + fp8": lambda: ops.attention_fp8(*ops.attention_fp8_prepare(qk, vt, B=B, S=S, H=H), **kw)}
    ref, got = legs["bf16"]().float(), legs["fp8 kernel"]().float()
    return legs, float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def wan_run():
    pipe = factory.build_wan_pipeline(device=DEV)
    g = torch.Generator("cpu").manual_seed(0)
    pe, ne = torch.randn(1, 512, 4096, generator=g).to(bf16), torch.randn(1, 512, 4096, generator=g).to(bf16)

    def run(on: bool):
        (pipe.enable_fp8_attention if on else pipe.disable_fp8_attention)()
        return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, height=480, width=832, num_frames=81, num_inference_steps=2,
                    guidance_scale=5.0, generator=torch.Generator().manual_seed(1)).images
    return run


def flux_run():
    pipe = factory.build_flux_pipeline(device=DEV)
    g = torch.Generator("cpu").manual_seed(0)
    pe, pp = torch.randn(1, 512, 4096, generator=g).to(bf16), torch.randn(1, 768, generator=g).to(bf16)

    def run(on: bool):
        (pipe.enable_fp8_attention if on else pipe.disable_fp8_attention)()
        return pipe(prompt_embeds=pe, pooled_prompt_embeds=pp, height=1024, width=1024, num_inference_steps=4,
                    generator=torch.Generator().manual_seed(1)).images
    return run


def step_table(title: str, what: str, run, reps: int):
    outs = {False: run(False).float(), True: run(True).float()}            # warm-up: tuning, capture
    mse, peak = float((outs[True] - outs[False]).pow(2).mean()), float(outs[False].abs().max())
    times = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            run(on)                                                          # re-capture after the toggle, outside the window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(on)
            e1.record()
            torch.cuda.synchronize()
            times[on].append(e0.elapsed_time(e1))
    print(f"\n| {title} | ms per call |\n|---|---|")
    for on in (False, True):
        t = times[on]
        print(f"| fp8 attention {'on' if on else 'off'} | {statistics.median(t):.1f} ({min(t):.1f} .. {max(t):.1f}) |")
    print(f"\n{what} PSNR, fp8 attention on against off, same seed (seeded random weights, peak {peak:.3g}): "
          f"{10 * math.log10(peak * peak / (mse + 1e-30)):.1f} dB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print(f"# FP8 attention against bf16 ({torch.cuda.get_device_name(0)}; median (min .. max) of {a.reps} windows of {a.inner} launches)\n")
    print("| attention (B, H, S), D = 128 | bf16 us | TFLOP/s | fp8 kernel us | TFLOP/s | prepare + fp8 us | fp8 vs bf16 rel rms |")
    print("|---|---|---|---|---|---|---|")
    for name, B, H, S in SHAPES:
        legs, rr = attention_legs(B, H, S)
        res = measure(legs, a.reps, a.inner)
        tf = lambda us: 4.0 * B * H * S * S * 128 / us * 1e-6  # noqa: E731
        cell = lambda v: f"{v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})"  # noqa: E731
        print(f"| {name} ({B}, {H}, {S}) | {cell(res['bf16'])} | {tf(res['bf16'][0]):.0f} | {cell(res['fp8 kernel'])} | "
              f"{tf(res['fp8 kernel'][0]):.0f} | {cell(res['prepare + fp8'])} | {rr:.2e} |", flush=True)
    if a.no_step:
        return
    step_table("Wan2.1-1.3B 480 x 832 x 81, 2 captured steps with CFG, latents out", "Latent", wan_run(), a.reps)
    torch.cuda.empty_cache()
    step_table("FLUX.1 1024 x 1024, 4 captured steps + decode", "Image", flux_run(), a.reps)


if __name__ == "__main__":
    main()
