"""FP8 linears (csrc/gemm_fp8.hip) against the bf16 path, at FLUX.1's own shapes and on one captured FLUX step.

    python tools/bench_fp8_linear.py [--reps 5] [--inner 10] [--no-step] > profiles/fp8_linear_numbers.md

Part one, per linear of a FLUX block at 1024 x 1024 (M = 4608 joint tokens): ``ops.linear`` (bf16, the tuned table's choice) against
``ops.linear_fp8`` on pre-quantised operands (the kernel alone) and against ``ops.quantize_rows_fp8`` + ``ops.linear_fp8`` (what a
step pays: the activation is quantised every time, the weight once).  Part two: the FluxPipeline at 1024 x 1024, seeded weights, 4 steps,
captured, fp8 off against on -- ms per call and the PSNR of the fp8 image against the bf16 image on the same seed.  Legs alternate
inside one process; a figure is the median of ``--reps`` timed windows with the range.  The operations of a linear are 2 M N K.
Needs a HIP device: there is no fallback."""
from __future__ import annotations

import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diffusers_amd import _lib as L, factory, ops    # noqa: E402
from bench_temporal_attention import measure          # noqa: E402

bf16 = torch.bfloat16
DEV = "cuda"
M, C = 4608, 3072
SHAPES = (("q|k (N 6144, K 3072)", M, 2 * C, C, 0), ("v^T swapped (M 3072, N 4608, K 3072)", C, M, C, 0),
          ("to_out (N 3072, K 3072)", M, C, C, 0), ("ff.0 / proj_mlp + gelu (N 12288, K 3072)", M, 4 * C, C, L.ACT_GELU_TANH),
          ("ff.2 (N 3072, K 12288)", M, C, 4 * C, 0), ("single proj_out (N 3072, K 15360)", M, C, 5 * C, 0))


def linear_legs(m: int, n: int, k: int, act: int):
    g = torch.Generator("cpu").manual_seed(n + k)
    x, w = torch.randn((m, k), generator=g).to(bf16).to(DEV), (torch.randn((n, k), generator=g) * k ** -0.5).to(bf16).to(DEV)
    b = torch.randn((n,), generator=g).to(bf16).to(DEV)
    xq, wq = ops.quantize_rows_fp8(x), ops.quantize_rows_fp8(w)
    legs = {"bf16": lambda: ops.linear(x, w, b, act=act), "fp8 kernel": lambda: ops.linear_fp8(*xq, *wq, b, act=act),
            "quantise + fp8": lambda: ops.linear_fp8(*ops.quantize_rows_fp8(x), *wq, b, act=act)}
    ref, got = legs["bf16"]().float(), legs["fp8 kernel"]().float()
    return legs, float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def step_legs():
    pipe = factory.build_flux_pipeline(device=DEV)
    g = torch.Generator("cpu").manual_seed(0)
    pe, pp = torch.randn(1, 512, 4096, generator=g).to(bf16), torch.randn(1, 768, generator=g).to(bf16)

    def run(fp8: bool):
        (pipe.enable_fp8_linears if fp8 else pipe.disable_fp8_linears)()
        return pipe(prompt_embeds=pe, pooled_prompt_embeds=pp, height=1024, width=1024, num_inference_steps=4,
                    generator=torch.Generator().manual_seed(1)).images
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print(f"# FP8 linears against bf16 ({torch.cuda.get_device_name(0)}; median (min .. max) of {a.reps} windows of {a.inner} launches)\n")
    print("| linear | bf16 us | TFLOP/s | fp8 kernel us | TFLOP/s | quantise + fp8 us | fp8 vs bf16 rel rms |")
    print("|---|---|---|---|---|---|---|")
    for name, m, n, k, act in SHAPES:
        legs, rr = linear_legs(m, n, k, act)
        res = measure(legs, a.reps, a.inner)
        tf = lambda us: 2.0 * m * n * k / us * 1e-6  # noqa: E731
        cell = lambda v: f"{v[0]:.1f} ({v[1]:.1f} .. {v[2]:.1f})"  # noqa: E731
        print(f"| {name} | {cell(res['bf16'])} | {tf(res['bf16'][0]):.0f} | {cell(res['fp8 kernel'])} | {tf(res['fp8 kernel'][0]):.0f} | "
              f"{cell(res['quantise + fp8'])} | {rr:.2e} |", flush=True)
    if a.no_step:
        return
    run = step_legs()
    imgs = {False: run(False).float(), True: run(True).float()}          # warm-up: tuning, capture
    mse = float((imgs[True] - imgs[False]).pow(2).mean())
    times = {False: [], True: []}
    for _ in range(a.reps):
        for fp8 in (False, True):
            run(fp8)                                                         # re-capture after the toggle, outside the window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(fp8)
            e1.record()
            torch.cuda.synchronize()
            times[fp8].append(e0.elapsed_time(e1))
    print("\n| FLUX.1 1024 x 1024, 4 captured steps + decode | ms per call |\n|---|---|")
    for fp8 in (False, True):
        t = times[fp8]
        print(f"| fp8 linears {'on' if fp8 else 'off'} | {statistics.median(t):.1f} ({min(t):.1f} .. {max(t):.1f}) |")
    print(f"\nImage PSNR, fp8 on against off, same seed (seeded random weights, images in [0, 1]): {-10 * math.log10(mse + 1e-30):.1f} dB")


if __name__ == "__main__":
    main()
