"""Temporal attention (csrc/attention_temporal.hip) against the route the other kernels offer for the same operation, at the four
motion-module shapes of an SD 1.5 512 x 512, 16-frame, CFG step (B = 2; HW = 4096 / 1024 / 256 / 64 with C = 320 / 640 / 1280 / 1280).

    python tools/bench_temporal_attention.py [--reps 5] [--inner 20] > profiles/temporal_attention_numbers.md

Leg one: ONE da_attention_temporal_bf16 launch on the column blocks of a frame-major [B F HW][3C] projection output.
Leg two: what the library could do before -- the projection output with heads zero-padded to a flash head size (40 -> 64, 80 -> 96),
da_permute_0213_bf16 to (B HW, F, 3C'), da_transpose_bf16 of the V block, da_attention_bf16 with B HW batches of F queries, and
da_permute_0213_bf16 back: four launches.  Both legs are checked against each other on the same values before they are timed.

Legs alternate inside one process; a timed call is ``--inner`` back-to-back launches between two device events (one launch is too
short for the event clock), a figure is the median of ``--reps`` such calls with the range, per launch.  GB/s is against the 8 F D
bytes a (pixel, head) sequence must move (Q, K, V read, O written, bf16).  Seeded data.  Needs a HIP device: there is no fallback."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diffusers_amd import ops                                   # noqa: E402
from diffusers_amd.layers import kernel_head_dim                # noqa: E402

bf16 = torch.bfloat16
DEV = "cuda"
HEADS = 8
SHAPES = ((4096, 320), (1024, 640), (256, 1280), (64, 1280))     # (HW, C)


def measure(legs: dict, reps: int, inner: int) -> dict:
    """{name: fn} -> {name: (median us, min us, max us)} per launch of fn; the legs alternate rep by rep."""
    times = {n: [] for n in legs}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for n, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def legs_of(B: int, F: int, HW: int, Cc: int):
    D = Cc // HEADS
    Dp = kernel_head_dim(D)
    Cp, rows = HEADS * Dp, B * F * HW
    vals = torch.randn((rows, 3, HEADS, D), generator=torch.Generator("cpu").manual_seed(HW)).to(bf16)
    qkv = vals.view(rows, 3 * Cc).to(DEV)
    padded = torch.zeros((rows, 3, HEADS, Dp), dtype=bf16)
    padded[..., :D] = vals
    qkv_p = padded.view(B, F, HW, 3 * Cp).to(DEV)
    out = torch.empty((rows, Cc), dtype=bf16, device=DEV)
    perm, vt = torch.empty((B, HW, F, 3 * Cp), dtype=bf16, device=DEV), torch.empty((Cp, rows), dtype=bf16, device=DEV)
    att, back = torch.empty((rows, Cp), dtype=bf16, device=DEV), torch.empty((B, F, HW, Cp), dtype=bf16, device=DEV)

    def temporal():
        return ops.temporal_attention(qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], B=B, F=F, HW=HW, H=HEADS, D=D, out=out)

    def permuted():
        ops.permute_0213(qkv_p, out=perm)
        p2 = perm.view(rows, 3 * Cp)
        ops.transpose(p2[:, 2 * Cp:], out=vt)
        ops.attention(p2[:, :Cp], p2[:, Cp:2 * Cp], vt, B=B * HW, H=HEADS, D=Dp, Sq=F, Skv=F, Skv_alloc=F, q_row_stride=3 * Cp,
                      k_row_stride=3 * Cp, q_batch_stride=F * 3 * Cp, k_batch_stride=F * 3 * Cp, vt_ld=rows, vt_batch_stride=F,
                      scale=D ** -0.5, out=att)
        return ops.permute_0213(att.view(B, HW, F, Cp), out=back)

    a = temporal().float().view(rows, HEADS, D)
    b = permuted().float().view(rows, HEADS, Dp)[..., :D]
    rr = float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    return {"temporal": temporal, "permuted": permuted}, rr, B * HW * HEADS * 8 * F * D


def pipeline_step_ms(tiny: bool, frames: int, reps: int):
    """One captured denoising step (CFG) of factory.build_animatediff_pipeline: median (min, max) ms of ``reps`` graph replays."""
    from diffusers_amd import factory
    pipe = factory.build_animatediff_pipeline(tiny=tiny)
    dim, side = pipe.unet.config.cross_attention_dim, pipe.unet.config.sample_size * pipe.vae_scale_factor
    g = torch.Generator("cpu").manual_seed(0)
    pe, npe = (torch.randn((1, 77, dim), generator=g).to(bf16) for _ in range(2))
    pipe(prompt_embeds=pe, negative_prompt_embeds=npe, num_frames=frames, height=side, width=side, num_inference_steps=2,
         generator=g, output_type="latent", use_graph=True)
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pipe._graph.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times), side


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_temporal_attention: needs a HIP device")
    if args.frames % 8:
        raise SystemExit("bench_temporal_attention: the permuted leg needs a frame count that is a multiple of 8 (Skv_alloc)")
    print(f"# Temporal attention: measured on one MI355X (the runtime reports the device as \"{torch.cuda.get_device_name(0)}\")\n")
    print(f"B = 2, F = {args.frames}, 8 heads; per launch, median of {args.reps} x {args.inner} launches (range).\n")
    print("| shape | temporal kernel (one launch) | permute, transpose, flash, permute (four launches) | four / one | legs differ by |")
    print("|---|---|---|---|---|")
    for HW, Cc in SHAPES:
        legs, rr, nbytes = legs_of(2, args.frames, HW, Cc)
        res = measure(legs, args.reps, args.inner)
        (t, tlo, thi), (p, plo, phi) = res["temporal"], res["permuted"]
        print(f"| HW {HW}, C {Cc} (D {Cc // HEADS}), {nbytes / 1e6:.1f} MB | {t:.1f} ({tlo:.1f} .. {thi:.1f}) us, {nbytes / t / 1e3:.0f} GB/s | "
              f"{p:.1f} ({plo:.1f} .. {phi:.1f}) us | {p / t:.2f}x | rel-rms {rr:.2e} |", flush=True)
    print(f"\nOne captured AnimateDiffPipeline step (CFG, {args.frames} frames, seeded weights), median of {args.reps} replays (range):\n")
    for tiny in (True, False):
        m, lo, hi, side = pipeline_step_ms(tiny, args.frames, args.reps)
        print(f"- {'tiny' if tiny else 'SD 1.5'} configuration, {side} x {side}: {m:.2f} ({lo:.2f} .. {hi:.2f}) ms", flush=True)
