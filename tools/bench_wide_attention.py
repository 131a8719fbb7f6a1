"""Wide-head flash attention (csrc/attention_wide.hip) against the three-launch path it replaces at the VAE mid blocks (fp32 scores
GEMM -> row softmax -> P.V GEMM in blocks of 4096 query rows; the Wan block: a per-frame loop of four launches).

    python tools/bench_wide_attention.py [--reps 5] [--skip-models] > profiles/wide_attention_numbers.md

Legs alternate inside one process; every figure is the median of ``--reps`` timed calls (device events around one call after a warm
call of each leg) with the range, and the peak of ``torch.cuda.max_memory_allocated`` above the level at the call's start.  Seeded
random data.  Needs a HIP device: there is no fallback."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diffusers_amd import factory, init as dinit, ops   # noqa: E402

bf16 = torch.bfloat16
DEV = "cuda"


def measure(legs: dict, reps: int) -> dict:
    """{name: fn} -> {name: (median ms, min ms, max ms, peak MiB above the start)}; the legs alternate rep by rep."""
    times, peak = {n: [] for n in legs}, {}
    for n, fn in legs.items():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for n, fn in legs.items():
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1))
            peak[n] = max(peak.get(n, 0), torch.cuda.max_memory_allocated() - base)
    return {n: (statistics.median(t), min(t), max(t), peak[n] / 2 ** 20) for n, t in times.items()}


def row(what: str, res: dict) -> None:
    cells = " | ".join(f"{m:.3f} ({lo:.3f} .. {hi:.3f}) ms, {mib:.0f} MiB" for m, lo, hi, mib in res.values())
    first, second = (v[0] for v in list(res.values())[:2])
    print(f"| {what} | {cells} | {second / first:.2f}x |", flush=True)


def three_launch(qk, vt, B, S, D, scale, qblk=4096):
    """VaeAttention's GEMM route on the same operands (per batch, blocks of ``qblk`` query rows)."""
    o = torch.empty((B * S, D), device=DEV, dtype=bf16)
    nb = min(qblk, S)
    scores = torch.empty((nb, S), device=DEV, dtype=torch.float32)
    probs = torch.empty((nb, S), device=DEV, dtype=bf16)
    for b in range(B):
        k = qk[b * S:(b + 1) * S, D:]
        for q0 in range(0, S, nb):
            n = min(nb, S - q0)
            ops.linear(qk[b * S + q0:b * S + q0 + n, :D], k, alpha=scale, out_f32=True, out=scores[:n])
            ops.softmax_rows(scores[:n], out=probs[:n])
            ops.linear(probs[:n], vt[:, b * S:(b + 1) * S], out=o[b * S + q0:b * S + q0 + n])
    return o


def kernel_rows(reps: int) -> None:
    print("| shape | flash kernel (one launch) | three-launch path | path / flash |\n|---|---|---|---|")
    for D, S, B in ((512, 4096, 1), (512, 8192, 1), (512, 16384, 1), (512, 24576, 1), (512, 32768, 1), (512, 65536, 1), (512, 4096, 4)):
        g = torch.Generator("cpu").manual_seed(S)
        qk = torch.randn((B * S, 2 * D), generator=g, dtype=bf16).to(DEV)
        vt = torch.randn((D, B * S), generator=g, dtype=bf16).to(DEV)
        scale = D ** -0.5
        flash = lambda: ops.attention(qk, qk[:, D:], vt, B=B, H=1, D=D, Sq=S, Skv=S, Skv_alloc=S, q_row_stride=2 * D,   # noqa: E731
                                      k_row_stride=2 * D, q_batch_stride=S * 2 * D, k_batch_stride=S * 2 * D, vt_ld=B * S,
                                      vt_batch_stride=S, scale=scale)
        gemm = lambda: three_launch(qk, vt, B, S, D, scale)                                # noqa: E731
        res = measure({"flash": flash, "gemm": gemm}, reps)
        a, b = flash().float(), gemm().float()
        rr = float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
        row(f"D {D}, S {S}, B {B} (routes differ by rel-rms {rr:.2e})", res)
        del qk, vt, a, b
        torch.cuda.empty_cache()


def model_rows(reps: int) -> None:
    print("\n| decode | default route (flash) | force_gemm_path | gemm / flash |\n|---|---|---|---|")
    vae, _ = factory.build_vae(dinit.SDXL_VAE, seed=1, device=DEV, init_device=DEV)
    for side in (128, 256):
        z = torch.randn((1, 4, side, side), generator=torch.Generator("cpu").manual_seed(side)).to(bf16).to(DEV)

        def leg(force):
            def run():
                vae.mid_attn.force_gemm_path = force
                return vae.decode(z).sample
            return run
        row(f"AutoencoderKL.decode, {side} x {side} latents", measure({"flash": leg(False), "gemm": leg(True)}, reps))
    vae.mid_attn.force_gemm_path = False
    del vae
    torch.cuda.empty_cache()
    wan, _ = factory.build_wan_vae(dinit.WAN_VAE, device=DEV, init_device=DEV)
    z = torch.randn((1, 16, 21, 60, 104), generator=torch.Generator("cpu").manual_seed(3)).to(bf16).to(DEV)

    def wleg(force):
        def run():
            wan.mid_attn.force_gemm_path = force
            return wan.decode(z).sample
        return run
    row("AutoencoderKLWan.decode, 21 x 60 x 104 latents", measure({"flash": wleg(False), "gemm": wleg(True)}, reps))
    # the mid block's attention alone (D 384, S 6240, B 21): norm, projections and ONE flash launch against the 84-launch frame loop
    x = torch.randn((21, 60, 104, 384), generator=torch.Generator("cpu").manual_seed(4)).to(bf16).to(DEV)

    def bleg(force):
        def run():
            wan.mid_attn.force_gemm_path = force
            return wan.mid_attn(x)
        return run
    row("Wan AttentionBlock, D 384, S 6240, B 21", measure({"flash": bleg(False), "gemm": bleg(True)}, reps))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-models", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide_attention: needs a HIP device")
    print(f"# Wide-head flash attention: measured on {torch.cuda.get_device_name(0)}\n")
    kernel_rows(args.reps)
    if not args.skip_models:
        model_rows(args.reps)
