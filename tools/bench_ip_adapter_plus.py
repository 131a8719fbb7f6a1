"""IP-Adapter Plus: the Resampler attention launch (csrc/attention_resampler.hip) against the route it replaces, the whole
ip_adapter.Resampler call, and one captured SDXL step with a plus adapter next to one with a base adapter.

    python tools/bench_ip_adapter_plus.py [--reps 5] [--inner 20] > profiles/ip_adapter_plus_numbers.md

Shapes: the two published Resamplers (SD 1.5 plus: width 768, 12 heads; SDXL plus ViT-H: width 1280, 20 heads), 16 latents over
257 image tokens and the latents themselves, B = 1 and 2 (one image; with and without the CFG negative).  Leg one: ONE
da_attention_resampler_bf16 launch on the column halves of the two stacked to_k | to_v outputs.  Leg two, what the flash kernel needs:
a torch.cat of both sources and the zero rows up to Skv_alloc = 288, a V transpose, then da_attention_bf16 -- three launches.  Both
legs are checked against each other before they are timed.  Legs alternate inside one process; a timed call is ``--inner`` back-to-back
launches between two device events, a figure is the median of ``--reps`` such calls with the range, per launch.  Issuing a launch from
Python costs more than these kernels run, so the new launch is ALSO timed as ``--inner`` launches captured into one HIP graph and
replayed: that column is the kernel's own time.  Seeded data.  Needs a HIP device: there is no fallback."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diffusers_amd import factory, init as dinit, ip_adapter, ops    # noqa: E402
from bench_ip_attention import captured_us                            # noqa: E402
from bench_temporal_attention import measure                          # noqa: E402

bf16 = torch.bfloat16
DEV = "cuda"
SIZES = (("plus sd15", dinit.SD15_UNET, 768), ("plus sdxl vit-h", dinit.SDXL_UNET, 1280))     # (checkpoint, U-Net config, width)
NQ, S0, EMBED = 16, 257, 1280


def legs_of(B: int, dim: int):
    H, S, sa = dim // 64, S0 + NQ, (S0 + NQ + 15) // 16 * 16
    r = lambda *s: torch.randn(s, generator=torch.Generator("cpu").manual_seed(dim + B + s[0])).to(bf16).to(DEV)  # noqa: E731
    qkv1, kv0 = r(B * NQ, 3 * dim), r(B * S0, 2 * dim)
    q, k1, v1 = qkv1[:, :dim], qkv1[:, dim:2 * dim], qkv1[:, 2 * dim:]
    out, tmp = (torch.empty((B * NQ, dim), dtype=bf16, device=DEV) for _ in range(2))
    zeros = torch.zeros((B, sa - S, 2 * dim), dtype=bf16, device=DEV)

    def new():
        return ops.resampler_attention(q, kv0[:, :dim], kv0[:, dim:], k1, v1, B=B, H=H, Nq=NQ, S0=S0, S0_alloc=S0, S1=NQ, S1_alloc=NQ,
                                       scale=0.125, out=out)

    def existing():
        kv = torch.cat([kv0.view(B, S0, 2 * dim), qkv1.view(B, NQ, 3 * dim)[..., dim:], zeros], 1).view(B * sa, 2 * dim)
        vt = kv[:, dim:].t().contiguous()
        return ops.attention(q, kv[:, :dim], vt, B=B, H=H, D=64, Sq=NQ, Skv=S, Skv_alloc=sa, q_row_stride=3 * dim, k_row_stride=2 * dim,
                             q_batch_stride=NQ * 3 * dim, k_batch_stride=sa * 2 * dim, vt_ld=B * sa, vt_batch_stride=sa, scale=0.125, out=tmp)
    a, b = new().float().clone(), existing().float().clone()
    return {"new": new, "existing": existing}, float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def sdxl_step_ms(plus: bool, reps: int):
    """One captured SDXL denoising step (CFG, 1024 x 1024, seeded weights): median (min, max) ms of ``reps`` graph replays."""
    pipe = factory.build_sdxl_pipeline(ip_adapter=["plus"] if plus else True)
    g = torch.Generator("cpu").manual_seed(0)
    r = lambda *s: torch.randn(s, generator=g).to(bf16)  # noqa: E731
    embeds = [r(2, 1, S0, EMBED) if plus else r(2, 1, 1024)]
    pipe(prompt_embeds=r(1, 77, 2048), negative_prompt_embeds=r(1, 77, 2048), pooled_prompt_embeds=r(1, 1280),
         negative_pooled_prompt_embeds=r(1, 1280), num_inference_steps=2, generator=g, output_type="latent", use_graph=True,
         ip_adapter_image_embeds=embeds)
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pipe._graph.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ip_adapter_plus: needs a HIP device")
    fmt = lambda t: f"{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f}) us"  # noqa: E731
    print("# IP-Adapter Plus (Resampler): measured on one MI355X\n")
    print(f"16 latents over 257 image tokens + the latents, heads of 64; per launch / call, median of {args.reps} x {args.inner} (range).\n")
    print("| checkpoint | B | workgroups | resampler kernel, captured graph | resampler kernel, launched from Python | cat + V transpose + "
          "flash kernel (three launches from Python) | three / one | legs differ by |")
    print("|---|---|---|---|---|---|---|---|")
    for name, _, dim in SIZES:
        for B in (1, 2):
            legs, rr = legs_of(B, dim)
            res = measure(legs, args.reps, args.inner)
            c = captured_us(legs["new"], args.reps, args.inner)
            print(f"| {name} | {B} | {B * dim // 64} | {fmt(c)} | {fmt(res['new'])} | {fmt(res['existing'])} | "
                  f"{res['existing'][0] / res['new'][0]:.2f}x | rel-rms {rr:.2e} |", flush=True)
    print("\nThe whole `ip_adapter.Resampler` call (4 layers, every launch issued from Python):\n")
    for name, cfg, dim in SIZES:
        sd = factory.build_ip_adapter_state_dict(cfg, plus=True, num_tokens=NQ, image_embed_dim=EMBED, dim=dim)["image_proj"]
        proj = ip_adapter.Resampler(sd, cfg["cross_attention_dim"], DEV)
        for B in (1, 2):
            x = torch.randn((B, 1, S0, EMBED), generator=torch.Generator("cpu").manual_seed(B)).to(bf16).to(DEV)
            t = measure({"call": lambda: proj(x)}, args.reps, 4)["call"]
            print(f"- {name}, B = {B}: {t[0] / 1e3:.2f} ({t[1] / 1e3:.2f} .. {t[2] / 1e3:.2f}) ms", flush=True)
    print(f"\nOne captured StableDiffusionXLPipeline step (CFG, 1024 x 1024, seeded weights), median of {args.reps} replays (range):\n")
    for plus in (False, True):
        m, lo, hi = sdxl_step_ms(plus, args.reps)
        print(f"- {'one plus adapter, 16 image tokens' if plus else 'one base adapter, 4 image tokens'}, scale 1.0: "
              f"{m:.2f} ({lo:.2f} .. {hi:.2f}) ms", flush=True)
