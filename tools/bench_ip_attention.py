"""The IP-Adapter image-prompt launch (csrc/attention_ip.hip) against the same operation through the existing kernels, at the
cross-attention shapes of SDXL and SD 1.5 (CFG batch 2, 1024 x 1024 / 512 x 512), N = 4 and 16 image tokens, and one captured SDXL
step with and without an adapter.

    python tools/bench_ip_attention.py [--reps 5] [--inner 20] > profiles/ip_adapter_numbers.md

Leg one: ONE da_attention_ip_bf16 launch, in place on `out`.  Leg two (D = 64 only: the masked flash kernel exists for that head size):
da_attention_bf16 on the image keys zero-padded to 16 with an additive key mask, V transposed beforehand, then a torch scaled add
onto `out` -- two launches.  Both legs are checked against each other before they are timed.  Legs alternate inside one process; a
timed call is ``--inner`` back-to-back launches between two device events, a figure is the median of ``--reps`` such calls with the
range, per launch.  Issuing a launch from Python costs more than these kernels run, so the image-prompt launch is ALSO timed as
``--inner`` launches captured into one HIP graph and replayed (no host work per launch): that column is the kernel's own time, and
its GB/s is against the 3 Sq D 2 bytes a (batch, head) must move (q read, out read and written).  Seeded data.  Needs
a HIP device: there is no fallback."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diffusers_amd import ops                                   # noqa: E402
from diffusers_amd.layers import kernel_head_dim                # noqa: E402
from bench_temporal_attention import measure                    # noqa: E402

bf16 = torch.bfloat16
DEV = "cuda"
SHAPES = (("SDXL 64 x 64", 4096, 10, 64), ("SDXL 32 x 32", 1024, 20, 64), ("SD 1.5 64 x 64", 4096, 8, 40), ("SD 1.5 32 x 32", 1024, 8, 80),
          ("SD 1.5 16 x 16", 256, 8, 160), ("SD 1.5 8 x 8", 64, 8, 160))     # (level, Sq, heads, head_dim)


def legs_of(B: int, Sq: int, H: int, d: int, N: int):
    D, sa, scale = kernel_head_dim(d), 16, 0.6
    Cc = H * D
    g = torch.Generator("cpu").manual_seed(Sq + N)
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (D - d,))], -1)  # noqa: E731
    q, out0 = (pad(torch.randn((B * Sq, H, d), generator=g)).view(B * Sq, Cc).to(bf16).to(DEV) for _ in range(2))
    kv = torch.zeros((B, sa, 2, H, D))
    kv[:, :N, :, :, :d] = torch.randn((B, N, 2, H, d), generator=g)
    kv = kv.view(B * sa, 2 * Cc).to(bf16).to(DEV)
    k, v = kv[:, :Cc], kv[:, Cc:]
    out = out0.clone()

    def accumulate():
        return ops.ip_attention_accumulate(out, q, [(k, v, N, sa, scale)], B=B, H=H, D=D, Sq=Sq, scale=d ** -0.5)
    legs = {"ip": accumulate}
    rr = None
    if D == 64:
        vt, kc = v.t().contiguous(), k.contiguous()
        bias = torch.zeros((B, 1, 1, 64), dtype=bf16, device=DEV)
        bias[..., N:] = -30000.0
        tmp = torch.empty((B * Sq, Cc), dtype=bf16, device=DEV)

        def existing():
            ops.attention(q, kc, vt, B=B, H=H, D=D, Sq=Sq, Skv=sa, Skv_alloc=sa, q_row_stride=Cc, k_row_stride=Cc, q_batch_stride=Sq * Cc,
                          k_batch_stride=sa * Cc, vt_ld=B * sa, vt_batch_stride=sa, scale=d ** -0.5, bias=bias, out=tmp)
            return out.add_(tmp, alpha=scale)
        legs["existing"] = existing
        out.copy_(out0)
        a = accumulate().float().clone()
        out.copy_(out0)
        b = existing().float().clone()
        rr = float((a - b).pow(2).mean().sqrt() / (b - out0.float()).pow(2).mean().sqrt())
    return legs, rr, B * H * 3 * Sq * D * 2


def captured_us(fn, reps: int, inner: int):
    """Per-launch time of ``fn`` with ``inner`` launches captured into one HIP graph: median (min, max) us of ``reps`` replays."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            for _ in range(inner):
                fn()
    times = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / inner)
    times = times[1:]                                  # (the first replay uploads the graph)
    return statistics.median(times), min(times), max(times)


def sdxl_step_ms(ip_adapter: bool, reps: int):
    """One captured SDXL denoising step (CFG, 1024 x 1024, seeded weights): median (min, max) ms of ``reps`` graph replays."""
    from diffusers_amd import factory
    pipe = factory.build_sdxl_pipeline(ip_adapter=ip_adapter)
    g = torch.Generator("cpu").manual_seed(0)
    r = lambda *s: torch.randn(s, generator=g).to(bf16)  # noqa: E731
    kw = {"ip_adapter_image_embeds": [r(2, 1, 1024)]} if ip_adapter else {}
    pipe(prompt_embeds=r(1, 77, 2048), negative_prompt_embeds=r(1, 77, 2048), pooled_prompt_embeds=r(1, 1280),
         negative_pooled_prompt_embeds=r(1, 1280), num_inference_steps=2, generator=g, output_type="latent", use_graph=True, **kw)
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
        raise SystemExit("bench_ip_attention: needs a HIP device")
    print("# IP-Adapter image-prompt attention: measured on one MI355X\n")
    print(f"B = 2, one adapter at scale 0.6; per launch, median of {args.reps} x {args.inner} launches (range).\n")
    print("| shape | N | image-prompt kernel, captured graph | image-prompt kernel, launched from Python | masked flash + scaled add "
          "(two launches from Python) | two / one | legs differ by |")
    print("|---|---|---|---|---|---|---|")
    for level, Sq, H, d in SHAPES:
        for N in (4, 16):
            legs, rr, nbytes = legs_of(2, Sq, H, d, N)
            res = measure(legs, args.reps, args.inner)
            t, tlo, thi = res["ip"]
            c, clo, chi = captured_us(legs["ip"], args.reps, args.inner)
            if "existing" in res:
                p, plo, phi = res["existing"]
                other, ratio, diff = f"{p:.1f} ({plo:.1f} .. {phi:.1f}) us", f"{p / t:.2f}x", f"rel-rms {rr:.2e}"
            else:
                other, ratio, diff = "- (no masked kernel at this head size)", "-", "-"
            print(f"| {level}, Sq {Sq}, {H} heads of {d}, {nbytes / 1e6:.1f} MB | {N} | {c:.1f} ({clo:.1f} .. {chi:.1f}) us, "
                  f"{nbytes / c / 1e3:.0f} GB/s | {t:.1f} ({tlo:.1f} .. {thi:.1f}) us | {other} | {ratio} | {diff} |", flush=True)
    print(f"\nOne captured StableDiffusionXLPipeline step (CFG, 1024 x 1024, seeded weights), median of {args.reps} replays (range):\n")
    for ip in (False, True):
        m, lo, hi = sdxl_step_ms(ip, args.reps)
        print(f"- {'one IP-Adapter of 4 tokens, scale 1.0' if ip else 'no adapter'}: {m:.2f} ({lo:.2f} .. {hi:.2f}) ms", flush=True)
