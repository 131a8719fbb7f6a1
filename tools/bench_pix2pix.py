"""Timing of the InstructPix2Pix path, all legs in one process on one GPU, each next to the composition of existing ops it replaces:

  conv_in   ops.conv_in_pix2pix(rep=3) at 64 x 64 x 320 (SD1.5, 512^2) and 128 x 128 x 320 (SDXL, 1024^2) against
            ops.euler_scale_model_input(rep=3) + torch.cat with [img, img, 0] + ops.conv_thin_in on the 8-channel tensor
  combine   ops.cfg_combine3 against the reference's five torch ops, at the two latent sizes
  step      one denoising step of the SD1.5-size pipeline at 512^2 (8-channel U-Net, Euler, guidance 7.5 / 1.5, HIP-graph replay and
            eager) against the same step driven with the concatenating path: scale_model_input(rep=3), torch.cat, the ordinary
            conv_in, the five-op combine, the step without CFG

Legs alternate inside every repetition and the median of ``--reps`` is reported with its min / max; kernel legs time ``--iters``
back-to-back launches between two device events, step legs a whole latent-output call divided by the step count.  Outputs are
compared first: the two paths must agree to the bit.  Seeded random weights: timings only.  Prints one JSON line.

    python tools/bench_pix2pix.py [--steps 20] [--reps 5] [--iters 200]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _events_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _alternate(legs, reps, measure):
    """{name: (median, min, max)} with the legs interleaved inside every repetition."""
    for fn in legs.values():                                # warm-up: every shape, every code object
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(measure(fn))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tiny", action="store_true", help="tiny models and sizes: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    from diffusers_amd import factory, ops
    from diffusers_amd.pipelines import StableDiffusionInstructPix2PixPipeline
    from diffusers_amd.schedulers import EulerDiscreteScheduler
    if not torch.cuda.is_available():
        raise RuntimeError("bench_pix2pix needs a HIP device: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    bf16 = torch.bfloat16
    g = torch.Generator().manual_seed(0)
    res = {}

    pipe = factory.build_sd15_pipeline(device=dev, tiny=args.tiny, pix2pix=True)
    pipe.scheduler = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    sch = pipe.scheduler
    sch.set_timesteps(args.steps, device=dev)
    step = torch.full((), 3, dtype=torch.int32, device=dev)
    w8, b8 = pipe.unet.conv_in_w, pipe.unet.conv_in_b
    cout = w8.shape[0]

    # ---- the kernels alone ---------------------------------------------------------------------------------------------------
    for hw in ((16,) if args.tiny else (64, 128)):
        lat, img = (torch.randn(1, 4, hw, hw, generator=g).to(bf16).to(dev) for _ in range(2))
        zero = torch.zeros_like(img)

        def fused_conv():
            return ops.conv_in_pix2pix(lat, img, w8, b8, table=sch.device_table, step_idx=step, rep=3)

        def composed_conv():
            xs = ops.euler_scale_model_input(lat, sch.device_table, step, rep=3)
            return ops.conv_thin_in(torch.cat([xs, torch.cat([img, img, zero])], dim=1), w8, b8, ksize=3, in_nchw=True)
        res[f"conv_in_{hw}x{hw}x{cout}_equal"] = bool(torch.equal(fused_conv(), composed_conv()))
        t = _alternate({"fused": fused_conv, "composed": composed_conv}, args.reps, lambda fn: _events_us(fn, args.iters))
        for k, (med, lo, hi) in t.items():
            res[f"conv_in_{hw}x{hw}x{cout}_{k}_us"] = round(med, 2)
            res[f"conv_in_{hw}x{hw}x{cout}_{k}_us_min_max"] = [round(lo, 2), round(hi, 2)]

        eps = torch.randn(3, 4, hw, hw, generator=g).to(bf16).to(dev)

        def fused_combine():
            return ops.cfg_combine3(eps, 7.5, 1.5)

        def torch_combine():
            t_, i_, u_ = eps.chunk(3)
            return u_ + 7.5 * (t_ - i_) + 1.5 * (i_ - u_)
        res[f"combine_{hw}x{hw}_equal"] = bool(torch.equal(fused_combine(), torch_combine()))
        t = _alternate({"fused": fused_combine, "torch_5_ops": torch_combine}, args.reps, lambda fn: _events_us(fn, args.iters))
        for k, (med, lo, hi) in t.items():
            res[f"combine_{hw}x{hw}_{k}_us"] = round(med, 2)
            res[f"combine_{hw}x{hw}_{k}_us_min_max"] = [round(lo, 2), round(hi, 2)]

    # ---- one step of the pipeline --------------------------------------------------------------------------------------------
    class Concatenating(StableDiffusionInstructPix2PixPipeline):
        """The same step with the ops the engine had before: scale x 3, torch.cat, the ordinary 8-channel conv_in, five torch ops."""

        def _step(self, latents, cond, guidance_scale, do_cfg):
            s = self.scheduler
            img = self._pix2pix["image_latents"]
            rep = 3 if do_cfg else 1
            xs = s.scale_model_input(latents, s.timesteps[0], rep=rep)
            blocks = [img, img, torch.zeros_like(img)][:rep]
            xin = torch.cat([xs, torch.cat(blocks)], dim=1)
            eps = self.unet(xin, None, None, conditioning=cond, sampler_table=s.device_table, step_idx=s.device_step, return_dict=False)[0]
            if do_cfg:
                t_, i_, u_ = eps.chunk(3)
                eps = u_ + guidance_scale * (t_ - i_) + self._image_guidance_scale * (i_ - u_)
            s.step_cfg(eps, latents, guidance_scale, out=latents, cfg=False, **self._step_noise_kw())
            return latents
    cat_pipe = Concatenating(vae=pipe.vae, unet=pipe.unet, scheduler=pipe.scheduler)
    px = 64 if args.tiny else 512
    seq, dim = (7, 64) if args.tiny else (77, 768)
    pe = torch.randn(1, seq, dim, generator=g).to(bf16).to(dev)
    image = torch.rand(1, 3, px, px, generator=g)
    kw = dict(image=image, num_inference_steps=args.steps, guidance_scale=7.5, image_guidance_scale=1.5, prompt_embeds=pe,
              negative_prompt_embeds=pe, output_type="latent")

    def leg(p, use_graph):
        return lambda: p(generator=torch.Generator().manual_seed(1), use_graph=use_graph, **kw).images
    legs = {"fused_graph": leg(pipe, True), "concatenating_graph": leg(cat_pipe, True), "fused_eager": leg(pipe, False),
            "concatenating_eager": leg(cat_pipe, False)}
    outs = {k: fn().clone() for k, fn in legs.items()}
    res["step_paths_equal"] = bool(all(torch.equal(outs["fused_graph"], o) for o in outs.values()))
    t = _alternate(legs, args.reps, _timed_ms)
    for k, (med, lo, hi) in t.items():
        res[f"step_{px}px_{k}_ms_per_step"] = round(med / args.steps, 4)
        res[f"step_{px}px_{k}_ms_per_step_min_max"] = [round(lo / args.steps, 4), round(hi / args.steps, 4)]
    print(json.dumps({"tool": "bench_pix2pix", "steps": args.steps, "reps": args.reps, "iters": args.iters, "tiny": bool(args.tiny),
                      "device": torch.cuda.get_device_name(0), **res}))


if __name__ == "__main__":
    main()
