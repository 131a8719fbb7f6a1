"""Timing of SDXL inpainting at 1024 x 1024 (30 scheduled steps, CFG 7.5, strength 1.0, HIP-graph replay), per denoising step, all
legs in one process on one GPU:

  (a) img2img                                      the loop inpainting builds on
  (b) inpainting, 4-channel U-Net                  (a) + the fused mask blend (ops.inpaint_blend_), graph replay
  (c) the same loop with the blend as ops.add_noise + four torch element-wise ops and a host-side coefficient per step, eager:
      the composition of existing ops the fused kernel replaces (not graph-replayable: the coefficient is a host scalar)
  (c0) the loop of (b) eager: what (c) is compared with launch for launch
  (d) inpainting, 9-channel U-Net                  conv_in from three sources, no blend

and the two kernels in isolation next to what they replace.  Per-step times come from the latent-output call time divided by the
step count (the calls differ only in their loops); legs alternate inside every repetition and the median is reported.  Seeded random
weights: timings only.  Prints one JSON line.

    python tools/bench_inpaint.py [--steps 30] [--reps 5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _kernel_us(fn, iters=200):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from diffusers_amd import factory, ops
    from diffusers_amd.pipelines import StableDiffusionXLImg2ImgPipeline, StableDiffusionXLInpaintPipeline, _InpaintMixin
    dev = torch.device("cuda", 0)
    bf16 = torch.bfloat16
    p4 = factory.build_sdxl_pipeline(device=dev, inpaint=True, unet_in_channels=4)
    p9 = factory.build_sdxl_pipeline(device=dev, inpaint=True, unet_in_channels=9)
    i2i = StableDiffusionXLImg2ImgPipeline(vae=p4.vae, unet=p4.unet, scheduler=p4.scheduler)

    class ComposedBlend(StableDiffusionXLInpaintPipeline):
        """Leg (c): the blend written with the ops of the parent commit."""

        def _step(self, latents, cond, guidance_scale, do_cfg):
            super(_InpaintMixin, self)._step(latents, cond, guidance_scale, do_cfg)      # the img2img step, without the fused blend
            st, sch = self._inpaint, self.scheduler
            j = sch._step_index
            if j < len(sch.timesteps):
                proper = sch.add_noise(st["image_latents"], st["noise"], sch.timesteps[j:j + 1])
            else:
                proper = st["image_latents"]
            latents.copy_((1 - st["mask"]) * proper + st["mask"] * latents)
            return latents
    pc = ComposedBlend(vae=p4.vae, unet=p4.unet, scheduler=p4.scheduler)

    g = torch.Generator().manual_seed(0)
    pe = torch.randn(1, 77, 2048, generator=g).to(bf16).to(dev)
    te = torch.randn(1, 1280, generator=g).to(bf16).to(dev)
    img = torch.rand(1, 3, 1024, 1024, generator=g)
    mask = torch.zeros(1024, 1024)
    mask[256:768, 256:768] = 1.0
    kw = dict(image=img, strength=1.0, num_inference_steps=args.steps, guidance_scale=7.5, prompt_embeds=pe, negative_prompt_embeds=pe,
              pooled_prompt_embeds=te, negative_pooled_prompt_embeds=te, output_type="latent")

    def leg(pipe, use_graph, inpaint=True):
        extra = dict(mask_image=mask) if inpaint else {}
        return lambda: pipe(generator=torch.Generator().manual_seed(1), use_graph=use_graph, **extra, **kw).images
    legs = {"a_img2img_graph": leg(i2i, True, False), "b_inpaint4_fused_graph": leg(p4, True), "c_inpaint4_composed_eager": leg(pc, False),
            "c0_inpaint4_fused_eager": leg(p4, False), "d_inpaint9_graph": leg(p9, True)}
    # outputs first (and warm-up: every shape, both capture paths): fused and composed blends must agree to the bit
    outs = {k: fn().clone() for k, fn in legs.items()}
    res = {"composed_equals_fused": bool(torch.equal(outs["c_inpaint4_composed_eager"], outs["b_inpaint4_fused_graph"])),
           "fused_graph_equals_eager": bool(torch.equal(outs["c0_inpaint4_fused_eager"], outs["b_inpaint4_fused_graph"]))}
    for fn in legs.values():
        fn()
    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():                          # alternate the legs inside every repetition
            times[k].append(_timed(fn))
    for k, v in times.items():
        v.sort()
        res[f"{k}_ms_per_step"] = v[len(v) // 2] / args.steps
        res[f"{k}_ms_per_step_min_max"] = [round(v[0] / args.steps, 4), round(v[-1] / args.steps, 4)]

    # the kernels alone (SDXL 1024^2: latents 1 x 4 x 128 x 128, conv_in 9 -> 320, CFG)
    sch = p4.scheduler
    lat, x0, nz = (torch.randn(1, 4, 128, 128, generator=g).to(bf16).to(dev) for _ in range(3))
    m = (torch.rand(1, 1, 128, 128, generator=g) >= 0.5).to(bf16).to(dev)
    tab = sch.add_noise_table(bf16)
    step = torch.full((), 3, dtype=torch.int32, device=dev)
    a, b = tab[3].tolist()
    res["k1_inpaint_blend_us"] = _kernel_us(lambda: ops.inpaint_blend_(lat, x0, nz, m, tab, step))
    res["k1_composed_add_noise_plus_torch_us"] = _kernel_us(lambda: lat.copy_((1 - m) * ops.add_noise(x0, nz, a, b) + m * lat))
    w9, b9 = p9.unet.conv_in_w, p9.unet.conv_in_b
    res["k2_conv_in_inpaint_us"] = _kernel_us(lambda: ops.conv_in_inpaint(lat, m, x0, w9, b9, table=sch.device_table, step_idx=step, rep=2))

    def composed_conv_in():
        xs = ops.euler_scale_model_input(lat, sch.device_table, step, rep=2)
        cat = torch.cat([xs, torch.cat([m] * 2), torch.cat([x0] * 2)], dim=1)
        return ops.conv_thin_in(cat, w9, b9, ksize=3, in_nchw=True)
    res["k2_composed_scale_cat_conv_thin_in_us"] = _kernel_us(composed_conv_in)
    w4, b4 = p4.unet.conv_in_w, p4.unet.conv_in_b
    res["conv_in_4ch_scale_plus_conv_thin_in_us"] = _kernel_us(
        lambda: ops.conv_thin_in(ops.euler_scale_model_input(lat, sch.device_table, step, rep=2), w4, b4, ksize=3, in_nchw=True))
    print(json.dumps({"tool": "bench_inpaint", "steps": args.steps, "reps": args.reps, "device": torch.cuda.get_device_name(0),
                      **{k: round(v, 4) if isinstance(v, float) else v for k, v in res.items()}}))


if __name__ == "__main__":
    main()
