"""GPU: the SDXL / SD1.5 img2img pipelines against an fp32 oracle loop (the restated encoder, add_noise and the oracle sampler
started at t_start, oracle.reference_math.unet_forward), HIP-graph replay against eager launches, the step count that follows
``strength``, and the base -> refiner hand-off at ``denoising_end`` / ``denoising_start``."""
import numpy as np
import pytest
import torch

from oracle import ref_runtime as RR
from oracle import reference_math as R
from oracle.samplers import DDIMOracle, EulerOracle, cfg_combine
from test_vae_encode_gpu import encoder_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16


def _embeds(seed, B, seq, dim, pooled):
    g = torch.Generator().manual_seed(seed)
    pe, npe = (torch.randn(B, seq, dim, generator=g).to(bf16) for _ in range(2))
    te, nte = (torch.randn(B, pooled, generator=g).to(bf16) for _ in range(2)) if pooled else (None, None)
    return pe, npe, te, nte


def _psnr01(a, b):
    mse = float((a.float().cpu() - b.float().cpu()).pow(2).mean())
    return 10 * np.log10(1.0 / max(mse, 1e-12))


def _count_steps(pipe, **kw):
    n = [0]

    def cb(p, i, t, d):
        n[0] += 1
        return {}
    out = pipe(callback_on_step_end=cb, **kw).images
    return out, n[0]


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
@pytest.mark.parametrize("strength", [0.3, 0.6])
def test_tiny_img2img_vs_fp32_oracle(kind, strength):
    from diffusers_amd import factory, init as dinit
    from diffusers_amd.unet_2d_condition import _DEFAULTS as UD
    steps, guidance, hw = 10, 5.0, 64
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    pipe = build(device=DEV, tiny=True, seed=0, img2img=True)
    ucfg = dict(UD)
    ucfg.update(dinit.TINY_SDXL_UNET if kind == "sdxl" else dinit.TINY_SD15_UNET)
    udim = ucfg["cross_attention_dim"]
    pe, npe, te, nte = _embeds(3, 1, 7, udim if isinstance(udim, int) else udim[0], 64 if kind == "sdxl" else 0)
    img = torch.rand(1, 3, hw, hw, generator=torch.Generator().manual_seed(4))
    kw = dict(image=img, strength=strength, num_inference_steps=steps, guidance_scale=guidance, prompt_embeds=pe.to(DEV),
              negative_prompt_embeds=npe.to(DEV), output_type="pt")
    if kind == "sdxl":
        kw.update(pooled_prompt_embeds=te.to(DEV), negative_pooled_prompt_embeds=nte.to(DEV))
    out_g, n_g = _count_steps(pipe, generator=torch.Generator().manual_seed(21), use_graph=True, **kw)
    out_e, n_e = _count_steps(pipe, generator=torch.Generator().manual_seed(21), use_graph=False, **kw)
    torch.cuda.synchronize()
    want_n = min(int(steps * strength), steps)
    assert n_g == n_e == want_n
    assert torch.equal(out_g, out_e), "graph replay and eager launches differ"

    # fp32 oracle: the same draws (posterior eps in fp32 for the force_upcast SDXL path, bf16 for SD1.5; then the add_noise noise)
    vcfg = dict(pipe.vae.config)
    sf = vcfg["scaling_factor"]
    usd = {k: v.float() for k, v in factory.build_unet(dinit.TINY_SDXL_UNET if kind == "sdxl" else dinit.TINY_SD15_UNET,
                                                       seed=0, device="cpu")[1].items()}
    _, vsd = factory.build_vae(dinit.TINY_VAE, seed=1, device="cpu", with_encoder=True)
    vsd = {k: v.float() for k, v in vsd.items()}
    g = torch.Generator().manual_seed(21)
    eps1 = torch.randn(1, 4, hw // 2, hw // 2, generator=g, dtype=torch.float32 if kind == "sdxl" else bf16).float()
    noise = torch.randn(1, 4, hw // 2, hw // 2, generator=g, dtype=bf16).float()
    mom = encoder_ref(vsd, vcfg, img * 2 - 1)
    mean, logvar = mom[:, :4], mom[:, 4:].clamp(-30, 20)
    z = (mean + torch.exp(0.5 * logvar) * eps1) * sf
    if kind == "sdxl":
        sch = EulerOracle(**factory.SDXL_SCHEDULER)
    else:
        sch = DDIMOracle(**factory.SD15_SCHEDULER)
    sch.set_timesteps(steps)
    t_start = steps - want_n
    ts = sch.timesteps[t_start:]
    if kind == "sdxl":
        sch.step_index = t_start
        x = z + noise * sch.sigmas[t_start]
        ids = torch.tensor([[hw, hw, 0, 0, hw, hw]], dtype=torch.float32)
        added = {"text_embeds": torch.cat([nte, te]).float(), "time_ids": ids.repeat(2, 1)}
    else:
        ac = sch.alphas_cumprod[int(ts[0])]
        x = ac ** 0.5 * z + (1 - ac) ** 0.5 * noise
        added = None
    ehs = torch.cat([npe, pe]).float()
    for t in ts:
        xin = sch.scale_model_input(x) if kind == "sdxl" else x
        eps = R.unet_forward(usd, ucfg, torch.cat([xin, xin]), float(t), ehs, added)
        e = cfg_combine(eps[:1], eps[1:], guidance)
        x = sch.step(e, x) if kind == "sdxl" else sch.step(e, int(t), x)
    ref = (R.vae_decode(vsd, vcfg, x / sf) * 0.5 + 0.5).clamp(0, 1)
    ps = _psnr01(out_g, ref)
    print(f"tiny {kind} img2img strength {strength}: {n_g} steps, PSNR vs fp32 oracle {ps:.1f} dB")
    assert ps >= 30.0


def test_base_to_refiner_handoff_is_bit_identical():
    """base(denoising_end=0.8, output_type="latent") -> img2img(image=latents, denoising_start=0.8) on the same U-Net and
    scheduler equals the full base run bit for bit (graph replay on both sides)."""
    from diffusers_amd import factory
    from diffusers_amd.pipelines import StableDiffusionXLImg2ImgPipeline
    base = factory.build_sdxl_pipeline(device=DEV, tiny=True, seed=0)
    ref = StableDiffusionXLImg2ImgPipeline(vae=base.vae, unet=base.unet, scheduler=base.scheduler)
    pe, npe, te, nte = _embeds(3, 1, 7, 64, 64)
    emb = dict(prompt_embeds=pe.to(DEV), negative_prompt_embeds=npe.to(DEV), pooled_prompt_embeds=te.to(DEV),
               negative_pooled_prompt_embeds=nte.to(DEV))
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(8)).to(bf16)
    full = base(latents=lat.to(DEV), num_inference_steps=12, guidance_scale=5.0, height=32, width=32, output_type="latent",
                **emb).images.clone()
    mid = base(latents=lat.to(DEV), num_inference_steps=12, guidance_scale=5.0, height=32, width=32, output_type="latent",
               denoising_end=0.8, **emb).images.clone()
    _, n = _count_steps(ref, image=mid, num_inference_steps=12, denoising_start=0.8, guidance_scale=5.0, output_type="latent",
                        **emb)
    out = ref(image=mid, num_inference_steps=12, denoising_start=0.8, guidance_scale=5.0, output_type="latent", **emb).images
    torch.cuda.synchronize()
    assert n > 0 and not torch.equal(mid, full)
    assert torch.equal(out, full)
    assert not torch.equal(mid, out)              # the caller's latents were not used as the loop's buffer


def _tiny_sdxl_img2img_call():
    from diffusers_amd import factory
    pipe = factory.build_sdxl_pipeline(device=DEV, tiny=True, seed=0, img2img=True)
    pe, npe, te, nte = _embeds(3, 1, 7, 64, 64)
    emb = dict(prompt_embeds=pe.to(DEV), negative_prompt_embeds=npe.to(DEV), pooled_prompt_embeds=te.to(DEV),
               negative_pooled_prompt_embeds=nte.to(DEV), num_inference_steps=4, strength=0.5, output_type="latent")
    u8 = np.random.default_rng(0).integers(0, 256, (32, 48, 3), dtype=np.uint8)
    return lambda image: pipe(image=image, generator=torch.Generator().manual_seed(1), **emb).images.clone(), u8


def test_img2img_accepts_numpy_images():
    call, u8 = _tiny_sdxl_img2img_call()
    with pytest.raises(ValueError, match="31 x 48"):
        call(u8[:31])                              # the tiny VAE's scale factor is 2
    a = call(u8)
    f = torch.from_numpy(u8).float() / 255.0
    assert torch.equal(a, call(f.permute(2, 0, 1)[None]))        # uint8 x / 255 in the kernel == the caller's fp32 division
    assert torch.equal(a, call(f.numpy()))                       # float NHWC array


def test_img2img_accepts_pil_images():
    Image = pytest.importorskip("PIL.Image")
    call, u8 = _tiny_sdxl_img2img_call()
    assert torch.equal(call(Image.fromarray(u8)), call(u8))


@pytest.mark.skipif(not RR.available(), reason="reference archive oracle/_ref/diffusers_ref.zip did not ship")
@pytest.mark.parametrize("case", [dict(strength=0.3), dict(strength=0.6), dict(denoising_start=0.8)])
def test_tiny_sdxl_img2img_vs_reference_pipeline(case):
    """The engine's StableDiffusionXLImg2ImgPipeline against the REAL reference StableDiffusionXLImg2ImgPipeline in fp32 on the same
    weights (encoder included), image, embeddings and generator: the reference's own preprocessing, get_timesteps / begin index,
    retrieve_latents + add_noise draw order and time ids.  ``denoising_start``: 4-channel latents in, no noise added."""
    from diffusers_amd import factory, init as dinit
    ref = RR.load_reference()
    f32 = torch.float32
    # the generator lives on the GPU: there a bf16 draw is the fp32 draw rounded (on the CPU the two dtypes take different paths),
    # so the fp32 reference's noise and the bf16 engine's (what a bf16 reference draws) are the same numbers
    ga, gb = torch.Generator(DEV).manual_seed(5), torch.Generator(DEV).manual_seed(5)
    assert torch.equal(torch.randn(4, 999, generator=ga, device=DEV, dtype=bf16),
                       torch.randn(4, 999, generator=gb, device=DEV, dtype=f32).to(bf16)), "premise of this comparison"
    pipe = factory.build_sdxl_pipeline(device=DEV, tiny=True, seed=0, img2img=True)
    _, usd = factory.build_unet(dinit.TINY_SDXL_UNET, seed=0, device="cpu")
    _, vsd = factory.build_vae(dinit.TINY_VAE, seed=1, device="cpu", with_encoder=True)
    rpipe = ref.StableDiffusionXLImg2ImgPipeline(
        vae=RR.build_vae(ref, dinit.TINY_VAE, vsd, DEV, f32), text_encoder=None, text_encoder_2=None, tokenizer=None,
        tokenizer_2=None, unet=RR.build_unet(ref, dinit.TINY_SDXL_UNET, usd, DEV, f32),
        scheduler=ref.EulerDiscreteScheduler(**factory.SDXL_SCHEDULER))
    rpipe.set_progress_bar_config(disable=True)
    pe, npe, te, nte = _embeds(3, 1, 7, 64, 64)
    if "denoising_start" in case:
        image = torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(6)).to(bf16).to(DEV)
    else:
        image = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    kw = dict(num_inference_steps=10, guidance_scale=5.0, output_type="pt", **case)

    def run(p, dtype):
        n = [0]

        def cb(pp, i, t, d):
            n[0] += 1
            return {}
        with torch.no_grad():
            out = p(image=image.to(dtype) if image.shape[1] == 4 else image, prompt_embeds=pe.to(DEV, dtype),
                    negative_prompt_embeds=npe.to(DEV, dtype), pooled_prompt_embeds=te.to(DEV, dtype),
                    negative_pooled_prompt_embeds=nte.to(DEV, dtype), generator=torch.Generator(DEV).manual_seed(21),
                    callback_on_step_end=cb, **kw).images
        return out, n[0]
    want, n_ref = run(rpipe, f32)
    got, n_eng = run(pipe, bf16)
    ps = _psnr01(got, want)
    print(f"tiny SDXL img2img {case} vs the reference pipeline (fp32): {n_eng} steps, PSNR {ps:.1f} dB")
    assert n_eng == n_ref and got.shape == want.shape
    assert ps >= 40.0
