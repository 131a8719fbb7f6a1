"""GPU: the 16-channel posterior and the FLUX latent-preparation kernel (csrc/vae_encode.hip) against the restatement of that file's
header, their memory footprint, AutoencoderKL.encode of the 16-channel VAE, and the FLUX img2img / inpainting pipelines: identities
(graph = plan = eager, no recapture, mask of ones = img2img, mask of zeros = the image latents, strength 1 = FluxPipeline), accuracy
against an fp32 oracle loop assembled here and -- where the reference archive shipped -- against the reference's own pipelines."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flux_img2img_emulation as FE
from footprint import bits_equal, guarded, poisoned
from oracle import ref_runtime as RR
from oracle import reference_math as R
from oracle.samplers import FlowMatchOracle
from test_kernel_footprint_gpu import _check, _p, _stream, rnd, run_both
from test_vae_encode_gpu import _encode_case, _k2_ref, _ulps, encoder_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16
LC = 16
SCALE, SHIFT, A, B_ = 0.3611, 0.1159, 0.6914, 0.3086          # (a, b: any pair of bf16 values)


def _same(got, want, sample):
    """MEAN / MOMENTS / NOISE: to the bit.  SAMPLE: std = exp(...) is the one step whose fp32 value comes from a library function --
    the kernel's expf and torch's may differ in the last fp32 bit, which moves a bf16 rounding in rare ties: at most one bf16 ulp, in
    fewer than 1 % of the elements (the rule of tests/test_vae_encode_gpu.py)."""
    if sample:
        assert _ulps(got, want) <= 1.0 and (got != want).float().mean() < 0.01
    else:
        assert torch.equal(got, want)


def _raw(B, HW, g, channels=2 * LC):
    """conv_out result [B][2L][HW]: means ~ N(0, 9), log-variances reaching past both clamp ends (-30, 20)."""
    raw = torch.randn(B, channels, HW, generator=g) * 3
    if channels == 2 * LC:
        raw[:, LC:] = torch.linspace(-45, 35, B * LC * HW).reshape(B, LC, HW)[:, torch.randperm(LC, generator=g)]
    return raw.to(bf16)


def _layout(raw, layout):
    """The source tensor and its (sB, sC, sP) for ``raw`` [B][C][HW]."""
    B, C, HW = raw.shape
    if layout == "nchw":
        return raw.contiguous(), (C * HW, HW, 1)
    sP = C if layout == "nhwc" else C + 8                        # "nhwc_wide": a pixel stride larger than the channel count
    src = torch.zeros(B, HW, sP, dtype=bf16)
    src[:, :, :C] = raw.transpose(1, 2)
    return src, (HW * sP, 1, sP)


# ---- da_vae_posterior_latents, L = 16 ---------------------------------------------------------------------------------------
_POST_CASES = [("moments", False, None, None)] + [(m, n, sh, sc) for m in ("mean", "sample") for n in (False, True)
                                                  for sh, sc in ((None, None), (SHIFT, SCALE), (None, SCALE))]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])             # nhwc: sP = 32, the implicit-GEMM conv_out result
@pytest.mark.parametrize("mode,noise,shift,scale", _POST_CASES)
def test_posterior_latents_16_channels_matches_restatement(layout, mode, noise, shift, scale):
    from diffusers_amd import _lib as L, ops
    g = torch.Generator().manual_seed(7)
    B, H, W = 2, 9, 13
    HW = H * W
    raw = _raw(B, HW, g)
    eps1 = torch.randn(B, LC, HW, generator=g).to(bf16) if mode == "sample" else None
    eps2 = torch.randn(B, LC, HW, generator=g).to(bf16) if noise else None
    a, b = (A, B_) if noise else (1.0, 0.0)
    src, strides = _layout(raw, layout)
    assert layout != "nhwc" or strides[2] == 32
    m = {"moments": L.POSTERIOR_MOMENTS, "mean": L.POSTERIOR_MEAN, "sample": L.POSTERIOR_SAMPLE}[mode]
    dv = lambda t: None if t is None else t.to(DEV).contiguous()     # noqa: E731
    y = ops.vae_posterior_latents(dv(src), strides, batch=B, hw=HW, latent_channels=LC, mode=m, eps1=dv(eps1), eps2=dv(eps2),
                                  scale=scale, shift=shift, a=a, b=b)
    want = _k2_ref(raw.to(DEV), None, None, dv(eps1), dv(eps2), mode, scale, shift, a, b)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B, 2 * LC if mode == "moments" else LC, HW)
    _same(y, want, mode == "sample")


def test_posterior_latents_16_channels_with_a_quant_conv_stays_unsupported():
    from diffusers_amd import _lib as L, ops
    x = torch.zeros(1, 32, 4, dtype=bf16, device=DEV)
    with pytest.raises(RuntimeError, match="DA_ERR_UNSUPPORTED"):
        ops.vae_posterior_latents(x, (128, 4, 1), batch=1, hw=4, latent_channels=16, mode=L.POSTERIOR_MEAN,
                                  wq=torch.zeros(32, 32, dtype=bf16, device=DEV), bq=torch.zeros(32, dtype=bf16, device=DEV))


# ---- da_flux_prepare_latents --------------------------------------------------------------------------------------------------
def _prepare_case(B, H, W, layout, mode, outputs, seed=11):
    from diffusers_amd import _lib as L, ops
    g = torch.Generator().manual_seed(seed)
    HW = H * W
    raw = _raw(B, HW, g, LC if mode == "noise" else 2 * LC)
    eps1 = torch.randn(B, LC, HW, generator=g).to(bf16).to(DEV) if mode == "sample" else None
    noise = torch.randn(B, LC, HW, generator=g).to(bf16).to(DEV)
    src, strides = _layout(raw, layout)
    m = {"mean": L.POSTERIOR_MEAN, "sample": L.POSTERIOR_SAMPLE, "noise": L.POSTERIOR_NOISE}[mode]
    shift, scale = (None, None) if mode == "noise" else (SHIFT, SCALE)
    got = ops.flux_prepare_latents(src.to(DEV), strides, batch=B, height=H, width=W, latent_channels=LC, mode=m, eps1=eps1,
                                   noise=noise.view(B, LC, H, W), shift=shift, scale=scale, a=A, b=B_, want_image_latents=outputs,
                                   want_noise=outputs)
    # the restatement of the file's header, then FluxPipeline._pack_latents (NOISE: the input is the latents -- mean of [z | z])
    r = raw.to(DEV) if mode != "noise" else torch.cat([raw, raw], 1).to(DEV)
    kind = "sample" if mode == "sample" else "mean"
    x = _k2_ref(r, None, None, eps1, noise, kind, scale, shift, A, B_)
    z = _k2_ref(r, None, None, eps1, None, kind, scale, shift, 1.0, 0.0)
    pk = lambda t: FE.pack_latents(t.reshape(B, LC, H, W))       # noqa: E731
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (B, (H // 2) * (W // 2), 4 * LC) and got[0].is_contiguous()
    _same(got[0], pk(x), mode == "sample")
    if outputs:
        _same(got[1], pk(z), mode == "sample")
        assert torch.equal(got[2], pk(noise))
    else:
        assert got[1] is None and got[2] is None


@pytest.mark.parametrize("outputs", [True, False])               # False: the optional outputs are NULL
@pytest.mark.parametrize("mode", ["mean", "sample", "noise"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "nhwc_wide"])
@pytest.mark.parametrize("B,H,W", [(2, 6, 10), (1, 2, 2), (3, 16, 24)])      # 3 x 5 tokens: odd and not square; one token; several blocks
def test_flux_prepare_latents_matches_packed_restatement(B, H, W, layout, mode, outputs):
    _prepare_case(B, H, W, layout, mode, outputs)


def test_flux_prepare_latents_grid_stride_takes_a_second_trip():
    """16 384 blocks of 256 (token, channel) threads cover 4 194 304 pairs: a 1024 x 1040 latent grid has 4 259 840."""
    assert 1024 * 1040 // 4 * LC > 16384 * 256
    _prepare_case(1, 1024, 1040, "nchw", "noise", True)


def test_pack_order_is_the_pipelines():
    from diffusers_amd.pipelines import FluxPipeline
    x = torch.arange(2 * 16 * 6 * 10, dtype=torch.float32).reshape(2, 16, 6, 10)
    p = FE.pack_latents(x)
    assert torch.equal(p, FluxPipeline._pack_latents(x, 2, 16, 6, 10))
    assert p[1, 1 * 5 + 3, 7 * 4 + 1 * 2 + 0] == x[1, 7, 2 * 1 + 1, 2 * 3 + 0]      # token (i, j), column c * 4 + di * 2 + dj


# ---- footprint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (6, 10), (34, 62)])
def test_flux_prepare_and_16_channel_posterior_footprint(H, W):
    from diffusers_amd import _lib as L
    lib, B, HW = L.load(), 2, H * W
    T = (H // 2) * (W // 2)
    g = torch.Generator().manual_seed(31)
    x = torch.zeros(B, HW, 32, dtype=bf16)
    x[:] = _raw(B, HW, g).transpose(1, 2)
    eps1, noise = rnd((B, LC, HW), 170), rnd((B, LC, HW), 171)
    # SAMPLE from the NHWC layout with a padded pixel stride (40: the tail of every pixel is poisoned), all three outputs guarded
    r = run_both("flux_prepare sample", lambda i, o: _check(L, lib.da_flux_prepare_latents(
        _p(i["x"]), HW * 40, 1, 40, _p(i["eps1"]), _p(i["noise"]), _p(o["x"]), _p(o["z"]), _p(o["n"]), B, H, W, LC, L.POSTERIOR_SAMPLE,
        L.LATENTS_SHIFT | L.LATENTS_SCALE, SHIFT, SCALE, A, B_, _stream()), "prepare"),
        dict(x=poisoned(x.to(DEV), ld=40), eps1=poisoned(eps1), noise=poisoned(noise)),
        lambda: dict(x=guarded((B, T, 64)), z=guarded((B, T, 64)), n=guarded((B, T, 64))))
    assert bits_equal(r["n"], FE.pack_latents(noise.reshape(B, LC, H, W)).contiguous())
    # NOISE from NCHW latents, optional outputs NULL
    lat = rnd((B, LC, HW), 172)
    r = run_both("flux_prepare noise", lambda i, o: _check(L, lib.da_flux_prepare_latents(
        _p(i["x"]), LC * HW, HW, 1, None, _p(i["noise"]), _p(o["x"]), None, None, B, H, W, LC, L.POSTERIOR_NOISE, 0, 0.0, 1.0, 0.75, 0.625,
        _stream()), "prepare"), dict(x=poisoned(lat), noise=poisoned(noise)), lambda: dict(x=guarded((B, T, 64))))
    want = ((0.75 * lat.float()).to(bf16).float() + (0.625 * noise.float()).to(bf16).float()).to(bf16)
    assert bits_equal(r["x"], FE.pack_latents(want.reshape(B, LC, H, W)).contiguous())
    # the 16-channel posterior: MOMENTS and SAMPLE + add_noise from the padded NHWC layout
    p = run_both("posterior16 moments", lambda i, o: _check(L, lib.da_vae_posterior_latents(
        _p(i["x"]), HW * 40, 1, 40, None, None, None, None, _p(o["y"]), B, HW, LC, L.POSTERIOR_MOMENTS, 0, 0.0, 1.0, 1.0, 0.0, _stream()),
        "moments"), dict(x=poisoned(x.to(DEV), ld=40)), lambda: dict(y=guarded((B, 32, HW))))["y"]
    assert bits_equal(p, x.to(DEV).transpose(1, 2).contiguous())
    run_both("posterior16 sample", lambda i, o: _check(L, lib.da_vae_posterior_latents(
        _p(i["x"]), HW * 40, 1, 40, None, None, _p(i["eps1"]), _p(i["noise"]), _p(o["y"]), B, HW, LC, L.POSTERIOR_SAMPLE,
        L.LATENTS_SHIFT | L.LATENTS_SCALE, SHIFT, SCALE, A, B_, _stream()), "sample"),
        dict(x=poisoned(x.to(DEV), ld=40), eps1=poisoned(eps1), noise=poisoned(noise)), lambda: dict(y=guarded((B, LC, HW))))


# ---- AutoencoderKL.encode, 16 channels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gemm_path", [False, True])
def test_tiny_flux_vae_encode_vs_fp32_encoder(gemm_path):
    """Under tests/test_vae_encode_gpu.py's own gate for the 4-channel encoder (rel_rms <= 1.5 x the torch-bf16 floor + 2e-3); the
    figure is printed.  conv_out (128 -> 32) runs on the implicit-GEMM conv, the posterior reads its NHWC result in place."""
    vae, dist = _encode_case("TINY_FLUX_VAE", 64, gemm_path)
    assert dist._strides == (32 * 32 * 32, 1, 32) and tuple(dist.parameters.shape) == (1, 32, 32, 32)
    assert torch.equal(dist.mode(), dist.mean) and torch.equal(dist.logvar, dist.parameters[:, 16:].clamp(-30, 20))
    g = torch.Generator().manual_seed(11)
    z = dist.sample(generator=g)
    eps = torch.randn(dist.mean.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float32).to(DEV).to(bf16)
    want = dist.mean + dist.std * eps
    assert _ulps(z, want) <= 1.0 and (z != want).float().mean() < 0.01
    sh, sc = float(vae.config.shift_factor), float(vae.config.scaling_factor)
    want = _k2_ref(dist.parameters.reshape(1, 32, -1), None, None, eps.reshape(1, 16, -1), None, "sample", sc, sh, 1.0, 0.0)
    _same(dist.latents(eps, shift=sh, scale=sc).reshape(1, 16, -1), want, True)


# ---- pipelines ------------------------------------------------------------------------------------------------------------------------
def _build(kind):
    from diffusers_amd import factory
    return factory.build_flux_pipeline(device=DEV, tiny=True, seed=5, img2img=kind == "img2img", inpaint=kind == "inpaint")


def _embeds():
    g = torch.Generator().manual_seed(3)
    return torch.randn(1, 16, 64, generator=g).to(bf16), torch.randn(1, 64, generator=g).to(bf16)


def _kw(output_type="latent"):
    pe, pp = _embeds()
    return dict(prompt_embeds=pe.to(DEV), pooled_prompt_embeds=pp.to(DEV), num_inference_steps=4, output_type=output_type,
                max_sequence_length=16)


def _image(seed=4):
    return torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(seed))


def _rect_mask(H=64, W_=64):
    m = torch.zeros(H, W_)
    m[H // 4:3 * H // 4, W_ // 8:W_ // 2] = 1.0
    return m


def _gen(seed=21):
    return torch.Generator().manual_seed(seed)


def _extra(kind, mask=None):
    return dict(mask_image=_rect_mask() if mask is None else mask) if kind == "inpaint" else {}


@pytest.mark.parametrize("kind", ["img2img", "inpaint"])
def test_graph_plan_and_eager_agree(kind):
    outs = {}
    for mode in (True, "plan", False):
        outs[mode] = _build(kind)(image=_image(), strength=0.6, generator=_gen(), use_graph=mode, **_extra(kind), **_kw()).images.clone()
    torch.cuda.synchronize()
    assert torch.isfinite(outs[True].float()).all() and tuple(outs[True].shape) == (1, 256, 64)
    assert torch.equal(outs[True], outs[False]), "graph replay and eager launches differ"
    assert torch.equal(outs["plan"], outs[False]), "plan replay and eager launches differ"


@pytest.mark.parametrize("kind", ["img2img", "inpaint"])
def test_second_call_with_another_image_mask_and_strength_does_not_recapture(kind):
    pipe = _build(kind)
    first = pipe(image=_image(), strength=0.6, generator=_gen(), **_extra(kind), **_kw()).images.clone()
    graph = pipe._graph
    m2 = torch.zeros(64, 64)
    m2[:, :32] = 1.0
    second = pipe(image=_image(8), strength=0.3, generator=_gen(7), **_extra(kind, m2), **_kw()).images.clone()
    assert pipe._graph is graph, "same shapes: the captured step must be replayed, its inputs refreshed in place"
    fresh = _build(kind)(image=_image(8), strength=0.3, generator=_gen(7), use_graph=False, **_extra(kind, m2), **_kw()).images
    assert torch.equal(second, fresh) and not torch.equal(first, second)


def test_masks_of_ones_and_zeros_and_strength_one():
    img = _image()
    i2i, inp = _build("img2img"), _build("inpaint")
    ref = i2i(image=img, strength=0.6, generator=_gen(), **_kw()).images.clone()
    ones = inp(image=img, mask_image=torch.ones(64, 64), strength=0.6, generator=_gen(), **_kw()).images.clone()
    assert torch.equal(ones, ref), "a mask of ones must leave the img2img loop untouched"
    zeros = inp(image=img, mask_image=torch.zeros(64, 64), strength=0.6, generator=_gen(), **_kw()).images.clone()
    # the packed image latents of the same posterior draw
    vc = inp.vae.config
    dist = inp.vae.encode_image((2.0 * img - 1.0).to(DEV).contiguous(), nchw=True, normalize=False)
    z = dist.latents(dist.draw_noise(_gen(), dtype=bf16), shift=float(vc.shift_factor), scale=float(vc.scaling_factor))
    assert torch.equal(zeros, FE.pack_latents(z)) and not torch.equal(zeros, ones)
    # strength 1: the text-to-image pipeline on the same noise (the second draw)
    from diffusers_amd.pipelines import FluxPipeline
    full = i2i(image=img, strength=1.0, generator=_gen(), **_kw()).images.clone()
    g = _gen()
    torch.randn(1, 16, 32, 32, generator=g, dtype=bf16)
    noise = torch.randn(1, 16, 32, 32, generator=g, dtype=bf16)
    t2i = FluxPipeline(scheduler=i2i.scheduler, vae=i2i.vae, transformer=i2i.transformer)
    assert torch.equal(full, t2i(latents=FE.pack_latents(noise), height=64, width=64, **_kw()).images)


def test_step_callback_sees_the_blended_latents():
    """After step i: (1 - m) * scale_noise(image latents, sigma[i + 1], noise) + m * (the step's result), as the reference's bf16
    torch ops; the step's own result is taken from an img2img loop fed the blended latents through its callback."""
    from diffusers_amd import ops
    pipe = _build("inpaint")
    seen = []
    out = pipe(image=_image(), mask_image=_rect_mask(), strength=0.6, generator=_gen(),
               callback_on_step_end=lambda p, i, t, d: seen.append(d["latents"].clone()) or {}, **_kw()).images
    st = pipe._inpaint
    tab, m = st["table"].cpu().tolist(), st["mask"].reshape(1, 256, 64)
    assert len(seen) == 3 and torch.equal(seen[-1], out) and tab[4] == [1.0, 0.0]
    start = FE.pack_latents(FE.scale_noise_ref(_unpack(st["image_latents"]), pipe.scheduler.sigmas[1].float().cpu(), _unpack(st["noise"])))
    # replay the plain step from the blended latents: the img2img pipeline, its latents replaced after every step
    i2i = _build("img2img")
    raw = []

    def cb(p, i, t, d):
        raw.append(d["latents"].clone())
        return {"latents": seen[i]}
    i2i(image=_image(), strength=0.6, generator=_gen(), callback_on_step_end=cb, **_kw())
    for i in range(3):
        a, b = tab[1 + i + 1]
        proper = ops.add_noise(st["image_latents"], st["noise"], a, b)
        assert torch.equal(seen[i], FE.blend_ref(m, proper, raw[i])), i
    assert torch.equal(ops.add_noise(st["image_latents"], st["noise"], *tab[1]), start)


def _unpack(x, h=32, w=32):
    B = x.shape[0]
    return x.view(B, h // 2, w // 2, 16, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, 16, h, w)


# ---- accuracy -----------------------------------------------------------------------------------------------------------------------
def _psnr01(a, b):
    mse = float((a.float().cpu() - b.float().cpu()).pow(2).mean())
    return 10 * np.log10(1.0 / max(mse, 1e-12))


def _oracle(kind, strength, img, mask, seed, steps=4, hw=64):
    """The reference loop in fp32 on the CPU: encoder, posterior sample, (z - shift) * scale, scale_noise, the transformer on packed
    tokens, the FlowMatch-Euler step, the mask blend (inpainting), decode."""
    from diffusers_amd import factory, init as dinit
    from diffusers_amd.autoencoder_kl import AutoencoderKL
    tsd = {k: v.float() for k, v in dinit.random_state_dict(dinit.flux_param_shapes(dinit.TINY_FLUX), seed=5).items()}
    _, vsd = factory.build_vae(dinit.TINY_FLUX_VAE, seed=6, device="cpu", with_encoder=True)
    vsd = {k: v.float() for k, v in vsd.items()}
    vcfg = dict(AutoencoderKL(**dinit.TINY_FLUX_VAE).config)
    sf, sh = vcfg["scaling_factor"], vcfg["shift_factor"]
    h = w = hw // 2
    g = torch.Generator().manual_seed(seed)
    mom = encoder_ref(vsd, vcfg, img * 2 - 1)
    mean, logvar = mom[:, :16], mom[:, 16:].clamp(-30, 20)
    eps = torch.randn(1, 16, h, w, generator=g, dtype=bf16).float()
    noise = torch.randn(1, 16, h, w, generator=g, dtype=bf16).float()
    z = (mean + torch.exp(0.5 * logvar) * eps - sh) * sf
    sch = FlowMatchOracle(shift=1.0)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / steps, steps))
    n_steps, t_start = FE.get_timesteps_ref(steps, strength)
    scale_noise = lambda j: FE.pack_latents(sch.sigmas[j] * noise + (1.0 - sch.sigmas[j]) * z)     # noqa: E731  (sigmas[steps] = 0)
    x = scale_noise(t_start)
    sch.step_index = t_start
    pe, pp = _embeds()
    ids = torch.zeros(h // 2, w // 2, 3)
    ids[..., 1] += torch.arange(h // 2)[:, None]
    ids[..., 2] += torch.arange(w // 2)[None, :]
    img_ids, txt_ids = ids.reshape(-1, 3), torch.zeros(pe.shape[1], 3)
    if kind == "inpaint":
        m = FE.pack_latents(F.interpolate((mask >= 0.5).float()[None, None], size=(h, w)).repeat(1, 16, 1, 1))
    for i in range(t_start, steps):
        v = R.flux_forward(tsd, dinit.TINY_FLUX, x, pe.float(), pp.float(), (sch.timesteps[i] / 1000).expand(1), img_ids, txt_ids)
        x = sch.step(v, x)
        if kind == "inpaint":
            x = (1 - m) * scale_noise(i + 1) + m * x
    return (R.vae_decode(vsd, vcfg, _unpack(x, h, w) / sf + sh) * 0.5 + 0.5).clamp(0, 1), n_steps


@pytest.mark.parametrize("kind", ["img2img", "inpaint"])
@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_tiny_flux_img2img_inpaint_vs_fp32_oracle(kind, strength):
    """Gate: image PSNR >= 30 dB, the gate test_tiny_img2img_vs_fp32_oracle / test_tiny_inpaint_vs_fp32_oracle apply to tiny models
    against the same kind of oracle.  Measured on one MI355X (strength 1.0 / 0.6): img2img 55.7 / 54.7 dB, inpainting 54.6 / 53.7 dB
    (DESIGN.md 8d)."""
    img, mask = _image(), _rect_mask()
    n = [0]

    def cb(p, i, t, d):
        n[0] += 1
        return {}
    out = _build(kind)(image=img, strength=strength, generator=_gen(), callback_on_step_end=cb, **_extra(kind, mask), **_kw("pt")).images
    torch.cuda.synchronize()
    with torch.no_grad():
        ref, want_n = _oracle(kind, strength, img, mask, 21)
    ps = _psnr01(out, ref)
    print(f"tiny FLUX {kind} strength {strength}: {want_n} steps, PSNR vs fp32 oracle {ps:.1f} dB")
    assert n[0] == want_n and tuple(out.shape) == (1, 3, 64, 64)
    assert ps >= 30.0


@pytest.mark.skipif(not RR.available(), reason="reference archive oracle/_ref/diffusers_ref.zip did not ship")
@pytest.mark.parametrize("kind", ["img2img", "inpaint"])
@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_tiny_flux_img2img_inpaint_vs_reference_pipeline(kind, strength):
    """The REAL reference FluxImg2ImgPipeline / FluxInpaintPipeline in fp32 on the same weights, image, mask, embeddings and device
    generator.  Gate tied to the reference's own floor: the engine's PSNR against the fp32 reference may be at most 3 dB below the
    PSNR of the reference's own bf16 run against its fp32 run (3 dB: the margin for the engine's different, fused, rounding points on
    a 4-step tiny model)."""
    from diffusers_amd import factory, init as dinit
    ref = RR.load_reference()
    f32 = torch.float32
    ga, gb = torch.Generator(DEV).manual_seed(5), torch.Generator(DEV).manual_seed(5)
    assert torch.equal(torch.randn(4, 999, generator=ga, device=DEV, dtype=bf16),
                       torch.randn(4, 999, generator=gb, device=DEV, dtype=f32).to(bf16)), "premise of this comparison"
    tsd = dinit.random_state_dict(dinit.flux_param_shapes(dinit.TINY_FLUX), seed=5)
    _, vsd = factory.build_vae(dinit.TINY_FLUX_VAE, seed=6, device="cpu", with_encoder=True)
    pe, pp = _embeds()
    image, mask = _image().to(DEV), _rect_mask()[None, None].to(DEV)

    def reference(dtype):
        tr = RR.build_model(ref, "FluxTransformer2DModel", dinit.TINY_FLUX, tsd, DEV, dtype)
        vae = RR.build_vae(ref, dinit.TINY_FLUX_VAE, vsd, DEV, dtype)
        cls = ref.FluxInpaintPipeline if kind == "inpaint" else ref.FluxImg2ImgPipeline
        p = cls(scheduler=ref.FlowMatchEulerDiscreteScheduler(shift=1.0, use_dynamic_shifting=False), vae=vae, text_encoder=None,
                tokenizer=None, text_encoder_2=None, tokenizer_2=None, transformer=tr)
        p.set_progress_bar_config(disable=True)
        return p

    def run(p, dtype):
        n = [0]

        def cb(pp_, i, t, d):
            n[0] += 1
            return {}
        extra = dict(mask_image=mask) if kind == "inpaint" else {}
        with torch.no_grad():
            out = p(image=image, strength=strength, num_inference_steps=4, guidance_scale=0.0, height=64, width=64, output_type="pt",
                    prompt_embeds=pe.to(DEV, dtype), pooled_prompt_embeds=pp.to(DEV, dtype), max_sequence_length=16,
                    generator=torch.Generator(DEV).manual_seed(21), callback_on_step_end=cb, **extra).images
        return out, n[0]
    want, n_ref = run(reference(f32), f32)
    floor, _ = run(reference(bf16), bf16)
    got, n_eng = run(_build(kind), bf16)
    ps, ps_floor = _psnr01(got, want), _psnr01(floor, want)
    print(f"tiny FLUX {kind} strength {strength} vs the reference pipeline (fp32): {n_eng} steps, engine PSNR {ps:.1f} dB, the "
          f"reference's own bf16 run {ps_floor:.1f} dB")
    assert n_eng == n_ref and got.shape == want.shape
    assert ps >= ps_floor - 3.0
