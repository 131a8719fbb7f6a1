"""CPU: host side of the FLUX img2img / inpainting pipelines -- the ABI tables, FlowMatchEulerDiscreteScheduler.scale_noise and its
add_noise table against the reference's bf16 torch expression, the FLUX get_timesteps, and the pipelines on the torch stand-ins of
tests/flux_img2img_emulation.py (draw order, the equalities that tie the two classes to FluxPipeline, the blend the callback sees,
the refusals, from_pretrained).  No kernel is launched."""
import inspect
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flux_img2img_emulation as FE
from diffusers_amd import _lib as L
from diffusers_amd import factory, init as dinit, loading, ops
from diffusers_amd.pipelines import FluxImg2ImgPipeline, FluxInpaintPipeline, FluxPipeline, calculate_shift, flux_get_timesteps
from diffusers_amd.schedulers import FlowMatchEulerDiscreteScheduler

bf16 = torch.bfloat16
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture
def emulated(monkeypatch):
    FE.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "TUNING", False)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_tables_carry_the_new_entry_point_without_a_plan_number():
    name = "da_flux_prepare_latents"
    assert name in L.SIGNATURES and name not in L.FN_IDS
    assert L.FN_COUNT == 36 and L.FN_IDS["da_dpmpp_2m_step"] == L.FN_COUNT - 1
    header = (ROOT / "include" / "diffusers_amd.h").read_text()
    assert f"int {name}(const void* in, long long sB, long long sC, long long sP, const void* eps1, const void* noise," in header
    assert "#define DA_ABI_VERSION 9" in header
    assert len(L.SIGNATURES[name][1]) == 20
    lib = L.load()
    assert lib.da_version() == L.ABI_VERSION == 9
    one = 1 << 12       # any non-null, 8-byte aligned value: a refused call dereferences nothing and launches nothing
    fn = lib.da_flux_prepare_latents

    def call(inp=one, eps1=one, noise=one, out=one, img=None, nz=None, B=1, H=4, W=6, Lc=16, mode=L.POSTERIOR_SAMPLE, flags=0, s=(96, 1, 32)):
        return fn(inp, s[0], s[1], s[2], eps1, noise, out, img, nz, B, H, W, Lc, mode, flags, 0.0, 1.0, 0.5, 0.5, None)

    assert call(inp=None) == 1 and call(noise=None) == 1 and call(out=None) == 1            # null required pointers
    assert call(H=5) == 1 and call(W=7) == 1                                                # odd grid
    assert call(mode=L.POSTERIOR_MOMENTS) == 1 and call(mode=4) == 1 and call(mode=-1) == 1  # a mode outside {MEAN, SAMPLE, NOISE}
    assert call(eps1=None) == 1                                                             # SAMPLE without eps1
    assert call(flags=4) == 1                                                               # flags outside the two known
    assert call(s=(-1, 1, 32)) == 1 and call(s=(96, -1, 32)) == 1 and call(s=(96, 1, -32)) == 1
    assert call(out=one + 2) == 1 and call(img=one + 4) == 1                                # misaligned packed outputs
    assert call(B=0) == 1 and call(Lc=0) == 1
    # L = 16 with a quant_conv stays unsupported by the posterior entry point; null pointers are refused before that
    post = lib.da_vae_posterior_latents
    assert post(one, 1, 1, 1, one, one, None, None, one, 1, 4, 16, L.POSTERIOR_MEAN, 0, 0.0, 1.0, 1.0, 0.0, None) == 3
    assert post(one, 1, 1, 1, None, None, None, None, one, 1, 4, 8, L.POSTERIOR_MEAN, 0, 0.0, 1.0, 1.0, 0.0, None) == 3
    assert post(None, 1, 1, 1, None, None, None, None, one, 1, 4, 16, L.POSTERIOR_MEAN, 0, 0.0, 1.0, 1.0, 0.0, None) == 1


def test_ops_wrapper_checks_arguments(monkeypatch):
    monkeypatch.setattr(ops, "_req", lambda *a, **k: None)          # (the device check: these calls never reach the library)
    x = torch.zeros(1, 4, 6, 32, dtype=bf16)
    n = torch.zeros(1, 16, 4, 6, dtype=bf16)
    kw = dict(batch=1, height=4, width=6, latent_channels=16, mode=L.POSTERIOR_MEAN, noise=n)
    with pytest.raises(ValueError, match="even latent grid"):
        ops.flux_prepare_latents(x, (768, 1, 32), **dict(kw, height=3))
    with pytest.raises(ValueError, match="reach element"):
        ops.flux_prepare_latents(x, (768, 1, 33), **kw)
    with pytest.raises(ValueError, match="reach element"):
        ops.flux_prepare_latents(x, (768, -1, 32), **kw)
    with pytest.raises(ValueError, match="noise must be a contiguous"):
        ops.flux_prepare_latents(x, (768, 1, 32), **dict(kw, noise=n[:, :8]))
    with pytest.raises(ValueError, match="eps1 is the posterior noise"):
        ops.flux_prepare_latents(x, (768, 1, 32), **dict(kw, mode=L.POSTERIOR_SAMPLE))
    with pytest.raises(ValueError, match="mode 0"):
        ops.flux_prepare_latents(x, (768, 1, 32), **dict(kw, mode=L.POSTERIOR_MOMENTS))


# ---- scheduler ------------------------------------------------------------------------------------------------------------------
def _scheduler(n, dynamic):
    sch = FlowMatchEulerDiscreteScheduler(shift=1.0 if dynamic else 3.0, use_dynamic_shifting=dynamic)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), device="cpu", mu=calculate_shift(256) if dynamic else None)
    return sch


@pytest.mark.parametrize("dynamic", [False, True])
@pytest.mark.parametrize("n", [4, 28])
def test_scale_noise_and_add_noise_table_equal_the_reference_expression(emulated, n, dynamic):
    sch = _scheduler(n, dynamic)
    g = torch.Generator().manual_seed(n)
    x, noise = (torch.randn(2, 16, 4, 6, generator=g).to(bf16) for _ in range(2))
    tab = sch.add_noise_table(bf16)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (n + 1, 2) and tab[n].tolist() == [1.0, 0.0]
    for j in range(n):
        want = FE.scale_noise_ref(x, sch.sigmas[j], noise)                 # sigma * noise + (1.0 - sigma) * sample on bf16 tensors
        a, b = (float(v) for v in tab[j])
        assert torch.equal(FE.I.add_noise(x, noise, a, b), want), j       # the arithmetic of da_inpaint_blend / the prepare kernel
        sig = sch.sigmas[j].to(bf16)
        assert (a, b) == (float(1.0 - sig), float(sig))
        # the public method: no begin index -> the timestep's index; a begin index -> that row; after a step -> the step index
        sch._begin_index = sch._step_index = None
        assert torch.equal(sch.scale_noise(x, sch.timesteps[j:j + 1], noise), want)
        sch.set_begin_index(j)
        assert torch.equal(sch.scale_noise(x, sch.timesteps[:1], noise), want)
        sch._begin_index, sch._step_index = 0, j
        assert torch.equal(sch.scale_noise(x, sch.timesteps[:1], noise), want)
    sch._begin_index = sch._step_index = None
    ptr = tab.data_ptr()
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), device="cpu", mu=0.9 if dynamic else None)
    assert sch.add_noise_table(bf16).data_ptr() == ptr                      # refreshed in place: a captured graph keeps the address
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / (n + 1), n + 1), device="cpu", mu=0.9 if dynamic else None)
    assert tuple(sch.add_noise_table(bf16).shape) == (n + 2, 2)
    with pytest.raises(ValueError, match="bf16 latents"):
        sch.scale_noise(x.float(), sch.timesteps[:1], noise.float())


@pytest.mark.parametrize("n,strength,steps,begin", [(4, 0.6, 3, 1), (4, 1.0, 4, 0), (4, 0.3, 2, 2), (28, 0.85, 24, 4), (4, 0.1, 1, 3)])
def test_get_timesteps_is_the_flux_formula(n, strength, steps, begin):
    """(4, 0.1): init_timestep = 0.4, t_start = int(3.6) = 3, so ONE step is left and the reference does not raise (the SD formula,
    with its int() around the product, would leave none); strength 0 is what leaves no step."""
    assert FE.get_timesteps_ref(n, strength) == (steps, begin)
    sch = _scheduler(n, True)
    ts, got, b = flux_get_timesteps(sch, n, strength)
    assert (got, b) == (steps, begin) and sch.begin_index == begin and torch.equal(ts, sch.timesteps[begin:])
    assert int(sch.device_step) == begin                                    # the device counter starts at the begin index


def _pipe(kind="img2img"):
    return factory.build_flux_pipeline(device="cpu", tiny=True, seed=5, img2img=kind == "img2img", inpaint=kind == "inpaint")


def _embeds(B=1):
    g = torch.Generator().manual_seed(3)
    return dict(prompt_embeds=torch.randn(B, 16, 64, generator=g).to(bf16), pooled_prompt_embeds=torch.randn(B, 64, generator=g).to(bf16))


def _image(B=1, seed=4):
    return torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(seed))


def _rect_mask(H=64, W_=64):
    m = torch.zeros(H, W_)
    m[H // 4:3 * H // 4, W_ // 8:W_ // 2] = 1.0
    return m


KW = dict(num_inference_steps=4, output_type="latent", use_graph=False, max_sequence_length=16)


def test_no_step_left_raises_the_reference_error(emulated):
    pipe = _pipe()
    with pytest.raises(ValueError, match="the number of pipeline steps is 0 which is < 1"):
        pipe(image=_image(), strength=0.0, **_embeds(), **KW)
    assert pipe(image=_image(), strength=0.1, generator=torch.Generator().manual_seed(1), **_embeds(), **KW).images.shape == (1, 256, 64)


# ---- pipelines on the stand-ins -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["img2img", "inpaint"])
def test_draw_order_and_start_latents(emulated, kind, monkeypatch):
    """(1) the posterior noise, (2) the noise, both bf16 of the latent shape, whatever force_upcast says; the loop starts from the
    reference's prepare_latents: pack(scale_noise((sample - shift_factor) * scaling_factor, sigma[t_start], noise))."""
    pipe = _pipe(kind)
    assert pipe.vae.config.force_upcast
    img = _image()
    starts = []
    monkeypatch.setattr(type(pipe), "_denoise", lambda self, x, step_args, n, ug, begin=0: starts.append((x.clone(), n, begin)) or x)
    extra = dict(mask_image=_rect_mask()) if kind == "inpaint" else {}
    pipe(image=img, strength=0.6, generator=torch.Generator().manual_seed(21), **extra, **_embeds(), **KW)
    (start, n_steps, begin), = starts
    assert (n_steps, begin) == (3, 1)
    g = torch.Generator().manual_seed(21)
    eps1 = torch.randn(1, 16, 32, 32, generator=g, dtype=bf16)
    noise = torch.randn(1, 16, 32, 32, generator=g, dtype=bf16)
    vc = pipe.vae.config
    dist = pipe.vae.encode_image((2.0 * img - 1.0).contiguous(), nchw=True, normalize=False)
    assert tuple(dist.parameters.shape) == (1, 32, 32, 32)
    # _encode_vae_image: (retrieve_latents(vae.encode(image), generator) - shift_factor) * scaling_factor as two bf16 torch ops; on
    # the GPU, where the reference runs, a Python scalar enters such an op in fp32 (torch's CPU kernels round it to bf16 first),
    # so the restatement spells the fp32 arithmetic and the two bf16 rounds out
    z = ((dist.latents(eps1).float() - vc.shift_factor).to(bf16).float() * vc.scaling_factor).to(bf16)
    assert torch.equal(z, dist.latents(eps1, shift=vc.shift_factor, scale=vc.scaling_factor))
    want = FE.pack_latents(FE.scale_noise_ref(z, pipe.scheduler.sigmas[1], noise))
    assert torch.equal(start, want)
    if kind == "inpaint":
        st = pipe._inpaint
        assert torch.equal(st["image_latents"], FE.pack_latents(z)) and torch.equal(st["noise"], FE.pack_latents(noise))
        mlat = F.interpolate((_rect_mask() >= 0.5).float()[None, None], size=(32, 32)).repeat(1, 16, 1, 1)
        assert torch.equal(st["mask"], FE.pack_latents(mlat).to(bf16).reshape(1, 1, -1))
        assert tuple(st["table"].shape) == (5, 2)


def test_strength_one_equals_the_text_to_image_pipeline_on_the_same_noise(emulated):
    pipe = _pipe()
    out = pipe(image=_image(), strength=1.0, generator=torch.Generator().manual_seed(7), **_embeds(), **KW).images
    g = torch.Generator().manual_seed(7)
    torch.randn(1, 16, 32, 32, generator=g, dtype=bf16)
    noise = torch.randn(1, 16, 32, 32, generator=g, dtype=bf16)
    t2i = FluxPipeline(scheduler=pipe.scheduler, vae=pipe.vae, transformer=pipe.transformer)
    want = t2i(latents=FE.pack_latents(noise), height=64, width=64, **_embeds(), **KW).images
    assert torch.equal(out, want)
    # `latents=` are the noise: moved, not re-drawn -- and the posterior noise is still the generator's first draw
    again = pipe(image=_image(), strength=1.0, latents=noise, generator=torch.Generator().manual_seed(7), **_embeds(), **KW).images
    assert torch.equal(again, want)
    # latents as `image`: no encode, no posterior draw -- the noise is the first draw
    zl = torch.randn(1, 16, 32, 32, generator=torch.Generator().manual_seed(1)).to(bf16)
    g = torch.Generator().manual_seed(9)
    noise = torch.randn(1, 16, 32, 32, generator=g, dtype=bf16)
    lat = pipe(image=zl, strength=1.0, generator=torch.Generator().manual_seed(9), **_embeds(), **KW).images
    assert torch.equal(lat, t2i(latents=FE.pack_latents(noise), height=64, width=64, **_embeds(), **KW).images)


def test_masks_of_ones_and_zeros_and_what_the_callback_sees(emulated):
    img, emb = _image(), _embeds()
    ref = _pipe("img2img")(image=img, strength=0.6, generator=torch.Generator().manual_seed(5), **emb, **KW).images
    pipe = _pipe("inpaint")
    ones = pipe(image=img, mask_image=torch.ones(64, 64), strength=0.6, generator=torch.Generator().manual_seed(5), **emb, **KW).images
    assert torch.equal(ones, ref)
    seen = []
    zeros = pipe(image=img, mask_image=torch.zeros(64, 64), strength=0.6, generator=torch.Generator().manual_seed(5),
                 callback_on_step_end=lambda p, i, t, d: seen.append((i, float(t), d["latents"].clone())) or {}, **emb, **KW).images
    st = pipe._inpaint
    assert torch.equal(zeros, st["image_latents"]) and len(seen) == 3
    assert [t for _, t, _ in seen] == [float(v) for v in pipe.scheduler.timesteps[1:]]
    # mask == 0: after step i the latents are the image latents at the noise level of step i + 1 (rows 2, 3 and the clean last row)
    for (i, _, lat), row in zip(seen, (2, 3, 4)):
        a, b = (float(v) for v in st["table"][row])
        assert torch.equal(lat, FE.I.add_noise(st["image_latents"], st["noise"], a, b) if row < 4 else st["image_latents"]), i
    # a real mask: the callback sees the blend of the step's result, which the reference's expression reproduces from the pieces
    pipe = _pipe("inpaint")
    steps = []
    orig = FluxPipeline._step
    pipe_cls_step = lambda self, lat, pe, cond: steps.append(orig(self, lat, pe, cond).clone()) or lat      # noqa: E731
    seen = []
    import unittest.mock as um
    with um.patch.object(FluxPipeline, "_step", pipe_cls_step):
        pipe(image=img, mask_image=_rect_mask(), strength=0.6, generator=torch.Generator().manual_seed(5),
             callback_on_step_end=lambda p, i, t, d: seen.append(d["latents"].clone()) or {}, **emb, **KW)
    st = pipe._inpaint
    m = st["mask"].reshape(1, 256, 64)
    assert 0 < float(m.float().mean()) < 1
    for i, (raw, got) in enumerate(zip(steps, seen)):
        proper = FE.scale_noise_ref(st["image_latents"], pipe.scheduler.sigmas[i + 2], st["noise"]) if i < 2 else st["image_latents"]
        assert torch.equal(got, FE.blend_ref(m, proper, raw)), i


def test_second_call_refreshes_static_inputs_in_place(emulated):
    pipe = _pipe("inpaint")
    pipe(image=_image(), mask_image=_rect_mask(), strength=0.6, generator=torch.Generator().manual_seed(1), **_embeds(), **KW)
    ptrs = {k: v.data_ptr() for k, v in pipe._inpaint.items()}
    key = pipe._graph_key_extra()
    pipe(image=_image(seed=8), mask_image=1 - _rect_mask(), strength=0.3, generator=torch.Generator().manual_seed(2), **_embeds(), **KW)
    assert ptrs == {k: v.data_ptr() for k, v in pipe._inpaint.items()} and key == pipe._graph_key_extra()
    mlat = F.interpolate((1 - _rect_mask())[None, None], size=(32, 32)).repeat(1, 16, 1, 1)
    assert torch.equal(pipe._inpaint["mask"], FE.pack_latents(mlat).to(bf16).reshape(1, 1, -1))


def test_image_batch_is_repeated_over_the_prompt_batch(emulated):
    pipe = _pipe()
    out = pipe(image=_image(), strength=0.6, generator=torch.Generator().manual_seed(3), **_embeds(2), **KW).images
    assert out.shape == (2, 256, 64) and not torch.equal(out[0], out[1])
    with pytest.raises(ValueError, match="Cannot duplicate `image` of batch size 2 to 3 text prompts"):
        pipe(image=_image(2), **_embeds(3), **KW)


def test_refusals(emulated):
    emb = _embeds()
    pipe, inp = _pipe("img2img"), _pipe("inpaint")
    with pytest.raises(ValueError, match="strength"):
        pipe(image=_image(), strength=1.5, **emb, **KW)
    with pytest.raises(ValueError, match="`image` input cannot be undefined"):
        pipe(**emb, **KW)
    with pytest.raises(ValueError, match="does not resize"):
        pipe(image=_image(), height=128, width=64, **emb, **KW)
    with pytest.raises(ValueError, match="divisible by 4"):
        pipe(image=torch.rand(1, 3, 64, 62), **emb, **KW)
    with pytest.raises(ValueError, match="multiples of the VAE scale factor"):
        pipe(image=torch.rand(1, 3, 64, 63), **emb, **KW)
    with pytest.raises(NotImplementedError, match="true-CFG"):
        pipe(image=_image(), negative_prompt_embeds=emb["prompt_embeds"], **emb, **KW)
    with pytest.raises(ValueError, match="they are taken as the noise"):
        pipe(image=_image(), latents=torch.zeros(1, 256, 64, dtype=bf16), **emb, **KW)
    with pytest.raises(NotImplementedError, match="padding_mask_crop"):
        inp(image=_image(), mask_image=_rect_mask(), padding_mask_crop=32, **emb, **KW)
    with pytest.raises(ValueError, match="`mask_image` input cannot be undefined"):
        inp(image=_image(), **emb, **KW)
    with pytest.raises(ValueError, match="`mask_image` is 32 x 32 but `image` is 64 x 64"):
        inp(image=_image(), mask_image=torch.zeros(32, 32), **emb, **KW)
    with pytest.raises(NotImplementedError, match="masked_image_latents"):
        inp(image=_image(), mask_image=_rect_mask(), masked_image_latents=torch.zeros(1, 256, 64), **emb, **KW)
    inp.transformer.config = type(inp.transformer.config)(dict(inp.transformer.config, in_channels=384))
    with pytest.raises(NotImplementedError, match="Fill checkpoint"):
        inp(image=_image(), mask_image=_rect_mask(), **emb, **KW)
    from diffusers_amd.transformer_flux import FluxTransformer2DModel
    with pytest.raises(ValueError, match="guidance_embeds=True"):          # the dev checkpoints stay refused
        FluxTransformer2DModel(**dict(dinit.TINY_FLUX, guidance_embeds=True))


def test_encode_of_a_16_channel_vae(emulated):
    vae, _ = factory.build_vae(dinit.TINY_FLUX_VAE, seed=6, device="cpu", with_encoder=True)
    x = torch.rand(2, 3, 16, 24, generator=torch.Generator().manual_seed(1)) * 2 - 1
    dist = vae.encode(x).latent_dist
    assert tuple(dist.parameters.shape) == (2, 32, 8, 12) and tuple(dist.mean.shape) == (2, 16, 8, 12)
    assert torch.equal(dist.mode(), dist.mean)
    g = torch.Generator().manual_seed(2)
    z = dist.sample(generator=g)
    eps = torch.randn(2, 16, 8, 12, generator=torch.Generator().manual_seed(2), dtype=torch.float32).to(bf16)
    assert torch.equal(z, dist.latents(eps)) and torch.equal(z, (dist.mean.float() + (dist.std * eps).float()).to(bf16))


def test_exports_factory_and_from_pretrained(emulated, tmp_path):
    import diffusers_amd
    assert diffusers_amd.FluxImg2ImgPipeline is FluxImg2ImgPipeline and diffusers_amd.FluxInpaintPipeline is FluxInpaintPipeline
    assert type(_pipe("img2img")) is FluxImg2ImgPipeline and type(_pipe("inpaint")) is FluxInpaintPipeline
    assert type(factory.build_flux_pipeline(device="cpu", tiny=True)) is FluxPipeline
    assert factory.build_flux_pipeline(device="cpu", tiny=True).vae.encoder is None
    assert factory.build_flux_pipeline(device="cpu", tiny=True, with_encoder=True).vae.encoder is not None
    i2i = inspect.signature(FluxImg2ImgPipeline.__call__).parameters
    inp = inspect.signature(FluxInpaintPipeline.__call__).parameters
    assert i2i["strength"].default == 0.6 and inp["strength"].default == 0.6 and i2i["num_inference_steps"].default == 28
    assert all(k in inp for k in ("image", "mask_image", "padding_mask_crop", "height", "width", "latents", "sigmas"))
    assert list(inspect.signature(FluxImg2ImgPipeline.__init__).parameters) == list(inspect.signature(FluxPipeline.__init__).parameters)
    # a local pipeline directory: model_index.json's _class_name picks the class
    from diffusers_amd.autoencoder_kl import AutoencoderKL
    from diffusers_amd.transformer_flux import FluxTransformer2DModel
    root = tmp_path / "pipe"
    tsd = dinit.random_state_dict(dinit.flux_param_shapes(FluxTransformer2DModel(**dinit.TINY_FLUX).config), seed=5)
    loading.save_reference_checkpoint(tsd, dict(dinit.TINY_FLUX, _class_name="FluxTransformer2DModel"), root / "transformer")
    vcfg = AutoencoderKL(**dinit.TINY_FLUX_VAE).config
    shapes = dinit.vae_decoder_param_shapes(vcfg)
    shapes.update(dinit.vae_encoder_param_shapes(vcfg))
    loading.save_reference_checkpoint(dinit.random_state_dict(shapes, seed=6), dict(dinit.TINY_FLUX_VAE, _class_name="AutoencoderKL"),
                                      root / "vae")
    (root / "scheduler").mkdir(parents=True)
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(_class_name="FlowMatchEulerDiscreteScheduler", shift=1.0)))
    want = _pipe("img2img")
    for name, cls in (("FluxImg2ImgPipeline", FluxImg2ImgPipeline), ("FluxInpaintPipeline", FluxInpaintPipeline)):
        index = {"_class_name": name, "_diffusers_version": "0.40.0", "transformer": ["diffusers", "FluxTransformer2DModel"],
                 "vae": ["diffusers", "AutoencoderKL"], "scheduler": ["diffusers", "FlowMatchEulerDiscreteScheduler"],
                 "text_encoder": [None, None], "text_encoder_2": [None, None], "tokenizer": [None, None], "tokenizer_2": [None, None]}
        (root / "model_index.json").write_text(json.dumps(index))
        pipe = getattr(diffusers_amd, name).from_pretrained(root, device="cpu")
        assert type(pipe) is cls and pipe.vae.encoder is not None and isinstance(pipe.scheduler, FlowMatchEulerDiscreteScheduler)
        with pytest.raises(ValueError, match=f"load it with diffusers_amd.{name}"):
            FluxPipeline.from_pretrained(root, device="cpu")
    extra = dict(mask_image=torch.ones(64, 64))
    a = pipe(image=_image(), generator=torch.Generator().manual_seed(2), **extra, **_embeds(), **KW).images
    b = want(image=_image(), generator=torch.Generator().manual_seed(2), **_embeds(), **KW).images
    assert torch.equal(a, b)
