"""CPU: host side of the InstructPix2Pix pipelines -- exports, class resolution from model_index.json, factory flags, the row order of
the tripled conditioning, the generator's draw order against a literal restatement of the reference's call, the do_cfg rule, the
refusals, the graph key, the pinned C ABI and a host-side model of the 8-channel conv_in's launch geometry.  Kernels are replaced by
the torch stand-ins of tests/pix2pix_emulation.py; no kernel is launched."""
import inspect
import json
import re
from pathlib import Path

import pytest
import torch

import pix2pix_emulation as PE
from test_euler_ancestral_cpu import euler_ancestral_step as euler_ancestral_step_standin

import diffusers_amd
from diffusers_amd import _lib as L
from diffusers_amd import factory, init as dinit, loading, ops
from diffusers_amd.pipelines import (StableDiffusionInstructPix2PixPipeline, StableDiffusionPipeline,
                                     StableDiffusionXLInstructPix2PixPipeline, StableDiffusionXLPipeline)
from diffusers_amd.schedulers import EulerAncestralDiscreteScheduler

bf16 = torch.bfloat16
HEADER = (Path(__file__).resolve().parents[1] / "include" / "diffusers_amd.h").read_text()


@pytest.fixture
def emulated(monkeypatch):
    PE.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "euler_ancestral_step", euler_ancestral_step_standin)
    monkeypatch.setattr(ops, "TUNING", False)


def _pipe(kind, **kw):
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    return build(device="cpu", tiny=True, seed=0, pix2pix=True, **kw)


def _embeds(kind, B=1, seed=3):
    g = torch.Generator().manual_seed(seed)
    pe, npe = (torch.randn(B, 7, 64, generator=g).to(bf16) for _ in range(2))
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=npe)
    if kind == "sdxl":
        te, nte = (torch.randn(B, 64, generator=g).to(bf16) for _ in range(2))
        kw.update(pooled_prompt_embeds=te, negative_pooled_prompt_embeds=nte)
    return kw


def _image(hw=32, seed=4, B=1):
    return torch.rand(B, 3, hw, hw, generator=torch.Generator().manual_seed(seed))


def _stop_before_the_loop(monkeypatch, pipe):
    """Replaces the denoising loop: the call returns its start latents, and what the loop would have got is kept."""
    seen = {}

    def denoise(latents, step_args, num_steps, use_graph, begin=0):
        seen.update(latents=latents.clone(), cond=step_args[0], guidance_scale=step_args[1], do_cfg=step_args[2], num_steps=num_steps,
                    key=pipe._make_graph_key(latents, *step_args))
        return latents
    monkeypatch.setattr(pipe, "_denoise", denoise)
    return seen


# ---- exports, loading, factory ---------------------------------------------------------------------------------------------
def test_exports_defaults_and_factory_flags():
    assert diffusers_amd.StableDiffusionInstructPix2PixPipeline is StableDiffusionInstructPix2PixPipeline
    assert diffusers_amd.StableDiffusionXLInstructPix2PixPipeline is StableDiffusionXLInstructPix2PixPipeline
    assert issubclass(StableDiffusionInstructPix2PixPipeline, StableDiffusionPipeline)
    assert issubclass(StableDiffusionXLInstructPix2PixPipeline, StableDiffusionXLPipeline)
    sd = inspect.signature(StableDiffusionInstructPix2PixPipeline.__call__).parameters
    xl = inspect.signature(StableDiffusionXLInstructPix2PixPipeline.__call__).parameters
    assert sd["num_inference_steps"].default == 100 and sd["guidance_scale"].default == 7.5 and sd["image_guidance_scale"].default == 1.5
    assert xl["num_inference_steps"].default == 100 and xl["guidance_scale"].default == 5.0 and xl["image_guidance_scale"].default == 1.5
    assert "denoising_end" in xl and "denoising_end" not in sd
    for p in (sd, xl):
        assert all(k in p for k in ("image", "latents", "num_images_per_prompt", "callback_on_step_end", "output_type", "use_graph"))
    assert "is_cosxl_edit" in inspect.signature(StableDiffusionXLInstructPix2PixPipeline.__init__).parameters
    for kind, cls in (("sd15", StableDiffusionInstructPix2PixPipeline), ("sdxl", StableDiffusionXLInstructPix2PixPipeline)):
        pipe = _pipe(kind)
        assert type(pipe) is cls and pipe.unet.config.in_channels == 8 and tuple(pipe.unet.conv_in_w.shape) == (64, 72)
        assert pipe.vae.encoder is not None
        for flag in (dict(img2img=True), dict(inpaint=True), dict(controlnet=True), dict(tiny_vae=True)):
            with pytest.raises(ValueError, match="pix2pix=True builds the InstructPix2Pix pipeline"):
                _pipe(kind, **flag)
    assert _pipe("sdxl").is_cosxl_edit is False


@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
def test_model_index_resolves_the_class_and_is_cosxl_edit(kind, tmp_path):
    from diffusers_amd.autoencoder_kl import AutoencoderKL
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    root = tmp_path / "pipe"
    ucfg = dict(dinit.TINY_SDXL_UNET if kind == "sdxl" else dinit.TINY_SD15_UNET, in_channels=8)
    usd = dinit.random_state_dict(dinit.unet_param_shapes(UNet2DConditionModel(**ucfg).config), seed=0)
    loading.save_reference_checkpoint(usd, dict(ucfg, _class_name="UNet2DConditionModel"), root / "unet")
    vcfg = AutoencoderKL(**dinit.TINY_VAE).config
    shapes = dinit.vae_decoder_param_shapes(vcfg)
    shapes.update(dinit.vae_encoder_param_shapes(vcfg))
    loading.save_reference_checkpoint(dinit.random_state_dict(shapes, seed=1), dict(dinit.TINY_VAE, _class_name="AutoencoderKL"), root / "vae")
    (root / "scheduler").mkdir(parents=True)
    sname, scfg = ("EulerDiscreteScheduler", factory.SDXL_SCHEDULER) if kind == "sdxl" else ("DDIMScheduler", factory.SD15_SCHEDULER)
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(scfg, _class_name=sname)))
    name = "StableDiffusionXLInstructPix2PixPipeline" if kind == "sdxl" else "StableDiffusionInstructPix2PixPipeline"
    index = {"_class_name": name, "_diffusers_version": "0.40.0", "unet": ["diffusers", "UNet2DConditionModel"],
             "vae": ["diffusers", "AutoencoderKL"], "scheduler": ["diffusers", sname], "text_encoder": [None, None],
             "tokenizer": [None, None]}
    if kind == "sdxl":
        index.update(text_encoder_2=[None, None], tokenizer_2=[None, None], force_zeros_for_empty_prompt=True, is_cosxl_edit=True)
    else:
        index.update(safety_checker=[None, None], feature_extractor=[None, None], image_encoder=[None, None], requires_safety_checker=False)
    (root / "model_index.json").write_text(json.dumps(index))
    pipe = getattr(diffusers_amd, name).from_pretrained(root, device="cpu")
    assert type(pipe).__name__ == name and pipe.unet.config.in_channels == 8 and pipe.vae.encoder is not None
    if kind == "sdxl":
        assert pipe.is_cosxl_edit is True and pipe._scales_image_latents is True
    base = StableDiffusionXLPipeline if kind == "sdxl" else StableDiffusionPipeline
    with pytest.raises(ValueError, match=f"load it with diffusers_amd.{name}"):
        base.from_pretrained(root, device="cpu")


# ---- conditioning rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
def test_rows_are_text_negative_negative(kind):
    pipe = _pipe(kind)
    e = _embeds(kind, B=2)
    pe, npe = e["prompt_embeds"], e["negative_prompt_embeds"]
    if kind == "sd15":
        rows, added = pipe._conditioning_inputs(pe, npe, True)
        assert added is None
        one, _ = pipe._conditioning_inputs(pe, npe, False)
    else:
        te, nte = e["pooled_prompt_embeds"], e["negative_pooled_prompt_embeds"]
        ids = torch.tensor([[32., 32., 0., 0., 32., 32.]])
        rows, added = pipe._conditioning_inputs(pe, npe, te, nte, ids, ids, True)
        assert torch.equal(added["text_embeds"], torch.cat([te, nte, nte])) and torch.equal(added["time_ids"], ids.repeat(6, 1))
        one, added1 = pipe._conditioning_inputs(pe, npe, te, nte, ids, ids, False)
        assert torch.equal(added1["text_embeds"], te) and torch.equal(added1["time_ids"], ids.repeat(2, 1))
    assert torch.equal(rows, torch.cat([pe, npe, npe])) and torch.equal(one, pe)


# ---- the call: draw order, do_cfg, image latents -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sampler", [("sd15", "ddim"), ("sdxl", "euler"), ("sd15", "euler_a"), ("sdxl", "euler_a")])
def test_draw_order_is_latents_then_step_noise_and_no_draw_for_the_image(emulated, monkeypatch, kind, sampler):
    """Restatement of the reference's call: prepare_image_latents takes the posterior's MODE (no draw), prepare_latents draws
    randn(shape) * init_noise_sigma, and a stochastic scheduler draws one tensor per step inside scheduler.step (EulerAncestral
    draws in every step, the last one with sigma_up = 0 included)."""
    pipe = _pipe(kind)
    if sampler == "euler_a":
        pipe.scheduler = EulerAncestralDiscreteScheduler(**factory.SDXL_SCHEDULER)
    seen = _stop_before_the_loop(monkeypatch, pipe)
    steps, B = 3, 2
    g = torch.Generator().manual_seed(21)
    out = pipe(image=_image(), num_inference_steps=steps, num_images_per_prompt=2, generator=g, output_type="latent",
               **_embeds(kind)).images
    r = torch.Generator().manual_seed(21)
    lat = torch.randn(B, 4, 16, 16, generator=r, dtype=bf16)
    want = (lat.float() * float(pipe.scheduler.init_noise_sigma)).to(bf16)
    assert tuple(out.shape) == (B, 4, 16, 16) and torch.equal(out, want)
    if sampler == "euler_a":
        rows = [torch.randn(B, 4, 16, 16, generator=r, dtype=bf16) for _ in range(steps)]
        assert tuple(pipe._noise_table.shape) == (steps, B, 4, 16, 16)
        for i, row in enumerate(rows):
            assert torch.equal(pipe._noise_table[i], row), i
    else:
        assert pipe._noise_table is None
    assert torch.equal(g.get_state(), r.get_state()), "the call drew something the restatement does not"
    # the image latents: the mode of the posterior, NOT multiplied by scaling_factor, one row broadcast over the batch
    il = pipe._pix2pix["image_latents"]
    mode = pipe.vae.encode_image(_image().contiguous(), nchw=True, normalize=True).mode()
    assert tuple(il.shape) == (1, 4, 16, 16) and torch.equal(il, mode)
    assert seen["cond"]["batch"] == 3 * B and seen["do_cfg"] is True and seen["num_steps"] == steps


def test_cosxl_edit_scales_the_image_latents_once(emulated, monkeypatch):
    plain, cosxl = _pipe("sdxl"), _pipe("sdxl")
    cosxl.is_cosxl_edit = cosxl._scales_image_latents = True
    for p in (plain, cosxl):
        _stop_before_the_loop(monkeypatch, p)
        p(image=_image(), num_inference_steps=2, output_type="latent", generator=torch.Generator().manual_seed(1), **_embeds("sdxl"))
    sf = float(plain.vae.config.scaling_factor)
    assert sf != 1.0
    assert torch.equal(cosxl._pix2pix["image_latents"], plain._pix2pix["image_latents"] * sf)
    ctor = StableDiffusionXLInstructPix2PixPipeline(vae=plain.vae, unet=plain.unet, scheduler=plain.scheduler, is_cosxl_edit=True)
    assert ctor._scales_image_latents is True


@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
@pytest.mark.parametrize("gs,igs,want", [(7.5, 1.5, True), (1.0, 1.5, False), (7.5, 0.9, False)])
def test_do_cfg_rule(emulated, monkeypatch, kind, gs, igs, want):
    pipe = _pipe(kind)
    seen = _stop_before_the_loop(monkeypatch, pipe)
    pipe(image=_image(), num_inference_steps=2, guidance_scale=gs, image_guidance_scale=igs, output_type="latent", **_embeds(kind))
    assert seen["do_cfg"] is want and seen["cond"]["batch"] == (3 if want else 1)


def test_latents_argument_and_image_batch(emulated, monkeypatch):
    pipe = _pipe("sd15")
    _stop_before_the_loop(monkeypatch, pipe)
    mine = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(8)).to(bf16)
    g = torch.Generator().manual_seed(5)
    state = g.get_state()
    out = pipe(image=_image(B=2), latents=mine, num_inference_steps=2, generator=g, output_type="latent", **_embeds("sd15", B=2)).images
    assert torch.equal(out, (mine.float() * float(pipe.scheduler.init_noise_sigma)).to(bf16)) and torch.equal(g.get_state(), state)
    assert tuple(pipe._pix2pix["image_latents"].shape) == (2, 4, 16, 16)
    # `image` given as latents is taken as it is
    lat_img = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(9)).to(bf16)
    pipe(image=lat_img, num_inference_steps=2, output_type="latent", **_embeds("sd15"))
    assert torch.equal(pipe._pix2pix["image_latents"], lat_img)
    with pytest.raises(ValueError, match="Cannot duplicate `image` of batch size 2 to 3 text prompts"):
        pipe(image=_image(B=2), num_inference_steps=2, num_images_per_prompt=3, output_type="latent", **_embeds("sd15"))


# ---- a whole call on the stand-ins against a hand-written loop -------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
def test_whole_call_equals_the_concatenating_loop(emulated, kind):
    pipe = _pipe(kind)
    steps, gs, igs = 3, 7.5, 1.5
    e = _embeds(kind)
    seen = []
    out = pipe(image=_image(), num_inference_steps=steps, guidance_scale=gs, image_guidance_scale=igs, output_type="latent",
               generator=torch.Generator().manual_seed(21), use_graph=False,
               callback_on_step_end=lambda p, i, t, d: seen.append(int(i)) or {}, **e).images.clone()
    assert seen == list(range(steps))
    # the reference's loop over the same components: cat x3, scale, cat with [img, img, 0] on dim 1, the ordinary conv_in
    sch = pipe.scheduler
    sch.set_timesteps(steps, device="cpu")
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(21), dtype=bf16)
    lat = ops.mul_scalar(lat, float(sch.init_noise_sigma))
    img = pipe.vae.encode_image(_image().contiguous(), nchw=True, normalize=True).mode()
    if kind == "sdxl":
        ids = torch.tensor([[32., 32., 0., 0., 32., 32.]])
        cond = pipe._conditioning(e["prompt_embeds"], e["negative_prompt_embeds"], e["pooled_prompt_embeds"],
                                  e["negative_pooled_prompt_embeds"], ids, ids, True)
    else:
        cond = pipe._conditioning(e["prompt_embeds"], e["negative_prompt_embeds"], True)
    sch.reset(0)
    for _ in range(steps):
        x3 = sch.scale_model_input(lat, sch.timesteps[0], rep=3) if sch.scales_model_input else torch.cat([lat] * 3)
        xin = torch.cat([x3, torch.cat([img, img, torch.zeros_like(img)])], dim=1).contiguous()
        eps = pipe.unet(xin, None, None, conditioning=cond, sampler_table=sch.device_table, step_idx=sch.device_step, return_dict=False)[0]
        t, i, u = (c.float() for c in eps.chunk(3))

        def r(v):
            return v.to(bf16).float()
        comb = r(r(u + r(gs * r(t - i))) + r(igs * r(i - u))).to(bf16)
        sch.step_cfg(comb, lat, gs, out=lat, cfg=False)
    assert torch.isfinite(out.float()).all() and torch.equal(out, lat)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
def test_refusals_by_name(emulated, kind):
    pipe = _pipe(kind)
    kw = dict(image=_image(), num_inference_steps=2, output_type="latent", **_embeds(kind))
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        pipe(guidance_rescale=0.7, **kw)
    with pytest.raises(NotImplementedError, match="ip_adapter_image"):
        pipe(ip_adapter_image=_image(), **kw)
    with pytest.raises(NotImplementedError, match="ip_adapter_image"):
        pipe(ip_adapter_image_embeds=[torch.zeros(1, 1, 8)], **kw)
    with pytest.raises(NotImplementedError, match="padding_mask_crop"):
        pipe(padding_mask_crop=32, **kw)
    with pytest.raises(ValueError, match="does not resize"):
        pipe(height=64, width=64, **kw)
    with pytest.raises(ValueError, match="31 x 32"):
        pipe(**dict(kw, image=_image()[:, :, :31]))
    with pytest.raises(ValueError, match="`image` input cannot be undefined"):
        pipe(**dict(kw, image=None))
    with pytest.raises(NotImplementedError, match="ControlNet"):
        type(pipe)(vae=pipe.vae, unet=pipe.unet, scheduler=pipe.scheduler, controlnet=object())
    # AutoencoderTiny: no posterior
    tiny = type(pipe)(vae=pipe.vae, unet=pipe.unet, scheduler=pipe.scheduler)
    tiny.vae = type("AutoencoderTiny", (), {"config": pipe.vae.config})()
    with pytest.raises(NotImplementedError, match="AutoencoderTiny has no posterior"):
        tiny(**kw)
    # a U-Net with time_cond_proj_dim
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    lcm = build(device="cpu", tiny=True, seed=0, pix2pix=True, time_cond_proj_dim=32)
    with pytest.raises(NotImplementedError, match="time_cond_proj_dim"):
        lcm(**kw)


@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
def test_channel_count_refusal_message(emulated, kind):
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    four = build(device="cpu", tiny=True, seed=0, with_encoder=True)            # an ordinary 4-channel U-Net in the pix2pix class
    pipe = type(_pipe(kind))(vae=four.vae, unet=four.unet, scheduler=four.scheduler)
    with pytest.raises(ValueError, match=r"Incorrect configuration settings! The config of `pipeline.unet`: .* expects 4 but received "
                                         r"`num_channels_latents`: 4 \+ `num_channels_image`: 4  = 8\. Please verify the config of "
                                         r"`pipeline.unet` or your `image` input\."):
        pipe(image=_image(), num_inference_steps=2, output_type="latent", **_embeds(kind))


def test_unet_image_cond_checks(emulated):
    pipe = _pipe("sd15")
    cond = pipe.unet.precompute_conditioning(torch.zeros(2, 7, 64, dtype=bf16), None)
    x, img = torch.zeros(1, 4, 16, 16, dtype=bf16), torch.zeros(1, 4, 16, 16, dtype=bf16)
    with pytest.raises(ValueError, match="three times"):
        pipe.unet(x, torch.tensor(1.0), None, conditioning=cond, image_cond=img)
    with pytest.raises(ValueError, match="exclude each other"):
        pipe.unet(x, torch.tensor(1.0), None, conditioning=cond, image_cond=img, inpaint_cond=(img[:, :1], img))
    with pytest.raises(ValueError, match="sampler table"):
        pipe.unet(x, torch.tensor(1.0), None, conditioning=cond, image_cond=img, scale_model_input=True)
    four = factory.build_sd15_pipeline(device="cpu", tiny=True, seed=0)
    c4 = four.unet.precompute_conditioning(torch.zeros(1, 7, 64, dtype=bf16), None)
    with pytest.raises(ValueError, match="8 input channels"):
        four.unet(x, torch.tensor(1.0), None, conditioning=c4, image_cond=img)
    # an 8-channel sample without image_cond: the ordinary conv_in, equal to the two-source form
    c1 = pipe.unet.precompute_conditioning(torch.zeros(1, 7, 64, dtype=bf16), None)
    g = torch.Generator().manual_seed(2)
    x, img = (torch.randn(1, 4, 16, 16, generator=g).to(bf16) for _ in range(2))
    a = pipe.unet(torch.cat([x, img], 1), torch.tensor(5.0), None, conditioning=c1).sample
    b = pipe.unet(x, torch.tensor(5.0), None, conditioning=c1, image_cond=img).sample
    assert torch.equal(a, b)


# ---- graph key -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
def test_graph_key_follows_image_guidance_scale_not_the_image(emulated, monkeypatch, kind):
    pipe = _pipe(kind)
    seen = _stop_before_the_loop(monkeypatch, pipe)
    keys = []
    for img, igs in ((_image(seed=4), 1.5), (_image(seed=5), 1.5), (_image(seed=5), 1.25)):
        lat = torch.zeros(1, 4, 16, 16, dtype=bf16)          # (one latents buffer shape; its address is not part of the key)
        pipe(image=img, latents=lat, num_inference_steps=2, image_guidance_scale=igs, output_type="latent", **_embeds(kind))
        keys.append(seen["key"])
    ptr = pipe._pix2pix["image_latents"].data_ptr()
    assert keys[0] == keys[1], "another image of the same size must reuse the captured step (buffer refreshed in place)"
    assert keys[1] != keys[2], "image_guidance_scale is baked into the captured combine: it must be part of the key"
    assert any(isinstance(k, tuple) and k[:1] == ("image_latents",) and k[1] == ptr and k[2] == (1, 4, 16, 16) for k in keys[0])
    assert 1.5 in keys[0] and 1.25 in keys[2]
    mode5 = pipe.vae.encode_image(_image(seed=5).contiguous(), nchw=True, normalize=True).mode()
    assert torch.equal(pipe._pix2pix["image_latents"], mode5)
    # another size: a new buffer, another key
    pipe(image=_image(hw=64), num_inference_steps=2, output_type="latent", **_embeds(kind))
    assert seen["key"] != keys[0] and tuple(pipe._pix2pix["image_latents"].shape) == (1, 4, 32, 32)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
FN_IDS_PINNED = {
    "da_gemm_bf16": 1, "da_gemm_pair_bf16": 2, "da_attention_bf16": 3, "da_groupnorm_nhwc_bf16": 4, "da_rmsnorm_bf16": 5,
    "da_layernorm_bf16": 6, "da_rmsnorm_rope_bf16": 7, "da_softmax_rows_f32_bf16": 8, "da_rmsnorm_channels_bf16": 9,
    "da_euler_scale_model_input": 10, "da_euler_step": 11, "da_x0_linear_step": 12, "da_flowmatch_step": 13, "da_unipc_flow_step": 14,
    "da_advance_step": 15, "da_cfg_rescale": 16, "da_cast_f32_bf16": 17, "da_mul_scalar": 18, "da_bcast_add_f32": 19,
    "da_patchify3d_bf16": 20, "da_unpatchify3d_bf16": 21, "da_transpose_bf16": 22, "da_nhwc_take_nchw_bf16": 23,
    "da_nhwc_take_postprocess": 24, "da_permute_0213_bf16": 25, "da_image_postprocess": 26, "da_frames_to_ncthw_bf16": 27,
    "da_timestep_embedding": 28, "da_linear_small_m_bf16": 29, "da_conv_thin_in_bf16": 30, "da_conv_thin_out_bf16": 31,
    "da_inpaint_blend": 32, "da_conv_in_inpaint": 33, "da_euler_ancestral_step": 34, "da_dpmpp_2m_step": 35}


def test_abi_is_unchanged_and_the_flag_is_declared():
    assert re.search(r"^#define DA_ABI_VERSION 9\b", HEADER, re.M) and L.ABI_VERSION == 9 and L.FN_COUNT == 36
    assert dict(L.FN_IDS) == FN_IDS_PINNED
    assert re.search(r"^#define DA_CFG_IMAGE_GUIDANCE 0x100\b", HEADER, re.M) and L.CFG_IMAGE_GUIDANCE == 0x100
    assert L.CFG_IMAGE_GUIDANCE & (L.DTYPE_BF16 | L.DTYPE_F32) == 0
    _i, _f, _ll, _vp = L._i, L._f, L._ll, L._vp
    assert L.SIGNATURES["da_cfg_rescale"] == (_i, [_vp, _vp, _vp, _i, _ll, _f, _f, _i, _vp])
    assert L.SIGNATURES["da_conv_in_inpaint"] == (_i, [_vp] * 8 + [_i] * 6 + [_vp])
    assert L.NOT_PLANNABLE == ("da_vae_conv_in_image", "da_vae_posterior_latents", "da_flux_prepare_latents")
    assert not [n for n in L.SIGNATURES if "pix2pix" in n or "combine3" in n], "no new exported entry point"


# ---- launch geometry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 3, 5, 64), (1, 17, 30, 320)])
def test_chunks_and_grid_for_kk_72_cover_every_output_once(shape):
    B, H, W, Cout = shape
    coc, nchunk, blocks, cover = PE.conv_in_launch_model(B, H, W, Cout, kk=72)
    assert coc == min(224, Cout) and coc % 8 == 0 and coc * 72 * 4 <= 64 * 1024
    assert nchunk == (2 if Cout == 320 else 1) and 1 <= blocks <= 768 // nchunk
    if Cout == 320:
        assert (coc, Cout - coc) == (224, 96)
    assert int(cover.min()) == 1 and int(cover.max()) == 1
    # the 9-channel form keeps its own chunking
    assert PE.conv_in_launch_model(1, 1, 1, 320, kk=81)[:2] == (200, 2)
