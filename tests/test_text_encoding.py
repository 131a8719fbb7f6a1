"""Tests that run the LIVE reference (needs /root/reference/src: build container only, skipped elsewhere).

1. Text-encoder front end against the reference pipelines' own ``encode_prompt`` on tiny random
   CLIP / T5 / UMT5 encoders and in-memory tokenizers -- the encoders are the caller's ``transformers`` modules, so only
   the host logic around them is under test.
2. ``from_reference_config`` on real reference objects and their ``state_dict``s.
3. The drop-in boundary: engine models + schedulers registered into the UNCHANGED reference
   SDXL / SD / Flux / Wan pipelines, whose own ``__call__`` drives them (kernels = the torch stand-ins of
   tests/ops_emulation.py; the kernels themselves are tested on the GPU)."""
import sys

import pytest
import torch

from oracle import build_ref

REF = build_ref.SRC.parent
pytestmark = pytest.mark.skipif(not build_ref.reference_present(), reason="reference sources not present")


def _tokenizer(max_len=16):
    from tokenizers import pre_tokenizers
    from transformers import CLIPTokenizer
    alpha = sorted(pre_tokenizers.ByteLevel.alphabet())
    vocab = {}
    for c in alpha:
        vocab[c] = len(vocab)
    for c in alpha:
        vocab[c + "</w>"] = len(vocab)
    merges = [("h", "e"), ("l", "l"), ("he", "ll"), ("hell", "o</w>"), ("c", "a"), ("ca", "t</w>")]
    for a, b in merges:
        vocab[a + b] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    return CLIPTokenizer(vocab=vocab, merges=merges, model_max_length=max_len), len(vocab)


def _clip(vocab, hidden, proj=None, seed=0):
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    torch.manual_seed(seed)
    cfg = CLIPTextConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=3,
                         num_attention_heads=2, max_position_embeddings=16, projection_dim=proj or hidden,
                         bos_token_id=vocab - 2, eos_token_id=vocab - 1, pad_token_id=vocab - 1)
    return (CLIPTextModelWithProjection(cfg) if proj else CLIPTextModel(cfg)).eval()


@pytest.fixture(scope="module")
def ref():
    sys.path.insert(0, str(REF))
    try:
        import diffusers
        yield diffusers
    finally:
        sys.path.remove(str(REF))


def _ref_unet_vae(ref, cross, sdxl):
    kw = dict(addition_embed_type="text_time", addition_time_embed_dim=8, projection_class_embeddings_input_dim=80) if sdxl else {}
    unet = ref.UNet2DConditionModel(block_out_channels=(32, 64), layers_per_block=1, sample_size=8, in_channels=4, out_channels=4,
                                    down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"),
                                    up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"), cross_attention_dim=cross,
                                    attention_head_dim=(2, 4) if sdxl else 8, norm_num_groups=32, **kw)
    vae = ref.AutoencoderKL(block_out_channels=(32, 64), in_channels=3, out_channels=3, latent_channels=4,
                            down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2)
    return unet, vae


@pytest.mark.parametrize("kw", [dict(prompt="hello a cat"), dict(prompt=["hello", "a cat cat"], negative_prompt=["cat", ""]),
                                dict(prompt="a cat", negative_prompt="hello", num_images_per_prompt=2),
                                dict(prompt="hello " * 30, do_classifier_free_guidance=False)])
def test_sd_encode_prompt_matches_reference(ref, kw):
    from diffusers_amd.text_encoding import encode_prompt_sd
    tok, nv = _tokenizer()
    enc = _clip(nv, 32)
    unet, vae = _ref_unet_vae(ref, 32, sdxl=False)
    pipe = ref.StableDiffusionPipeline(vae=vae, text_encoder=enc, tokenizer=tok, unet=unet, scheduler=ref.DDIMScheduler(),
                                       safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    args = dict(num_images_per_prompt=1, do_classifier_free_guidance=True)
    args.update(kw)
    want_p, want_n = pipe.encode_prompt(device="cpu", **args)
    got_p, got_n = encode_prompt_sd(tok, enc, device="cpu", dtype=torch.float32, **args)
    assert torch.equal(got_p, want_p)
    assert (got_n is None and want_n is None) or torch.equal(got_n, want_n)


@pytest.mark.parametrize("kw", [dict(prompt="hello a cat"), dict(prompt="hello", prompt_2="a cat", negative_prompt="cat"),
                                dict(prompt=["hello", "a cat"], negative_prompt=["", "cat"], negative_prompt_2=["hello", ""],
                                     num_images_per_prompt=2),
                                dict(prompt="a cat", clip_skip=1), dict(prompt="a cat", do_classifier_free_guidance=False)])
@pytest.mark.parametrize("force_zeros", [True, False])
def test_sdxl_encode_prompt_matches_reference(ref, kw, force_zeros):
    from diffusers_amd.text_encoding import encode_prompt_sdxl
    tok, nv = _tokenizer()
    tok2, _ = _tokenizer()
    e1, e2 = _clip(nv, 32, seed=1), _clip(nv, 32, proj=32, seed=2)
    unet, vae = _ref_unet_vae(ref, 64, sdxl=True)
    pipe = ref.StableDiffusionXLPipeline(vae=vae, text_encoder=e1, text_encoder_2=e2, tokenizer=tok, tokenizer_2=tok2, unet=unet,
                                         scheduler=ref.EulerDiscreteScheduler(), force_zeros_for_empty_prompt=force_zeros)
    args = dict(num_images_per_prompt=1, do_classifier_free_guidance=True)
    args.update(kw)
    want = pipe.encode_prompt(device="cpu", **args)
    got = encode_prompt_sdxl([tok, tok2], [e1, e2], device="cpu", force_zeros_for_empty_prompt=force_zeros,
                             dtype=torch.float32, **args)
    for g, w in zip(got, want):
        assert (g is None and w is None) or (g.shape == w.shape and torch.equal(g, w))


def test_negative_prompt_errors_match_reference():
    from diffusers_amd.text_encoding import encode_prompt_sd
    tok, nv = _tokenizer()
    enc = _clip(nv, 32)
    with pytest.raises(TypeError):
        encode_prompt_sd(tok, enc, "a cat", "cpu", negative_prompt=["cat"])
    with pytest.raises(ValueError):
        encode_prompt_sd(tok, enc, ["a cat", "hello"], "cpu", negative_prompt=["cat"])


def _t5_tokenizer(max_len=24):
    """In-memory word-level tokenizer with T5's special tokens (<pad> = 0, </s> appended)."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    from transformers import PreTrainedTokenizerFast
    words = ["<pad>", "</s>", "<unk>", "hello", "a", "cat", "on", "the", "mat", "&", "red"]
    tk = Tokenizer(models.WordLevel({w: i for i, w in enumerate(words)}, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    tk.post_processor = processors.TemplateProcessing(single="$A </s>", special_tokens=[("</s>", 1)])
    return PreTrainedTokenizerFast(tokenizer_object=tk, pad_token="<pad>", eos_token="</s>", unk_token="<unk>",
                                   model_max_length=max_len), len(words)


def _t5(vocab, d=32, seed=0, umt5=False):
    from transformers import T5Config, T5EncoderModel, UMT5Config, UMT5EncoderModel
    torch.manual_seed(seed)
    kw = dict(vocab_size=vocab, d_model=d, d_kv=8, d_ff=64, num_layers=2, num_heads=4, relative_attention_num_buckets=8,
              relative_attention_max_distance=16, dropout_rate=0.0, pad_token_id=0, eos_token_id=1)
    return (UMT5EncoderModel(UMT5Config(**kw)) if umt5 else T5EncoderModel(T5Config(**kw))).eval()


@pytest.mark.parametrize("kw", [dict(prompt="hello a cat"), dict(prompt=["hello", "a cat on the mat"], prompt_2=["red cat", "hello"],
                                                                 num_images_per_prompt=2),
                                dict(prompt="a cat", max_sequence_length=8)])
def test_flux_encode_prompt_matches_reference(ref, kw):
    from diffusers_amd.text_encoding import encode_prompt_flux
    tok, nv = _tokenizer()
    tok2, nv2 = _t5_tokenizer()
    clip, t5 = _clip(nv, 32, seed=3), _t5(nv2, seed=4)
    tr = ref.FluxTransformer2DModel(patch_size=1, in_channels=4, num_layers=1, num_single_layers=1, attention_head_dim=16,
                                    num_attention_heads=2, joint_attention_dim=32, pooled_projection_dim=32, axes_dims_rope=[4, 4, 8])
    vae = ref.AutoencoderKL(block_out_channels=(32,), in_channels=3, out_channels=3, latent_channels=1,
                            down_block_types=("DownEncoderBlock2D",), up_block_types=("UpDecoderBlock2D",))
    pipe = ref.FluxPipeline(scheduler=ref.FlowMatchEulerDiscreteScheduler(), vae=vae, text_encoder=clip, tokenizer=tok,
                            text_encoder_2=t5, tokenizer_2=tok2, transformer=tr)
    args = dict(num_images_per_prompt=1, max_sequence_length=16)
    args.update(kw)
    with torch.no_grad():                                   # the reference's __call__ runs under no_grad as well
        want = pipe.encode_prompt(device="cpu", **args)
    got = encode_prompt_flux(tok, clip, tok2, t5, device="cpu", dtype=torch.float32, **args)
    for g_, w_ in zip(got, want):
        assert g_.shape == w_.shape and torch.equal(g_, w_)


@pytest.mark.parametrize("kw", [dict(prompt="hello a cat"), dict(prompt=["hello   a &amp; cat", "a cat on the mat"],
                                                                 negative_prompt=["red", "hello"], num_videos_per_prompt=2),
                                dict(prompt=["a cat", "hello"], negative_prompt="red cat"),
                                dict(prompt="a cat on the mat", do_classifier_free_guidance=False, max_sequence_length=6)])
def test_wan_encode_prompt_matches_reference(ref, kw):
    from diffusers_amd.text_encoding import encode_prompt_wan
    tok, nv = _t5_tokenizer()
    enc = _t5(nv, seed=5, umt5=True)
    tr = ref.WanTransformer3DModel(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=12, in_channels=16,
                                   out_channels=16, text_dim=32, freq_dim=32, ffn_dim=32, num_layers=1, rope_max_seq_len=32)
    vae = ref.AutoencoderKLWan(base_dim=8, z_dim=16, dim_mult=[1, 1, 1, 1], num_res_blocks=1, temperal_downsample=[False, True, True])
    pipe = ref.WanPipeline(tokenizer=tok, text_encoder=enc, vae=vae, scheduler=ref.FlowMatchEulerDiscreteScheduler(shift=3.0),
                           transformer=tr)
    args = dict(do_classifier_free_guidance=True, num_videos_per_prompt=1, max_sequence_length=12)
    args.update(kw)
    with torch.no_grad():
        want_p, want_n = pipe.encode_prompt(device="cpu", dtype=torch.float32, **args)
    got_p, got_n = encode_prompt_wan(tok, enc, device="cpu", dtype=torch.float32, **args)
    assert got_p.shape == want_p.shape and torch.equal(got_p, want_p)
    assert (got_n is None and want_n is None) or torch.equal(got_n, want_n)
    with pytest.raises(ValueError):
        encode_prompt_wan(tok, enc, ["a cat", "hello"], negative_prompt=["red"], device="cpu")


def test_engine_classes_build_from_reference_configs(ref):
    """`from_reference_config(EngineClass, reference_object.config)` for every model class and scheduler, and the packed
    layout the engine builds from the reference module's own state_dict has the inventory the engine expects."""
    import diffusers_amd as da
    from diffusers_amd import init as dinit
    pairs = [
        (da.UNet2DConditionModel, ref.UNet2DConditionModel, dinit.TINY_SDXL_UNET, dinit.unet_param_shapes),
        (da.AutoencoderKL, ref.AutoencoderKL, dinit.TINY_VAE, None),
        (da.FluxTransformer2DModel, ref.FluxTransformer2DModel, dinit.TINY_FLUX, dinit.flux_param_shapes),
        (da.WanTransformer3DModel, ref.WanTransformer3DModel, dinit.TINY_WAN, dinit.wan_param_shapes),
        (da.UNet2DModel, ref.UNet2DModel, dinit.TINY_DDPM, dinit.unet2d_param_shapes),
        (da.AutoencoderKLWan, ref.AutoencoderKLWan, dinit.TINY_WAN_VAE, None),
    ]
    for ours, theirs, cfg, shapes in pairs:
        rm = theirs(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()})
        m = da.from_reference_config(ours, rm.config)
        for k, v in cfg.items():
            got = m.config[k]
            assert (tuple(got) if isinstance(got, (list, tuple)) else got) == (tuple(v) if isinstance(v, (list, tuple)) else v), (ours.__name__, k)
        m.load_state_dict(rm.state_dict(), device="cpu")           # the reference module's own keys / shapes
        if shapes is not None:
            assert {k: tuple(v.shape) for k, v in rm.state_dict().items()} == dict(shapes(dict(m.config)))
    for ours, theirs in [(da.EulerDiscreteScheduler, ref.EulerDiscreteScheduler), (da.DDIMScheduler, ref.DDIMScheduler),
                         (da.DDPMScheduler, ref.DDPMScheduler),
                         (da.FlowMatchEulerDiscreteScheduler, ref.FlowMatchEulerDiscreteScheduler)]:
        rs = theirs()
        s = da.from_reference_config(ours, rs.config)
        for k in s.config:
            assert k in rs.config and (s.config[k] == rs.config[k] or list(s.config[k]) == list(rs.config[k])), (ours.__name__, k)
    # swapping scheduler classes through a foreign config (Euler config -> DDIM), the reference idiom
    assert da.from_reference_config(da.DDIMScheduler, ref.EulerDiscreteScheduler(beta_schedule="scaled_linear").config).config.beta_schedule == "scaled_linear"
    with pytest.raises(TypeError):
        da.from_reference_config(da.AutoencoderKL, dict(ref.AutoencoderKL().config, not_an_option=1))


def test_engine_components_under_the_unchanged_reference_pipeline(ref, monkeypatch):
    """Boundary B1 / B2 / B5: engine UNet + VAE + scheduler registered into the REAL reference
    StableDiffusionXLPipeline, whose own __call__ then drives them (encode_prompt, prepare_latents, scale_model_input,
    unet(...), CFG, scheduler.step, vae.decode, postprocess).  Kernels are the torch stand-ins of tests/ops_emulation.py, so
    this checks the duck-typed surface -- signatures, config attributes, return conventions -- not the kernels."""
    import numpy as np
    import diffusers_amd as da
    import ops_emulation
    from diffusers_amd import init as dinit, ops
    ops_emulation.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "TUNING", False)
    tok, nv = _tokenizer()
    tok2, _ = _tokenizer()
    e1, e2 = _clip(nv, 32, seed=1), _clip(nv, 32, proj=64, seed=2)
    as_lists = lambda c: {k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items()}     # noqa: E731
    torch.manual_seed(0)
    runet = ref.UNet2DConditionModel(**as_lists(dinit.TINY_SDXL_UNET)).eval()
    rvae = ref.AutoencoderKL(**as_lists(dinit.TINY_VAE)).eval()
    rs = ref.EulerDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                                    timestep_spacing="leading")
    pipe = ref.StableDiffusionXLPipeline(vae=rvae, text_encoder=e1, text_encoder_2=e2, tokenizer=tok, tokenizer_2=tok2,
                                         unet=runet, scheduler=rs)
    pipe.set_progress_bar_config(disable=True)
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    kw = dict(prompt="hello a cat", negative_prompt="cat", num_inference_steps=3, guidance_scale=5.0, height=32, width=32,
              output_type="pt")
    want = pipe(latents=lat.clone(), **kw).images                               # the reference, fp32
    pipe.to(torch.bfloat16)                                                     # deployment dtype (text encoders included)
    unet = da.from_reference_config(da.UNet2DConditionModel, runet.config)
    unet.load_state_dict(runet.state_dict(), device="cpu")
    vae = da.from_reference_config(da.AutoencoderKL, rvae.config)
    vae.load_state_dict(rvae.state_dict(), device="cpu")
    pipe.register_modules(unet=unet, vae=vae, scheduler=da.EulerDiscreteScheduler.from_config(rs.config))
    got = pipe(latents=lat.clone().to(torch.bfloat16), **kw).images
    psnr = 10 * np.log10(1.0 / float((got.float() - want).pow(2).mean()))
    print(f"[drop-in] engine under the reference SDXL pipeline: PSNR vs the all-reference fp32 run = {psnr:.1f} dB")
    assert got.shape == want.shape and psnr >= 40.0


def _as_lists(c):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items()}


def _psnr(a, b):
    import numpy as np
    return 10 * np.log10(1.0 / float((a.float() - b.float()).pow(2).mean()))


@pytest.fixture()
def emulated_kernels(monkeypatch):
    import ops_emulation
    from diffusers_amd import ops
    ops_emulation.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "TUNING", False)


def test_engine_under_the_reference_flux_pipeline(ref, emulated_kernels):
    """FluxTransformer2DModel + AutoencoderKL + FlowMatchEuler under the unchanged reference FluxPipeline.__call__
    (its latent packing, image ids, timestep / 1000, shift handling, retrieve_timesteps(sigmas=...))."""
    import diffusers_amd as da
    from diffusers_amd import init as dinit
    tok, nv = _tokenizer()
    tok2, nv2 = _t5_tokenizer()
    torch.manual_seed(0)
    rtr = ref.FluxTransformer2DModel(**_as_lists(dinit.TINY_FLUX)).eval()
    rvae = ref.AutoencoderKL(**_as_lists(dinit.TINY_FLUX_VAE)).eval()
    rs = ref.FlowMatchEulerDiscreteScheduler(shift=1.0, use_dynamic_shifting=False)
    pipe = ref.FluxPipeline(scheduler=rs, vae=rvae, text_encoder=_clip(nv, 64, seed=3), tokenizer=tok,
                            text_encoder_2=_t5(nv2, d=64, seed=4), tokenizer_2=tok2, transformer=rtr)
    pipe.set_progress_bar_config(disable=True)
    lat = torch.randn(1, 64, 64, generator=torch.Generator().manual_seed(1))
    kw = dict(prompt="hello a cat", num_inference_steps=3, guidance_scale=0.0, height=32, width=32, output_type="pt",
              max_sequence_length=16)
    want = pipe(latents=lat.clone(), **kw).images
    pipe.to(torch.bfloat16)
    tr = da.from_reference_config(da.FluxTransformer2DModel, rtr.config)
    tr.load_state_dict(rtr.state_dict(), device="cpu")
    vae = da.from_reference_config(da.AutoencoderKL, rvae.config)
    vae.load_state_dict(rvae.state_dict(), device="cpu")
    pipe.register_modules(transformer=tr, vae=vae, scheduler=da.FlowMatchEulerDiscreteScheduler.from_config(rs.config))
    got = pipe(latents=lat.clone().to(torch.bfloat16), **kw).images
    ps = _psnr(got, want)
    print(f"[drop-in] engine under the reference Flux pipeline: PSNR {ps:.1f} dB")
    assert got.shape == want.shape and ps >= 40.0


def test_engine_under_the_reference_wan_pipeline(ref, emulated_kernels):
    """WanTransformer3DModel + AutoencoderKLWan + UniPC under the unchanged reference WanPipeline.__call__ (two
    transformer calls per step with cache contexts, fp32 latents, latent de-normalisation, video post-processing)."""
    import diffusers_amd as da
    from diffusers_amd import init as dinit
    tok, nv = _t5_tokenizer()
    torch.manual_seed(0)
    rtr = ref.WanTransformer3DModel(**_as_lists(dinit.TINY_WAN)).eval()
    rvae = ref.AutoencoderKLWan(**_as_lists(dinit.TINY_WAN_VAE)).eval()
    rs = ref.UniPCMultistepScheduler(prediction_type="flow_prediction", use_flow_sigmas=True, flow_shift=3.0)
    pipe = ref.WanPipeline(tokenizer=tok, text_encoder=_t5(nv, d=64, seed=5, umt5=True), vae=rvae, scheduler=rs, transformer=rtr)
    pipe.set_progress_bar_config(disable=True)
    lat = torch.randn(1, 16, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    kw = dict(prompt="a cat on the mat", negative_prompt="red", num_inference_steps=3, guidance_scale=5.0, height=64, width=64,
              num_frames=9, output_type="pt", max_sequence_length=16)
    want = pipe(latents=lat.clone(), **kw).frames
    pipe.to(torch.bfloat16)
    tr = da.from_reference_config(da.WanTransformer3DModel, rtr.config)
    tr.load_state_dict(rtr.state_dict(), device="cpu")
    vae = da.from_reference_config(da.AutoencoderKLWan, rvae.config)
    vae.load_state_dict(rvae.state_dict(), device="cpu")
    pipe.register_modules(transformer=tr, vae=vae, scheduler=da.UniPCMultistepScheduler.from_config(rs.config))
    got = pipe(latents=lat.clone(), **kw).frames
    ps = _psnr(got, want)
    print(f"[drop-in] engine under the reference Wan pipeline (UniPC + AutoencoderKLWan): PSNR {ps:.1f} dB")
    assert got.shape == want.shape == (1, 9, 3, 64, 64) and ps >= 40.0


def test_engine_under_the_reference_sd_pipeline(ref, emulated_kernels):
    import diffusers_amd as da
    from diffusers_amd import factory, init as dinit
    tok, nv = _tokenizer()
    torch.manual_seed(0)
    runet = ref.UNet2DConditionModel(**_as_lists(dinit.TINY_SD15_UNET)).eval()
    rvae = ref.AutoencoderKL(**_as_lists(dinit.TINY_VAE)).eval()
    rs = ref.DDIMScheduler(**factory.SD15_SCHEDULER)
    pipe = ref.StableDiffusionPipeline(vae=rvae, text_encoder=_clip(nv, 64, seed=3), tokenizer=tok, unet=runet, scheduler=rs,
                                       safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(2))
    kw = dict(prompt="hello a cat", negative_prompt="cat", num_inference_steps=3, guidance_scale=7.5, height=32, width=32,
              output_type="pt")
    want = pipe(latents=lat.clone(), **kw).images
    pipe.to(torch.bfloat16)
    unet = da.from_reference_config(da.UNet2DConditionModel, runet.config)
    unet.load_state_dict(runet.state_dict(), device="cpu")
    vae = da.from_reference_config(da.AutoencoderKL, rvae.config)
    vae.load_state_dict(rvae.state_dict(), device="cpu")
    pipe.register_modules(unet=unet, vae=vae, scheduler=da.DDIMScheduler.from_config(rs.config))
    got = pipe(latents=lat.clone().to(torch.bfloat16), **kw).images
    ps = _psnr(got, want)
    print(f"[drop-in] engine under the reference SD pipeline (DDIM): PSNR {ps:.1f} dB")
    assert got.shape == want.shape and ps >= 40.0


def test_unet_forward_handles_controlnet_residuals_and_the_encoder_mask(ref, emulated_kernels):
    """Reference-forward arguments beyond the BASELINE call (unet_2d_condition.py:979-994) that the mirror HANDLES:
    ControlNet residuals (:1191-1222), ``encoder_attention_mask`` (:1071-1073) and no-op ``cross_attention_kwargs`` --
    against the live reference U-Net on the same weights; the rest must be refused loudly, never ignored."""
    import diffusers_amd as da
    torch.manual_seed(0)
    from diffusers_amd import init as dinit
    runet = ref.UNet2DConditionModel(**_as_lists(dinit.TINY_SDXL_UNET)).eval()
    unet = da.from_reference_config(da.UNet2DConditionModel, runet.config)
    unet.load_state_dict(runet.state_dict(), device="cpu")
    g = torch.Generator().manual_seed(5)
    B = 2
    sample = torch.randn(B, 4, 16, 16, generator=g)
    ehs = torch.randn(B, 7, 64, generator=g)
    added = {"text_embeds": torch.randn(B, 64, generator=g), "time_ids": torch.tensor([[16., 16., 0., 0., 16., 16.]] * B)}
    t = torch.tensor(500.0)
    mask = torch.tensor([[1, 1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0, 0]])
    with torch.no_grad():
        plain = runet(sample, t, ehs, added_cond_kwargs=added).sample
        # residual shapes = the reference's skip connections (conv_in, each resnet / downsampler output) and the mid block
        shapes = [(B, 64, 16, 16), (B, 64, 16, 16), (B, 64, 8, 8), (B, 128, 8, 8)]
        down = [0.3 * torch.randn(s, generator=g) for s in shapes]
        mid = 0.3 * torch.randn(B, 128, 8, 8, generator=g)
        want_cn = runet(sample, t, ehs, added_cond_kwargs=added, down_block_additional_residuals=tuple(down),
                        mid_block_additional_residual=mid).sample
        want_mask = runet(sample, t, ehs, added_cond_kwargs=added, encoder_attention_mask=mask).sample
    to = lambda x: x.to(torch.bfloat16)  # noqa: E731
    addb = {k: to(v) if k == "text_embeds" else v for k, v in added.items()}

    def rel(a, b):
        return float((a.float() - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
    got_plain = unet(to(sample), t, to(ehs), added_cond_kwargs=addb, cross_attention_kwargs={"scale": 1.0}).sample
    got_cn = unet(to(sample), t, to(ehs), added_cond_kwargs=addb, down_block_additional_residuals=tuple(to(d) for d in down),
                  mid_block_additional_residual=to(mid)).sample
    got_mask = unet(to(sample), t, to(ehs), added_cond_kwargs=addb, encoder_attention_mask=mask).sample
    e0, e1, e2 = rel(got_plain, plain), rel(got_cn, want_cn), rel(got_mask, want_mask)
    print(f"[drop-in] UNet forward extras vs the live reference: plain {e0:.2e}, ControlNet residuals {e1:.2e}, "
          f"encoder_attention_mask {e2:.2e}; the extras move the output by {rel(want_cn, plain):.2e} / {rel(want_mask, plain):.2e}")
    assert max(e0, e1, e2) < 2.5e-2
    assert rel(want_cn, plain) > 10 * e1 and rel(want_mask, plain) > 3 * e2      # the checks above are not vacuous
    for bad in (dict(attention_mask=torch.ones(B, 256)), dict(class_labels=torch.zeros(B)), dict(timestep_cond=torch.zeros(B, 8)),
                dict(cross_attention_kwargs={"scale": 0.5}), dict(cross_attention_kwargs={"gligen": {}}),
                dict(down_block_additional_residuals=tuple(to(d) for d in down)),
                dict(down_block_additional_residuals=tuple(to(d) for d in down[:-1]), mid_block_additional_residual=to(mid)),
                dict(down_intrablock_additional_residuals=[to(down[0])]), dict(encoder_attention_mask=torch.ones(B, 5))):
        with pytest.raises(ValueError):
            unet(to(sample), t, to(ehs), added_cond_kwargs=addb, **bad)
