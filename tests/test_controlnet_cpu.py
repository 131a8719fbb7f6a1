"""CPU: ControlNetModel and the two ControlNet pipelines on the torch stand-ins of tests/controlnet_emulation.py -- the state_dict
inventory and the refusals, ``forward`` against a plain torch restatement of the reference module (fp32 oracle, bf16 floor), and
the pipelines' host logic (image checks, batching, refusals, the capture key).  No kernel is launched."""
import math

import numpy as np
import pytest
import torch

import controlnet_emulation as CE
import diffusers_amd as da
from diffusers_amd import factory, init as dinit, ops
from diffusers_amd.pipelines import control_image_batch, prepare_control_image

bf16 = torch.bfloat16


@pytest.fixture
def emulated(monkeypatch):
    CE.install(monkeypatch, ops)


# ---- 1. inventory and config ---------------------------------------------------------------------------------------------
def _restated_inventory(cfg):
    """The reference constructor's parameters (controlnet.py ``__init__``), restated: name -> shape."""
    sh = {}

    def conv(p, co, ci, k):
        sh[p + ".weight"], sh[p + ".bias"] = (co, ci, k, k), (co,)

    def lin(p, co, ci, bias=True):
        sh[p + ".weight"] = (co, ci)
        if bias:
            sh[p + ".bias"] = (co,)

    def norm(p, c):
        sh[p + ".weight"], sh[p + ".bias"] = (c,), (c,)

    def resnet(p, ci, co, temb):
        norm(p + ".norm1", ci), conv(p + ".conv1", co, ci, 3), lin(p + ".time_emb_proj", co, temb)
        norm(p + ".norm2", co), conv(p + ".conv2", co, co, 3)
        if ci != co:
            conv(p + ".conv_shortcut", co, ci, 1)

    def transformer(p, c, cross, layers, linear):
        norm(p + ".norm", c)
        for q in (".proj_in", ".proj_out"):
            lin(p + q, c, c) if linear else conv(p + q, c, c, 1)
        for k in range(layers):
            b = f"{p}.transformer_blocks.{k}"
            for nm in ("norm1", "norm2", "norm3"):
                norm(f"{b}.{nm}", c)
            for a, kd in (("attn1", c), ("attn2", cross)):
                lin(f"{b}.{a}.to_q", c, c, False), lin(f"{b}.{a}.to_k", c, kd, False), lin(f"{b}.{a}.to_v", c, kd, False)
                lin(f"{b}.{a}.to_out.0", c, c)
            lin(f"{b}.ff.net.0.proj", 8 * c, c), lin(f"{b}.ff.net.2", c, 4 * c)

    boc = cfg["block_out_channels"]
    n, temb = len(boc), 4 * boc[0]
    tl = cfg["transformer_layers_per_block"]
    tl = tl if isinstance(tl, tuple) else (tl,) * n
    conv("conv_in", boc[0], 4, 3)
    lin("time_embedding.linear_1", temb, boc[0]), lin("time_embedding.linear_2", temb, temb)
    if cfg["addition_embed_type"] == "text_time":
        lin("add_embedding.linear_1", temb, cfg["projection_class_embeddings_input_dim"]), lin("add_embedding.linear_2", temb, temb)
    emb = cfg["conditioning_embedding_out_channels"]
    conv("controlnet_cond_embedding.conv_in", emb[0], 3, 3)
    for i in range(len(emb) - 1):
        conv(f"controlnet_cond_embedding.blocks.{2 * i}", emb[i], emb[i], 3)
        conv(f"controlnet_cond_embedding.blocks.{2 * i + 1}", emb[i + 1], emb[i], 3)
    conv("controlnet_cond_embedding.conv_out", boc[0], emb[-1], 3)
    zero, prev = [boc[0]], boc[0]
    for i, bt in enumerate(cfg["down_block_types"]):
        for j in range(cfg["layers_per_block"]):
            resnet(f"down_blocks.{i}.resnets.{j}", prev if j == 0 else boc[i], boc[i], temb)
            if bt == "CrossAttnDownBlock2D":
                transformer(f"down_blocks.{i}.attentions.{j}", boc[i], cfg["cross_attention_dim"], tl[i], cfg["use_linear_projection"])
            zero.append(boc[i])
        if i != n - 1:
            conv(f"down_blocks.{i}.downsamplers.0.conv", boc[i], boc[i], 3)
            zero.append(boc[i])
        prev = boc[i]
    resnet("mid_block.resnets.0", boc[-1], boc[-1], temb), resnet("mid_block.resnets.1", boc[-1], boc[-1], temb)
    transformer("mid_block.attentions.0", boc[-1], cfg["cross_attention_dim"], tl[-1], cfg["use_linear_projection"])
    for k, c in enumerate(zero):
        conv(f"controlnet_down_blocks.{k}", c, c, 1)
    conv("controlnet_mid_block", boc[-1], boc[-1], 1)
    return sh


@pytest.mark.parametrize("name,n_zero,params", [("TINY_SD15_CONTROLNET", 4, None), ("TINY_SDXL_CONTROLNET", 4, None),
                                                ("SD15_CONTROLNET", 12, 361_279_120), ("SDXL_CONTROLNET", 9, 1_251_014_160)])
def test_state_dict_inventory(name, n_zero, params):
    cn = da.ControlNetModel(**getattr(dinit, name))
    got = dict(dinit.controlnet_param_shapes(cn.config))
    assert got == _restated_inventory(dict(cn.config))
    assert sum(k.startswith("controlnet_down_blocks.") and k.endswith(".weight") for k in got) == n_zero
    if params is not None:      # the published sizes of lllyasviel/sd-controlnet-* (361 M) and diffusers/controlnet-*-sdxl-1.0 (1.25 B)
        assert sum(math.prod(s) for s in got.values()) == params
    assert got["controlnet_cond_embedding.conv_out.weight"][0] == cn.config.block_out_channels[0]


def test_config_defaults_and_refusals():
    c = da.ControlNetModel().config
    assert c.conditioning_embedding_out_channels == (16, 32, 96, 256) and c.block_out_channels == (320, 640, 1280, 1280)
    assert c.controlnet_conditioning_channel_order == "rgb" and c.global_pool_conditions is False and c.cross_attention_dim == 1280
    assert da.ControlNetModel().conditioning_scale_factor == 8
    assert da.ControlNetModel(**dinit.TINY_SD15_CONTROLNET).conditioning_scale_factor == 2
    with pytest.raises(TypeError, match="unexpected config keys .*up_block_types"):
        da.ControlNetModel(up_block_types=("UpBlock2D",))
    with pytest.raises(ValueError, match="class_embed_type"):
        da.ControlNetModel(class_embed_type="timestep")
    with pytest.raises(NotImplementedError, match="global_pool_conditions"):
        da.ControlNetModel(global_pool_conditions=True)
    with pytest.raises(ValueError, match="addition_embed_type='text'"):
        da.ControlNetModel(addition_embed_type="text")
    with pytest.raises(ValueError, match="conditioning_channels=1"):
        da.ControlNetModel(conditioning_channels=1)
    cn = da.from_reference_config(da.ControlNetModel, dict(dinit.TINY_SD15_CONTROLNET, _class_name="ControlNetModel",
                                                           block_out_channels=[64, 128]))
    assert cn.config.block_out_channels == (64, 128)


# ---- 2. forward against the restatement ------------------------------------------------------------------------------------
def _case(flavour, seed=0):
    ucfg = dinit.TINY_SDXL_UNET if flavour == "sdxl" else dinit.TINY_SD15_UNET
    cn, sd = factory.build_controlnet(ucfg, seed=3, device="cpu", conditioning_embedding_out_channels=(16, 32))
    g = torch.Generator().manual_seed(seed)
    sample = torch.randn(2, 4, 16, 16, generator=g).to(bf16)
    ehs = torch.randn(2, 7, 64, generator=g).to(bf16)
    image = torch.rand(2, 3, 32, 32, generator=g).to(bf16).float()        # pixels the bf16 cast keeps exactly
    added = None
    if flavour == "sdxl":
        added = {"text_embeds": torch.randn(2, 64, generator=g).to(bf16),
                 "time_ids": torch.tensor([[32., 32., 0., 0., 32., 32.]]).repeat(2, 1)}
    return cn, sd, ucfg, sample, ehs, image, added


def _restated(sd, cfg, dtype, sample, ehs, image, added, scale):
    ad = None if added is None else {"text_embeds": added["text_embeds"].to(dtype), "time_ids": added["time_ids"]}
    down, mid = CE.controlnet_forward(CE.cast(sd, dtype), cfg, sample.to(dtype), 801.0, ehs.to(dtype), image.to(dtype), scale, ad)
    return down + [mid]


@pytest.mark.parametrize("flavour", ["sd15", "sdxl"])
def test_forward_against_the_restatement(emulated, flavour):
    """Every residual within 1.5 x the error the SAME restatement makes in bf16 on the CPU (the floor of the number format; the
    margin covers another summation order of K), and the residuals matter: on the fp32 restatement they move the U-Net's output
    by more than 10 x that error."""
    cn, sd, ucfg, sample, ehs, image, added = _case(flavour)
    cfg, scale = dict(cn.config), 0.7
    ref = _restated(sd, cfg, torch.float32, sample, ehs, image, added, scale)
    low = _restated(sd, cfg, bf16, sample, ehs, image, added, scale)
    out = cn(sample, 801.0, ehs, image, conditioning_scale=scale, added_cond_kwargs=added)
    got = list(out.down_block_res_samples) + [out.mid_block_res_sample]
    assert len(got) == len(ref) == 5 and all(g.dtype == bf16 and g.shape == r.shape for g, r in zip(got, ref))
    worst = 0.0
    for k, (g, lo, r) in enumerate(zip(got, low, ref)):
        floor, err = CE.rel_rms(lo, r), CE.rel_rms(g, r)
        print(f"[controlnet cpu {flavour}] residual {k}: engine path {err:.3e}, bf16 restatement (floor) {floor:.3e}")
        assert err <= 1.5 * floor, (k, err, floor)
        worst = max(worst, err, floor)
    unet, usd = factory.build_unet(ucfg, seed=0, device="cpu")
    ucfg_full, f32 = dict(unet.config), CE.cast(usd, torch.float32)
    ad = None if added is None else {"text_embeds": added["text_embeds"].float(), "time_ids": added["time_ids"]}
    base = CE.unet_forward(f32, ucfg_full, sample.float(), 801.0, ehs.float(), ad)
    moved = CE.unet_forward(f32, ucfg_full, sample.float(), 801.0, ehs.float(), ad, ref[:-1], ref[-1])
    effect = CE.rel_rms(moved, base)
    print(f"[controlnet cpu {flavour}] the residuals move the U-Net output by {effect:.3e} (worst error {worst:.3e})")
    assert effect > 10 * worst
    # the engine U-Net's NCHW residual path and its hand-off hook add the same residuals
    cond = unet.precompute_conditioning(ehs, added)
    a = unet(sample, 801.0, None, conditioning=cond, down_block_additional_residuals=got[:-1], mid_block_additional_residual=got[-1]).sample
    ccn = cn.precompute_conditioning(ehs, added, image, conditioning_scale=scale)
    feats = cn.features(sample, ccn, timestep=801.0)
    b = unet(sample, 801.0, None, conditioning=cond, controlnet_handoff=cn.handoff(feats, ccn["gate"])).sample
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="controlnet_handoff"):
        unet(sample, 801.0, None, conditioning=cond, down_block_additional_residuals=got[:-1], mid_block_additional_residual=got[-1],
             controlnet_handoff=lambda s, m: None)


def test_forward_refusals_and_image_forms(emulated):
    cn, sd, ucfg, sample, ehs, image, added = _case("sd15")
    with pytest.raises(NotImplementedError, match="guess_mode"):
        cn(sample, 801.0, ehs, image, guess_mode=True)
    with pytest.raises(ValueError, match="class_labels"):
        cn(sample, 801.0, ehs, image, class_labels=torch.zeros(2))
    with pytest.raises(ValueError, match="the image must be 2 x the latents' size"):
        cn(sample, 801.0, ehs, image[:, :, :16, :16])
    with pytest.raises(ValueError, match="4 channels, 3 expected"):
        cn(sample, 801.0, ehs, torch.zeros(2, 4, 32, 32))
    # uint8 NHWC pixels, fp32 NHWC, fp32 NCHW and bf16 NCHW of the same image give the same residuals; the embedding's padding
    # channels are zero
    u8 = (torch.rand(2, 32, 32, 3, generator=torch.Generator().manual_seed(1)) * 255).to(torch.uint8)
    f_nhwc = u8.float() / 255.0
    outs = [cn(sample, 801.0, ehs, im, return_dict=False)[1] for im in
            (u8, f_nhwc, f_nhwc.permute(0, 3, 1, 2).contiguous(), f_nhwc.permute(0, 3, 1, 2).contiguous().to(bf16))]
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    emb = cn.precompute_conditioning(ehs, None, u8)["embed"]
    assert tuple(emb.shape) == (2, 16, 16, 64) and emb[..., :32].abs().sum() > 0 and not emb[..., 32:].any()
    # scale 0: the hand-off leaves its targets as they are
    cond = cn.precompute_conditioning(ehs, None, u8, conditioning_scale=0.0)
    feats = cn.features(sample, cond, timestep=801.0)
    tg = [torch.randn_like(f) for f in feats]
    keep = [t.clone() for t in tg]
    cn.handoff_(tg[:-1], tg[-1], feats, cond["gate"])
    assert all(torch.equal(a, b) for a, b in zip(tg, keep))


# ---- 3. pipeline host logic ------------------------------------------------------------------------------------------------
def _pipe(flavour, **kw):
    build = factory.build_sdxl_pipeline if flavour == "sdxl" else factory.build_sd15_pipeline
    return build(device="cpu", tiny=True, controlnet=True, **kw)


def _call_kw(flavour, n=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    kw = dict(prompt_embeds=torch.randn(n, 7, 64, generator=g).to(bf16), negative_prompt_embeds=torch.randn(n, 7, 64, generator=g).to(bf16),
              num_inference_steps=2, output_type="latent")
    if flavour == "sdxl":
        kw.update(pooled_prompt_embeds=torch.randn(n, 64, generator=g).to(bf16),
                  negative_pooled_prompt_embeds=torch.randn(n, 64, generator=g).to(bf16))
    return kw


def _spy(pipe):
    seen = {}

    def denoise(latents, step_args, num_steps, use_graph, begin=0):
        seen.update(latents=latents, cond=step_args[0], key=pipe._make_graph_key(latents, *step_args))
        return latents
    pipe._denoise = denoise
    return seen


def test_control_image_forms_and_messages():
    img = torch.rand(1, 3, 32, 48)
    t, nchw = prepare_control_image(img, 2, "cpu")
    assert nchw and t.dtype == torch.float32 and torch.equal(t, img)              # not normalised to [-1, 1], not resized
    assert prepare_control_image(img[0], 2, "cpu")[0].shape == (1, 3, 32, 48)
    u8 = (img[0].permute(1, 2, 0) * 255).to(torch.uint8).numpy()
    t, nchw = prepare_control_image(u8, 2, "cpu")
    assert not nchw and t.dtype == torch.uint8 and tuple(t.shape) == (1, 32, 48, 3)
    t, nchw = prepare_control_image(u8.astype(np.float64) / 255, 2, "cpu")
    assert not nchw and t.dtype == torch.float32
    Image = pytest.importorskip("PIL.Image")
    t, nchw = prepare_control_image(Image.fromarray(u8), 2, "cpu")
    assert not nchw and torch.equal(t[0], torch.from_numpy(u8))
    with pytest.raises(ValueError, match=r"`image` is 31 x 48: height and width must be multiples of the VAE scale factor 2 "
                                         r"\(the engine does not resize images\)"):
        prepare_control_image(img[:, :, :31], 2, "cpu")
    with pytest.raises(NotImplementedError, match="`image` as a list"):
        prepare_control_image([img, img], 2, "cpu")
    with pytest.raises(ValueError, match="3 channels"):
        prepare_control_image(torch.zeros(1, 4, 32, 32), 2, "cpu")
    with pytest.raises(ValueError, match="has to be of type"):
        prepare_control_image("edges.png", 2, "cpu")
    with pytest.raises(ValueError, match="required"):
        prepare_control_image(None, 2, "cpu")


def test_control_image_batching():
    a, b = torch.full((1, 3, 2, 2), 1.0), torch.full((1, 3, 2, 2), 2.0)
    one = control_image_batch(a, 3, 3, True)
    assert one.shape[0] == 6 and torch.equal(one, a.expand(6, -1, -1, -1))
    two = control_image_batch(torch.cat([a, b]), 4, 2, True)          # repeat_interleave per prompt, then the CFG doubling
    assert [float(x[0, 0, 0]) for x in two] == [1, 1, 2, 2, 1, 1, 2, 2]
    assert [float(x[0, 0, 0]) for x in control_image_batch(torch.cat([a, b]), 2, 1, False)] == [1, 2]
    with pytest.raises(ValueError, match="2 control images for 3 samples"):
        control_image_batch(torch.cat([a, b]), 3, 1, False)


@pytest.mark.parametrize("flavour", ["sd15", "sdxl"])
def test_pipeline_call_conditioning_and_key(emulated, flavour):
    pipe = _pipe(flavour)
    assert type(pipe) is (da.StableDiffusionXLControlNetPipeline if flavour == "sdxl" else da.StableDiffusionControlNetPipeline)
    assert pipe.components["controlnet"] is pipe.controlnet
    seen = _spy(pipe)
    g = torch.Generator().manual_seed(7)
    img, img2 = torch.rand(1, 3, 32, 32, generator=g), torch.rand(1, 3, 32, 32, generator=g)
    kw = _call_kw(flavour, n=2)
    pipe(image=img, num_images_per_prompt=2, guidance_scale=5.0, **kw)
    cn = seen["cond"]["controlnet"]
    assert tuple(seen["latents"].shape) == (4, 4, 16, 16)                                 # height / width come from the image
    assert cn["batch"] == 8 and tuple(cn["embed"].shape) == (8, 16, 16, 64) and tuple(cn["gate"].shape) == (8, 128)
    assert torch.equal(cn["embed"][0], cn["embed"][7]) and bool((cn["gate"] == 1.0).all()) and cn["gate"].dtype == torch.float32
    assert (cn["aug_emb"] is not None) == (flavour == "sdxl")
    key, embed_ptr = seen["key"], cn["embed"].data_ptr()
    # another image: same key, same static buffers, new contents
    before = cn["embed"].clone()
    pipe(image=img2, num_images_per_prompt=2, guidance_scale=5.0, **kw)
    cn2 = seen["cond"]["controlnet"]
    assert seen["key"] == key and cn2["embed"].data_ptr() == embed_ptr and not torch.equal(cn2["embed"], before)
    # another scale, other weights, another shape: another key
    pipe(image=img2, num_images_per_prompt=2, guidance_scale=5.0, controlnet_conditioning_scale=0.5, **kw)
    assert seen["key"] != key and bool((seen["cond"]["controlnet"]["gate"] == 0.5).all())
    pipe(image=img2, num_images_per_prompt=2, guidance_scale=5.0, **kw)
    assert seen["key"] == key
    pipe.controlnet.load_state_dict(dinit.random_state_dict(dinit.controlnet_param_shapes(pipe.controlnet.config), seed=9), device="cpu")
    pipe(image=img2, num_images_per_prompt=2, guidance_scale=5.0, **kw)
    assert seen["key"] != key
    key = seen["key"]
    pipe(image=torch.rand(1, 3, 32, 64), num_images_per_prompt=2, guidance_scale=5.0, **kw)
    assert seen["key"] != key and tuple(seen["latents"].shape) == (4, 4, 16, 32)
    # without CFG the control image is not doubled
    pipe(image=img, guidance_scale=1.0, **kw)
    assert seen["cond"]["controlnet"]["batch"] == 2
    assert pipe._cn_call is None


@pytest.mark.parametrize("flavour", ["sd15", "sdxl"])
def test_pipeline_refusals(emulated, flavour):
    pipe = _pipe(flavour)
    _spy(pipe)
    img, kw = torch.rand(1, 3, 32, 32), _call_kw(flavour)
    with pytest.raises(NotImplementedError, match="guess_mode"):
        pipe(image=img, guess_mode=True, **kw)
    with pytest.raises(NotImplementedError, match="control_guidance_start"):
        pipe(image=img, control_guidance_start=0.2, **kw)
    with pytest.raises(NotImplementedError, match="control_guidance_end"):
        pipe(image=img, control_guidance_end=0.8, **kw)
    with pytest.raises(NotImplementedError, match="`image` as a list"):
        pipe(image=[img, img], **kw)
    with pytest.raises(NotImplementedError, match="controlnet_conditioning_scale"):
        pipe(image=img, controlnet_conditioning_scale=[1.0, 0.5], **kw)
    with pytest.raises(ValueError, match="`image` is 32 x 31"):
        pipe(image=img[..., :31], **kw)
    with pytest.raises(ValueError, match="does not resize"):
        pipe(image=img, height=64, width=64, **kw)
    with pytest.raises(ValueError, match="required"):
        pipe(**kw)
    cls, parts = type(pipe), dict(vae=pipe.vae, unet=pipe.unet, scheduler=pipe.scheduler)
    with pytest.raises(NotImplementedError, match="several ControlNets"):
        cls(controlnet=[pipe.controlnet, pipe.controlnet], **parts)
    with pytest.raises(ValueError, match="needs its `controlnet`"):
        cls(**parts)
    other = da.ControlNetModel(**dict(dinit.TINY_SD15_CONTROLNET, block_out_channels=(64, 192)))
    with pytest.raises(ValueError, match="`block_out_channels` = .* does not match the U-Net's"):
        cls(controlnet=other, **parts)
    eight = da.ControlNetModel(**dict(pipe.controlnet.config, conditioning_embedding_out_channels=(16, 32, 96, 256)))
    with pytest.raises(ValueError, match="downsamples 8 x, the VAE 2 x"):
        cls(controlnet=eight, **parts)


def test_whole_call_on_the_stand_ins(emulated):
    """Eager, tiny SD1.5: scale 0 and zeroed zero convs both give the base pipeline's latents to the bit; scale 1 does not."""
    pipe = _pipe("sd15")
    base = factory.build_sd15_pipeline(device="cpu", tiny=True)
    kw = _call_kw("sd15")
    kw.update(latents=torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(2)).to(bf16), guidance_scale=5.0, use_graph=False)
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    want = base(height=32, width=32, **kw).images
    assert torch.equal(pipe(image=img, controlnet_conditioning_scale=0.0, **kw).images, want)
    assert not torch.equal(pipe(image=img, **kw).images, want)
    zero = factory.build_controlnet(dinit.TINY_SD15_UNET, seed=3, device="cpu", zero_convs=True, conditioning_embedding_out_channels=(16, 32))[0]
    pz = factory.build_sd15_pipeline(device="cpu", tiny=True, controlnet=zero)
    assert torch.equal(pz(image=img, **kw).images, want)


def test_packed_cache_and_from_pretrained(emulated, tmp_path):
    """``from_pretrained`` over a reference-layout directory: packs once, the second load reads the packed file; the pipeline's
    ``controlnet`` slot loads through it."""
    from diffusers_amd.loading import save_reference_checkpoint
    cn, sd = factory.build_controlnet(dinit.TINY_SD15_UNET, seed=3, device="cpu", conditioning_embedding_out_channels=(16, 32))
    d = save_reference_checkpoint(sd, dict(cn.config, _class_name="ControlNetModel"), tmp_path / "cn")
    a = da.ControlNetModel.from_pretrained(d, device="cpu")
    assert len(list((d / "diffusers_amd_packed").glob("ControlNetModel-*.safetensors"))) == 1
    b = da.ControlNetModel.from_pretrained(d, device="cpu")
    g = torch.Generator().manual_seed(0)
    x, ehs, img = torch.randn(1, 4, 16, 16, generator=g).to(bf16), torch.randn(1, 7, 64, generator=g).to(bf16), torch.rand(1, 3, 32, 32, generator=g)
    outs = [m(x, 500.0, ehs, img, return_dict=False)[1] for m in (cn, a, b)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_pipeline_from_a_local_directory(emulated, tmp_path):
    """A pipeline directory whose ``model_index.json`` has a ``controlnet`` slot, and the usual recipe: a base SDXL directory plus
    ``controlnet=``; both equal the pipeline assembled by hand from the same seeded weights."""
    import json
    from diffusers_amd import loading
    from diffusers_amd.autoencoder_kl import AutoencoderKL
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    root = tmp_path / "pipe"
    usd = dinit.random_state_dict(dinit.unet_param_shapes(UNet2DConditionModel(**dinit.TINY_SDXL_UNET).config), seed=0)
    loading.save_reference_checkpoint(usd, dict(dinit.TINY_SDXL_UNET, _class_name="UNet2DConditionModel"), root / "unet")
    vsd = dinit.random_state_dict(dinit.vae_decoder_param_shapes(AutoencoderKL(**dinit.TINY_VAE).config), seed=1)
    loading.save_reference_checkpoint(vsd, dict(dinit.TINY_VAE, _class_name="AutoencoderKL"), root / "vae")
    cn, csd = factory.build_controlnet(dinit.TINY_SDXL_UNET, seed=3, device="cpu", conditioning_embedding_out_channels=(16, 32))
    loading.save_reference_checkpoint(csd, dict(cn.config, _class_name="ControlNetModel"), root / "controlnet")
    (root / "scheduler").mkdir(parents=True)
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(factory.SDXL_SCHEDULER, _class_name="EulerDiscreteScheduler")))
    index = {"_class_name": "StableDiffusionXLControlNetPipeline", "unet": ["diffusers", "UNet2DConditionModel"],
             "vae": ["diffusers", "AutoencoderKL"], "scheduler": ["diffusers", "EulerDiscreteScheduler"],
             "controlnet": ["diffusers", "ControlNetModel"], "text_encoder": [None, None], "tokenizer": [None, None]}
    (root / "model_index.json").write_text(json.dumps(index))
    kw = _call_kw("sdxl")
    kw.update(latents=torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(2)).to(bf16), guidance_scale=5.0, use_graph=False)
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    want = _pipe("sdxl")(image=img, **{k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}).images
    pipe = da.StableDiffusionXLControlNetPipeline.from_pretrained(root, device="cpu")
    assert isinstance(pipe.controlnet, da.ControlNetModel)
    assert torch.equal(pipe(image=img, **{k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}).images, want)
    (root / "model_index.json").write_text(json.dumps({k: v for k, v in dict(index, _class_name="StableDiffusionXLPipeline").items()
                                                       if k != "controlnet"}))
    with pytest.raises(ValueError, match="needs its `controlnet`"):
        da.StableDiffusionXLControlNetPipeline.from_pretrained(root, device="cpu")
    pipe = da.StableDiffusionXLControlNetPipeline.from_pretrained(root, device="cpu", controlnet=cn)
    assert pipe.controlnet is cn
    assert torch.equal(pipe(image=img, **{k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}).images, want)
    with pytest.raises(ValueError, match="StableDiffusionXLPipeline"):          # (the other family's class still refuses it)
        da.StableDiffusionControlNetPipeline.from_pretrained(root, device="cpu", controlnet=cn)
