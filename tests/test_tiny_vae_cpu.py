"""AutoencoderTiny's host side: config validation, state-dict inventory, decode / encode on the CPU stand-ins against the restated
reference (tests/tiny_vae_emulation.py), wiring into the package and the pipelines, the ABI facts of the two additions, and the
host-side model of the conv kernel's address arithmetic."""
import inspect
import math
import re
from pathlib import Path

import pytest
import torch

import diffusers_amd
from conftest import rel_rms
from diffusers_amd import _lib as L
from diffusers_amd import factory, init as dinit, ops
from diffusers_amd import pipelines as P
from diffusers_amd.autoencoder_tiny import AutoencoderTiny, AutoencoderTinyOutput

import tiny_vae_emulation as TE

bf16 = torch.bfloat16
HEADER = (Path(__file__).resolve().parent.parent / "include" / "diffusers_amd.h").read_text()


# ---- config ---------------------------------------------------------------------------------------------------------
def test_defaults_are_the_reference_config():
    c = AutoencoderTiny().config
    assert dict(c) == dict(dinit.TAESD, block_out_channels=(64, 64, 64, 64))
    assert c.scaling_factor == 1.0 and c.shift_factor == 0.0 and c.force_upcast is False and c.latent_magnitude == 3
    assert dinit.TAESDXL == dinit.TAESD and dinit.TAEF1["latent_channels"] == 16
    assert c.get("latents_mean") is None                     # what the pipelines' _decode asks every VAE config


@pytest.mark.parametrize("kw, key", [
    (dict(encoder_block_out_channels=(64, 64, 128, 64)), "encoder_block_out_channels"),
    (dict(decoder_block_out_channels=(32, 64, 64, 64)), "decoder_block_out_channels"),
    (dict(act_fn="swish"), "act_fn"),
    (dict(upsample_fn="bilinear"), "upsample_fn"),
    (dict(upsampling_scaling_factor=4), "upsampling_scaling_factor"),
    (dict(latent_channels=32), "latent_channels"),
    (dict(num_encoder_blocks=(1, 3, 3)), "encoder_block_out_channels"),
    (dict(num_decoder_blocks=(3, 3, 1)), "decoder_block_out_channels"),
])
def test_unsupported_configs_are_refused_by_name(kw, key):
    with pytest.raises(ValueError, match=key):
        AutoencoderTiny(**kw)


def test_unknown_keys_raise_type_error():
    with pytest.raises(TypeError, match="norm_num_groups"):
        AutoencoderTiny(norm_num_groups=32)


def test_from_config_round_trip():
    ref_json = dict(dinit.TAEF1, _class_name="AutoencoderTiny", _diffusers_version="0.35.0",
                    block_out_channels=[64, 64, 64, 64], encoder_block_out_channels=[64, 64, 64, 64],
                    decoder_block_out_channels=[64, 64, 64, 64], num_encoder_blocks=[1, 3, 3, 3], num_decoder_blocks=[3, 3, 3, 1])
    m = AutoencoderTiny.from_config(ref_json)
    assert dict(m.config) == dict(dinit.TAEF1, block_out_channels=(64, 64, 64, 64))
    again = AutoencoderTiny.from_config(m.config)
    assert dict(again.config) == dict(m.config)
    with pytest.raises(ValueError, match="block_out_channels"):
        AutoencoderTiny(block_out_channels=(64, 64))


# ---- inventory ------------------------------------------------------------------------------------------------------
def _count(sh):
    return sum(math.prod(s) for s in sh.values())


def test_parameter_counts():
    enc = dinit.tiny_vae_param_shapes(dinit.TAESD, halves=("encoder",))
    dec = dinit.tiny_vae_param_shapes(dinit.TAESD, halves=("decoder",))
    both = dinit.tiny_vae_param_shapes(dinit.TAESD)
    assert (_count(enc), _count(dec), _count(both)) == (1222532, 1222531, 2445063)
    assert not set(enc) & set(dec) and list(both) == list(enc) + list(dec)
    f1 = dinit.tiny_vae_param_shapes(dinit.TAEF1)
    # 12 more latent channels on either side of the bottleneck: 12 * 64 * 9 weights each way + 12 encoder biases
    assert _count(f1) == 2445063 + 2 * 12 * 64 * 9 + 12
    assert f1["decoder.layers.0.weight"] == (64, 16, 3, 3) and f1["encoder.layers.14.weight"] == (16, 64, 3, 3)


def test_state_dict_keys_follow_the_sequential_indices():
    dec = dinit.tiny_vae_param_shapes(dinit.TAESD, halves=("decoder",))
    # 0 conv, 1 ReLU, 2-4 blocks, 5 Upsample, 6 conv, 7-9, 10, 11, 12-14, 15, 16, 17 block, 18 conv_out
    assert "decoder.layers.1.weight" not in dec and not any(k.startswith(("decoder.layers.5.", "decoder.layers.10.", "decoder.layers.15.")) for k in dec)
    assert dec["decoder.layers.0.weight"] == (64, 4, 3, 3) and dec["decoder.layers.0.bias"] == (64,)
    for n in (6, 11, 16):
        assert dec[f"decoder.layers.{n}.weight"] == (64, 64, 3, 3) and f"decoder.layers.{n}.bias" not in dec
    assert dec["decoder.layers.18.weight"] == (3, 64, 3, 3) and dec["decoder.layers.18.bias"] == (3,)
    blocks = sorted({int(k.split(".")[2]) for k in dec if ".conv." in k})
    assert blocks == [2, 3, 4, 7, 8, 9, 12, 13, 14, 17]
    assert {k.split(".", 3)[3] for k in dec if k.startswith("decoder.layers.2.")} == {f"conv.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")}
    enc = dinit.tiny_vae_param_shapes(dinit.TAESD, halves=("encoder",))
    assert enc["encoder.layers.0.weight"] == (64, 3, 3, 3) and "encoder.layers.0.bias" in enc
    for n in (2, 6, 10):
        assert enc[f"encoder.layers.{n}.weight"] == (64, 64, 3, 3) and f"encoder.layers.{n}.bias" not in enc
    assert enc["encoder.layers.14.weight"] == (4, 64, 3, 3) and sorted({int(k.split(".")[2]) for k in enc if ".conv." in k}) == [1, 3, 4, 5, 7, 8, 9, 11, 12, 13]
    # the restatement walks the same keys
    sd = {k: torch.zeros(s) for k, s in dinit.tiny_vae_param_shapes(dinit.TAESD).items()}
    assert len(TE.ref_layers(sd, dinit.TAESD, "decoder", torch.float32)) == 19 and len(TE.ref_layers(sd, dinit.TAESD, "encoder", torch.float32)) == 15


def test_strict_load_and_missing_encoder():
    vae, sd = factory.build_tiny_vae(dinit.TINY_TAESD, seed=4, device="cpu", with_encoder=False)
    assert vae.encoder is None and vae._weights_generation > 0
    with pytest.raises(NotImplementedError, match="encoder half was not loaded"):
        vae.encode(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="round trip"):
        vae.forward(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="unexpected AutoencoderTiny keys"):
        AutoencoderTiny(**dinit.TINY_TAESD).load_state_dict(dict(sd, **{"decoder.layers.99.weight": torch.zeros(1)}), device="cpu", strict=True)
    full, sd_full = factory.build_tiny_vae(dinit.TINY_TAESD, seed=4, device="cpu")
    assert full.encoder is not None and all(torch.equal(sd_full[k], v) for k, v in sd.items())


def test_packed_cache_round_trip(tmp_path):
    from diffusers_amd import packed_cache as PC
    for with_encoder in (False, True):
        vae, _ = factory.build_tiny_vae(dinit.TINY_TAEF1, seed=2, device="cpu", with_encoder=with_encoder)
        path = PC.save_packed(vae, tmp_path / f"t{int(with_encoder)}.safetensors", source_fingerprint="f")
        again = PC.load_packed(AutoencoderTiny, path, device="cpu", expect_fingerprint="f")
        a, b = PC.packed_tensors(vae), PC.packed_tensors(again)
        assert (again.encoder is not None) == with_encoder and list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_from_pretrained_packs_once_and_reads_the_cache(tmp_path):
    import json
    from safetensors.torch import save_file
    from diffusers_amd import packed_cache as PC
    cfg = dict(dinit.TINY_TAESD, _class_name="AutoencoderTiny", block_out_channels=[64, 64])
    sd = dinit.random_state_dict(dinit.tiny_vae_param_shapes(dinit.TINY_TAESD), seed=6)
    d = tmp_path / "vae"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(cfg))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    first = AutoencoderTiny.from_pretrained(tmp_path, subfolder="vae", device="cpu")
    cached = list((d / "diffusers_amd_packed").glob("AutoencoderTiny-*.safetensors"))
    assert len(cached) == 1 and first.encoder is not None and dict(first.config) == dict(dinit.TINY_TAESD, block_out_channels=(64, 64))
    again = AutoencoderTiny.from_pretrained(tmp_path, subfolder="vae", device="cpu")
    a, b = PC.packed_tensors(first), PC.packed_tensors(again)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a) and again._weights_generation != first._weights_generation


# ---- decode / encode on the stand-ins -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_case():
    cfg = dinit.TINY_TAESD
    sd = dinit.random_state_dict(dinit.tiny_vae_param_shapes(cfg), seed=11)
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(2, 4, 8, 6, generator=g) * 2).to(bf16)
    img = (torch.rand(2, 3, 16, 12, generator=g) * 2 - 1).to(bf16)
    return cfg, sd, z, img


def _floor_gate(got, ref32, ref16, what):
    e, f = rel_rms(got, ref32), rel_rms(ref16, ref32)
    print(f"[tiny-vae] {what}: engine {e:.3e}  floor {f:.3e}")
    assert e <= 1.5 * f, f"{what}: engine rel rms {e:.3e} > 1.5 x floor {f:.3e}"


@pytest.mark.parametrize("div, add", [(1.0, 0.0), (0.13025, 0.0), (0.3611, 0.1159)])
def test_decode_on_stand_ins_matches_the_restatement(monkeypatch, tiny_case, div, add):
    cfg, sd, z, _ = tiny_case
    TE.install(monkeypatch, ops)
    vae = AutoencoderTiny(**cfg).load_state_dict(sd, device="cpu")
    got = vae.decode(z, latents_div=div, latents_add=add).sample
    assert got.dtype == bf16 and tuple(got.shape) == (2, 3, 16, 12)
    ref32 = TE.ref_decode(sd, cfg, z, torch.float32, div, add)
    _floor_gate(got, ref32, TE.ref_decode(sd, cfg, z, bf16, div, add), f"decode / {div} + {add}")
    assert vae.decode(z, return_dict=False)[0].shape == got.shape
    for mode in ("pt", "np", "uint8"):
        out = vae.decode(z, latents_div=div, latents_add=add, postprocess=mode).sample
        want = TE.ref_postprocess(ref32, mode)
        assert out.shape == want.shape and out.dtype == want.dtype
        if mode == "uint8":
            assert int((out.int() - want.int()).abs().max()) <= 1
        else:                                        # the fused postprocess is the postprocess of the decoder's own bf16 output
            assert float((out - TE.ref_postprocess(got, mode)).abs().max()) <= 1e-6


def test_encode_on_stand_ins_matches_the_restatement(monkeypatch, tiny_case):
    cfg, sd, _, img = tiny_case
    TE.install(monkeypatch, ops)
    vae = AutoencoderTiny(**cfg).load_state_dict(sd, device="cpu")
    out = vae.encode(img)
    assert isinstance(out, AutoencoderTinyOutput) and out.latents.dtype == bf16 and tuple(out.latents.shape) == (2, 4, 8, 6)
    ref32 = TE.ref_encode(sd, cfg, img, torch.float32)
    _floor_gate(out.latents, ref32, TE.ref_encode(sd, cfg, img, bf16), "encode")
    # pixels in [0, 1]: fp32 NCHW, fp32 NHWC and bytes (bytes are another image: compare with its own restatement)
    img01 = ((img.float() + 1) / 2)
    assert torch.equal(vae.encode_image(img01.contiguous(), nchw=True).latents, out.latents)
    assert torch.equal(vae.encode_image(img01.permute(0, 2, 3, 1).contiguous(), nchw=False).latents, out.latents)
    u8 = (img01.permute(0, 2, 3, 1) * 255).round().to(torch.uint8).contiguous()
    lat8 = vae.encode_image(u8, nchw=False).latents
    ref8 = TE.ref_encode(sd, cfg, (u8.float() / 255).to(bf16).permute(0, 3, 1, 2) * 2 - 1, torch.float32)
    assert rel_rms(lat8, ref8) < 2e-2
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        vae.encode_image(img01.contiguous(), nchw=True, normalize=False)
    with pytest.raises(ValueError, match="multiple of 2"):
        vae.encode(torch.zeros(1, 3, 7, 8))
    assert vae.encode(img, return_dict=False)[0].shape == out.latents.shape


def test_decode_packs_the_affine_map_and_pads_conv_in():
    cfg, sd = dinit.TINY_TAESD, dinit.random_state_dict(dinit.tiny_vae_param_shapes(dinit.TINY_TAESD), seed=11)
    vae = AutoencoderTiny(**cfg).load_state_dict(sd, device="cpu")
    d = vae.decoder
    assert torch.equal(d.out_w, ops.pack_conv_weight(sd["decoder.layers.6.weight"] * 2))
    assert torch.equal(d.out_b, (sd["decoder.layers.6.bias"].float() * 2 - 1).to(bf16))
    first = d.steps[0]
    assert first.k_valid == 4 and tuple(first.weight.shape) == (64, 576) and not first.weight.view(64, 9, 64)[..., 4:].any()
    assert torch.equal(first.weight.view(64, 9, 64)[..., :4], sd["decoder.layers.0.weight"].permute(0, 2, 3, 1).reshape(64, 9, 4))
    assert [type(s).__name__ for s in d.steps] == ["_ReluConv", "_Block", "_PlainConv", "_Block"] and d.steps[2].up


def test_scale_and_unscale_latents():
    vae = AutoencoderTiny()
    x = torch.linspace(-4, 4, 33)
    assert torch.equal(vae.scale_latents(x), x.div(6).add(0.5).clamp(0, 1))
    assert torch.equal(vae.unscale_latents(x), x.sub(0.5).mul(6))


# ---- wiring ---------------------------------------------------------------------------------------------------------
def test_exported_and_found_by_the_pipeline_loader():
    assert diffusers_amd._EXPORTS["AutoencoderTiny"] == "autoencoder_tiny" and "AutoencoderTiny" in diffusers_amd.__all__
    assert diffusers_amd.AutoencoderTiny is AutoencoderTiny
    from diffusers_amd import packed_cache as PC
    assert "AutoencoderTiny" in PC._SHAPES


def test_pipelines_take_it_in_the_vae_slot():
    vae, _ = factory.build_tiny_vae(dinit.TAESDXL, seed=1, device="cpu", with_encoder=False)
    pipe = factory.build_sdxl_pipeline(device="cpu", tiny=True, tiny_vae=True, scheduler="lcm")
    assert isinstance(pipe.vae, AutoencoderTiny) and pipe.vae_scale_factor == 2 and pipe.vae.encoder is None
    full = type(pipe)(vae=vae, unet=pipe.unet, scheduler=pipe.scheduler)           # the real TAESDXL in the same pipeline: 8 x
    assert full.vae_scale_factor == 8
    flux = factory.build_flux_pipeline(device="cpu", tiny=True, tiny_vae=True)
    assert isinstance(flux.vae, AutoencoderTiny) and flux.vae.config.latent_channels == 16 and flux.vae_scale_factor == 2
    assert flux.vae.config.scaling_factor == 0.3611 and flux.vae.config.shift_factor == 0.1159
    for build in (factory.build_sdxl_pipeline, factory.build_sd15_pipeline, factory.build_flux_pipeline):
        with pytest.raises(ValueError, match="no posterior"):
            build(device="cpu", tiny=True, tiny_vae=True, img2img=True)


@pytest.mark.parametrize("cls", [P.StableDiffusionImg2ImgPipeline, P.StableDiffusionXLImg2ImgPipeline, P.StableDiffusionInpaintPipeline,
                                 P.StableDiffusionXLInpaintPipeline, P.FluxImg2ImgPipeline, P.FluxInpaintPipeline])
def test_image_conditioned_pipelines_refuse_it(cls):
    pipe = object.__new__(cls)
    pipe.vae = AutoencoderTiny()
    n = len(inspect.signature(pipe._image_call).parameters)
    with pytest.raises(NotImplementedError, match=f"{cls.__name__}: AutoencoderTiny has no posterior"):
        pipe._image_call(*([None] * n))
    # an AutoencoderKL goes on to the pipeline's own first check
    pipe.vae = object()
    with pytest.raises(Exception) as e:
        pipe._image_call(*([None] * n))
    assert "AutoencoderTiny" not in str(e.value)


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_abi_facts():
    assert re.search(r"^#define DA_ACT_RELU 7\b", HEADER, re.M) and L.ACT_RELU == 7
    assert re.search(r"^#define DA_ABI_VERSION 9\b", HEADER, re.M) and L.ABI_VERSION == 9 and L.FN_COUNT == 36
    name = "da_tiny_vae_latents_in"
    assert re.search(r"^int da_tiny_vae_latents_in\(const void\* x, void\* y, int B, int L, int H, int W, float in_div, float in_add, "
                     r"float magnitude,\s+void\* stream\);", HEADER, re.M)
    _i, _f, _vp = L._i, L._f, L._vp
    assert L.SIGNATURES[name] == (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp])
    assert name in L.PASS_THROUGH and name not in L.FN_IDS and name not in L.NOT_PLANNABLE
    assert L.PASS_THROUGH[name] == "runs once per decode, outside any recorded step; ops.tiny_vae_latents_in refuses under a recording"
    assert L.NOT_PLANNABLE == ("da_vae_conv_in_image", "da_vae_posterior_latents", "da_flux_prepare_latents")
    assert len(L.TILE_NAMES) == 22                                 # no new DA_TILE_*


def test_latents_in_wrapper_refuses_under_a_recording(monkeypatch):
    monkeypatch.setattr(L._tls, "recorder", object(), raising=False)
    with pytest.raises(RuntimeError, match="not replayable by a launch plan"):
        ops.tiny_vae_latents_in(torch.zeros(1, 4, 2, 2, dtype=bf16))


# ---- the conv kernel's address arithmetic, host-side model -----------------------------------------------------------
def test_tiles_cover_every_pixel_once():
    for B, H, W in ((1, 1, 1), (2, 3, 5), (1, 17, 33), (2, 64, 64), (1, 9, 70)):
        seen = torch.zeros(B, H, W, dtype=torch.int32)
        for b, y0, x0 in TE.tiles(B, H, W):
            assert y0 < H and x0 < W
            seen[b, y0:y0 + TE.TH, x0:x0 + TE.TW] += 1
            for off, inside in TE.halo_offsets(b, y0, x0, H, W):
                assert 0 <= off and off + 8 <= B * H * W * 64          # clamped: in the tensor whether it is used or not
            outs = TE.output_offsets(b, y0, x0, H, W)
            assert all(0 <= o and o + 4 <= B * H * W * 64 for o in outs)
        assert bool((seen == 1).all())


def test_offsets_past_2_31_elements_need_more_than_32_bits():
    """4096 x 4096 x 64 channels is 2^30 elements an image: image 2 of a batch of 3 starts at element 2^31 = byte 2^32.  The model in
    unbounded integers stays in the tensor; the same sums in a 31-bit (signed int) element index or a 32-bit byte offset do not --
    which is what the kernel's size_t arithmetic is there for."""
    B, H, W = 3, 4096, 4096
    total = B * H * W * 64
    assert total > 1 << 31
    last = list(TE.tiles(1, H, W))[-1]
    b, y0, x0 = 2, last[1], last[2]
    for t in ((b, y0, x0), (b, 0, 0), (0, y0, x0)):
        halo = TE.halo_offsets(*t, H, W)
        outs = TE.output_offsets(*t, H, W)
        assert all(0 <= o and o + 8 <= total for o, _ in halo) and all(0 <= o and o + 4 <= total for o in outs)
        assert len(set(outs)) == len(outs) == TE.TH * TE.TW * 16
    assert min(TE.output_offsets(b, 0, 0, H, W)) >= 1 << 31 and min(o for o, _ in TE.halo_offsets(b, 0, 0, H, W)) >= 1 << 31
    assert TE.output_offsets(b, y0, x0, H, W, wrap=31) != TE.output_offsets(b, y0, x0, H, W)
    assert TE.halo_offsets(b, y0, x0, H, W, wrap=31) != TE.halo_offsets(b, y0, x0, H, W)
    assert all((2 * o) >> 32 for o in TE.output_offsets(b, y0, x0, H, W))            # every byte offset of the tile needs bit 32
    # the halo of an edge tile: clamped chunks are flagged and read a pixel of the same image
    edge = TE.halo_offsets(b, y0, x0, H, W)
    assert any(not inside for _, inside in edge) and all(o >= b * H * W * 64 for o, _ in edge)
