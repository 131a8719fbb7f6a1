"""CPU: host side of AutoencoderKL.encode and the img2img pipelines -- get_timesteps / denoising_start arithmetic against a literal
restatement of the reference formulas (pipeline_stable_diffusion_xl_img2img.py get_timesteps), the refiner's add-time-ids, input
validation, the encoder's parameter inventory and the schedulers' add_noise coefficients.  No kernel is launched."""
import math

import numpy as np
import pytest
import torch

from diffusers_amd import factory, init as dinit
from diffusers_amd.autoencoder_kl import AutoencoderKL
from diffusers_amd.pipelines import StableDiffusionXLImg2ImgPipeline, get_timesteps, prepare_image
from diffusers_amd.schedulers import DDIMScheduler, DDPMScheduler, EulerDiscreteScheduler
from diffusers_amd.unet_2d_condition import UNet2DConditionModel


def _ref_get_timesteps(timesteps, order, n_train, num_inference_steps, strength, denoising_start):
    """The reference's get_timesteps, restated literally (t_start, number of steps)."""
    if denoising_start is None:
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        return t_start * order, num_inference_steps - t_start
    discrete_timestep_cutoff = int(round(n_train - (denoising_start * n_train)))
    num_inference_steps = (timesteps < discrete_timestep_cutoff).sum().item()
    if order == 2 and num_inference_steps % 2 == 0:
        num_inference_steps = num_inference_steps + 1
    t_start = len(timesteps) - num_inference_steps
    return t_start, num_inference_steps


def _schedulers():
    return [EulerDiscreteScheduler(**factory.SDXL_SCHEDULER), DDIMScheduler(**factory.SD15_SCHEDULER)]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("steps", [1, 4, 7, 20, 50])
@pytest.mark.parametrize("strength", [0.0, 0.05, 0.3, 0.5, 0.6, 0.99, 1.0])
def test_get_timesteps_strength_matches_reference(which, steps, strength):
    sch = _schedulers()[which]
    sch.set_timesteps(steps, device="cpu")
    ts, n, begin = get_timesteps(sch, steps, strength)
    want_begin, want_n = _ref_get_timesteps(sch.timesteps, sch.order, 1000, steps, strength, None)
    assert (begin, n) == (want_begin, want_n)
    assert torch.equal(ts, sch.timesteps[want_begin:]) and len(ts) == want_n
    assert sch.begin_index == want_begin
    if strength == 1.0:
        assert begin == 0 and n == steps
    if int(steps * strength) == 0:
        assert n == 0                      # the pipelines refuse this (no step would run)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("steps", [4, 10, 25, 40])
@pytest.mark.parametrize("start", [0.1, 0.5, 0.8, 0.95])
def test_get_timesteps_denoising_start_matches_reference(which, steps, start):
    sch = _schedulers()[which]
    sch.set_timesteps(steps, device="cpu")
    ts, n, begin = get_timesteps(sch, steps, 0.3, denoising_start=start)
    want_begin, want_n = _ref_get_timesteps(sch.timesteps, sch.order, 1000, steps, 0.3, start)
    assert (begin, n) == (want_begin, want_n) and sch.begin_index == want_begin
    cutoff = int(round(1000 - start * 1000))
    # the hand-off property: the base stops exactly where the refiner starts
    from diffusers_amd.pipelines import denoising_end_steps
    assert denoising_end_steps(sch, start) == begin
    assert all(int(t) < cutoff for t in ts)


def test_set_begin_index_moves_the_device_step_counter():
    sch = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    sch.set_timesteps(10, device="cpu")
    get_timesteps(sch, 10, 0.6)
    assert int(sch.device_step) == 4 and sch.step_index is None


def _tiny_sdxl_img2img(requires_aesthetics_score, tiny_cfg):
    vae = AutoencoderKL(**dinit.TINY_VAE)
    unet = UNet2DConditionModel(**tiny_cfg)
    return StableDiffusionXLImg2ImgPipeline(vae=vae, unet=unet, scheduler=EulerDiscreteScheduler(**factory.SDXL_SCHEDULER),
                                            requires_aesthetics_score=requires_aesthetics_score)


def test_sdxl_img2img_add_time_ids():
    proj = 64
    base = dict(dinit.TINY_SDXL_UNET)
    p = _tiny_sdxl_img2img(False, base)
    ids, neg = p._get_add_time_ids((32, 48), (0, 0), (32, 48), 6.0, 2.5, (16, 16), (4, 4), (8, 8),
                                   text_encoder_projection_dim=proj)
    # without the aesthetics score: [orig, crop, target]; the negative ids take the POSITIVE crop (the reference's own quirk)
    assert ids.tolist() == [[32, 48, 0, 0, 32, 48]] and neg.tolist() == [[16, 16, 0, 0, 8, 8]]
    with pytest.raises(ValueError, match="enable `requires_aesthetics_score`|disable `requires_aesthetics_score`|incorrect config"):
        _tiny_sdxl_img2img(True, base)._get_add_time_ids((32, 48), (0, 0), (32, 48), 6.0, 2.5, (16, 16), (4, 4), (8, 8),
                                                         text_encoder_projection_dim=proj)
    # a refiner-shaped U-Net: five ids (orig, crop, aesthetic score)
    d = base["addition_time_embed_dim"]
    ref_cfg = dict(base, projection_class_embeddings_input_dim=base["projection_class_embeddings_input_dim"] - d)
    r = _tiny_sdxl_img2img(True, ref_cfg)
    ids, neg = r._get_add_time_ids((32, 48), (2, 3), (32, 48), 6.1, 2.5, (16, 16), (4, 4), (8, 8),
                                   text_encoder_projection_dim=proj)
    assert ids.tolist() == [[32, 48, 2, 3, float(torch.tensor(6.1, dtype=torch.bfloat16))]]
    assert neg.tolist() == [[16, 16, 4, 4, 2.5]]
    with pytest.raises(ValueError, match="enable `requires_aesthetics_score`|disable `requires_aesthetics_score`"):
        _tiny_sdxl_img2img(False, ref_cfg)._get_add_time_ids((32, 48), (0, 0), (32, 48), 6.0, 2.5, (16, 16), (0, 0), (8, 8),
                                                             text_encoder_projection_dim=proj)


def test_prepare_image_validation():
    # 3 channels: an image; 4 channels: latents (encode is skipped); anything else is refused
    kind, t, nchw, norm = prepare_image(torch.rand(1, 3, 32, 16), 8, 4, "cpu")
    assert kind == "image" and nchw and norm and t.dtype == torch.float32
    kind, t, nchw, norm = prepare_image(torch.rand(1, 3, 32, 16) * 2 - 1, 8, 4, "cpu")
    assert kind == "image" and not norm                       # already in [-1, 1]: not normalised again
    kind, t = prepare_image(torch.randn(2, 4, 5, 7), 8, 4, "cpu")
    assert kind == "latents" and t.dtype == torch.bfloat16 and t.shape == (2, 4, 5, 7)
    with pytest.raises(ValueError, match="5 channels"):
        prepare_image(torch.rand(1, 5, 32, 32), 8, 4, "cpu")
    with pytest.raises(ValueError, match="30 x 32"):
        prepare_image(torch.rand(1, 3, 30, 32), 8, 4, "cpu")
    with pytest.raises(ValueError, match="32 x 20"):
        prepare_image(np.zeros((32, 20, 3), np.uint8), 8, 4, "cpu")
    kind, t, nchw, norm = prepare_image(np.zeros((32, 16, 3), np.uint8), 8, 4, "cpu")
    assert kind == "image" and not nchw and norm and t.dtype == torch.uint8 and t.shape == (1, 32, 16, 3)
    kind, t, nchw, norm = prepare_image(np.full((2, 16, 16, 3), 0.5, np.float64), 8, 4, "cpu")
    assert t.dtype == torch.float32 and not nchw
    with pytest.raises(ValueError, match="type"):
        prepare_image("not an image", 8, 4, "cpu")


def test_encode_without_encoder_weights_raises():
    vae, _ = factory.build_vae(dinit.TINY_VAE, seed=1, device="cpu")
    assert vae.encoder is None
    with pytest.raises(NotImplementedError, match="encoder half of this VAE was not loaded"):
        vae.encode(torch.zeros(1, 3, 16, 16))
    venc, sd = factory.build_vae(dinit.TINY_VAE, seed=1, device="cpu", with_encoder=True)
    assert venc.encoder is not None and any(k.startswith("encoder.") for k in sd)
    # the decoder weights do not depend on whether the encoder was generated too
    _, sd_dec = factory.build_vae(dinit.TINY_VAE, seed=1, device="cpu")
    assert all(torch.equal(sd[k], v) for k, v in sd_dec.items())


@pytest.mark.parametrize("cfg", [dinit.TINY_VAE, dinit.SD_VAE])
def test_vae_encoder_param_shapes(cfg):
    full = dict(AutoencoderKL(**cfg).config)
    enc, dec = dinit.vae_encoder_param_shapes(full), dinit.vae_decoder_param_shapes(full)
    assert not set(enc) & set(dec)
    assert all(k.startswith(("encoder.", "quant_conv.")) for k in enc)
    boc, lpb, lat = full["block_out_channels"], full["layers_per_block"], full["latent_channels"]
    assert enc["encoder.conv_in.weight"] == (boc[0], 3, 3, 3) and enc["encoder.conv_out.weight"] == (2 * lat, boc[-1], 3, 3)
    assert enc["quant_conv.weight"] == (2 * lat, 2 * lat, 1, 1)
    n_res = sum(1 for k in enc if k.endswith(".conv1.weight"))
    assert n_res == len(boc) * lpb + 2
    assert sum(1 for k in enc if "downsamplers" in k) == 2 * (len(boc) - 1)
    # conv_shortcut exactly where a block widens the channels
    shortcuts = sorted(k for k in enc if "conv_shortcut.weight" in k)
    want = [f"encoder.down_blocks.{i}.resnets.0.conv_shortcut.weight" for i in range(1, len(boc)) if boc[i] != boc[i - 1]]
    assert shortcuts == sorted(want)
    if cfg is dinit.SD_VAE:      # the SD / SDXL VAE encoder: 34 163 592 parameters (+ 72 of quant_conv)
        assert sum(math.prod(s) for s in enc.values()) == 34163592 + 72


@pytest.mark.parametrize("kind", ["euler", "ddim", "ddpm"])
def test_add_noise_coefficients_follow_the_reference(kind):
    bf = torch.bfloat16
    if kind == "euler":
        sch = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
        sch.set_timesteps(20, device="cpu")
        get_timesteps(sch, 20, 0.6)                      # begin index 8
        a, b = sch._add_noise_coeffs(sch.timesteps[8:9].repeat(2), bf)
        assert a == [1.0, 1.0] and b == [float(sch.sigmas.to(bf)[8])] * 2
        sch2 = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
        sch2.set_timesteps(20, device="cpu")             # no begin index: the index of each timestep
        a, b = sch2._add_noise_coeffs(sch2.timesteps[[3, 11]], bf)
        assert b == [float(sch2.sigmas.to(bf)[3]), float(sch2.sigmas.to(bf)[11])]
        return
    sch = DDIMScheduler(**factory.SD15_SCHEDULER) if kind == "ddim" else DDPMScheduler(**dinit.DDPM_SCHEDULER)
    sch.set_timesteps(10, device="cpu")
    t = torch.tensor([801, 1, 999])
    a, b = sch._add_noise_coeffs(t, bf)
    ac = sch.alphas_cumprod.to(dtype=bf)
    assert a == [float(v) for v in ac[t] ** 0.5] and b == [float(v) for v in (1 - ac[t]) ** 0.5]
    assert all(v == float(torch.tensor(v, dtype=bf)) for v in a + b)


@pytest.mark.parametrize("with_encoder", [False, True])
def test_packed_cache_round_trips_the_encoder(tmp_path, with_encoder):
    from diffusers_amd import packed_cache as PC
    vae, _ = factory.build_vae(dinit.TINY_VAE, seed=1, device="cpu", with_encoder=with_encoder)
    path = PC.save_packed(vae, tmp_path / "vae.safetensors", source_fingerprint="f")
    again = PC.load_packed(AutoencoderKL, path, device="cpu", expect_fingerprint="f")
    assert (again.encoder is not None) == with_encoder
    a, b = PC.packed_tensors(vae), PC.packed_tensors(again)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
