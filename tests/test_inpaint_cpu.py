"""CPU: host side of the inpainting pipelines -- mask preprocessing, the schedulers' add_noise tables, the draw order and start
latents of prepare_latents against a literal restatement (kernels replaced by the torch stand-ins of tests/inpaint_emulation.py),
the channel-count check and the refusals.  No kernel is launched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inpaint_emulation
from diffusers_amd import factory, ops
from diffusers_amd.pipelines import (StableDiffusionInpaintPipeline, StableDiffusionXLInpaintPipeline, get_timesteps,
                                     prepare_mask)
from diffusers_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler

bf16 = torch.bfloat16


@pytest.fixture
def emulated(monkeypatch):
    inpaint_emulation.install(monkeypatch, ops)


def _mask_32x48():
    v = torch.rand(32, 48, generator=torch.Generator().manual_seed(2))
    v[0, 0], v[0, 1], v[0, 2] = 0.5, 0.4999, 0.5001
    return v


def test_mask_forms_agree():
    v = _mask_32x48()
    want = (v >= 0.5).float()[None, None]
    assert want[0, 0, 0, 0] == 1 and want[0, 0, 0, 1] == 0 and want[0, 0, 0, 2] == 1          # the threshold is v >= 0.5
    forms = [v, v[None], v[None, None], v.numpy(), v.numpy()[..., None], v.numpy()[None, ..., None], [v]]
    for m in forms:
        got = prepare_mask(m, 2, "cpu")
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1, 32, 48) and torch.equal(got, want)
    two = prepare_mask(torch.stack([v, 1 - v])[:, None], 2, "cpu")
    assert tuple(two.shape) == (2, 1, 32, 48) and torch.equal(two[:1], want)
    # uint8 is read as x / 255: 127 keeps, 128 repaints
    u8 = (torch.arange(32 * 48) % 256).to(torch.uint8).reshape(32, 48).numpy()
    want8 = (torch.from_numpy(u8) >= 128).float()[None, None]
    assert torch.equal(prepare_mask(u8, 2, "cpu"), want8) and torch.equal(prepare_mask(u8[..., None], 2, "cpu"), want8)
    flat = want8.reshape(-1)                                      # (value k sits at flat index k)
    assert flat[127] == 0 and flat[128] == 1
    Image = pytest.importorskip("PIL.Image")
    assert torch.equal(prepare_mask(Image.fromarray(u8, mode="L"), 2, "cpu"), want8)
    assert torch.equal(prepare_mask(Image.fromarray(np.stack([u8] * 3, -1)), 2, "cpu"), want8)   # RGB grey -> "L"


def test_mask_refusals():
    with pytest.raises(ValueError, match="31 x 48"):
        prepare_mask(torch.zeros(31, 48), 2, "cpu")
    with pytest.raises(ValueError, match="must be"):
        prepare_mask(torch.zeros(2, 3, 32, 48), 2, "cpu")
    with pytest.raises(ValueError, match="type"):
        prepare_mask("mask.png", 2, "cpu")


def _schedulers():
    return {"euler": EulerDiscreteScheduler(**factory.SDXL_SCHEDULER),
            "euler_karras": EulerDiscreteScheduler(use_karras_sigmas=True, **factory.SDXL_SCHEDULER),
            "ddim": DDIMScheduler(**factory.SD15_SCHEDULER),
            "dpm": DPMSolverMultistepScheduler(**factory.SDXL_DPM_SCHEDULER)}


@pytest.mark.parametrize("kind", ["euler", "euler_karras", "ddim", "dpm"])
def test_add_noise_table_rows(kind):
    sch = _schedulers()[kind]
    sch.set_timesteps(10, device="cpu")
    get_timesteps(sch, 10, 0.6)                                   # a begin index and no step index: left as they are
    tab = sch.add_noise_table(bf16)
    assert sch.begin_index == 4 and sch.step_index is None
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (11, 2) and tab[10].tolist() == [1.0, 0.0]
    for j in range(10):
        sch._begin_index, sch._step_index = 0, j
        a, b = sch._add_noise_coeffs(sch.timesteps[j:j + 1], bf16)
        assert tab[j].tolist() == [a[0], b[0]], j
        assert a[0] == float(torch.tensor(a[0], dtype=bf16)) and b[0] == float(torch.tensor(b[0], dtype=bf16))
    if kind.startswith("euler"):
        assert tab[:10, 0].tolist() == [1.0] * 10 and tab[:10, 1].tolist() == [float(v) for v in sch.sigmas.to(bf16)[:10]]
    if kind == "ddim":
        ac = sch.alphas_cumprod.to(bf16)[sch.timesteps.long()]
        assert tab[:10, 0].tolist() == [float(v) for v in ac ** 0.5] and tab[:10, 1].tolist() == [float(v) for v in (1 - ac) ** 0.5]
    ptr = tab.data_ptr()
    sch.set_timesteps(10, device="cpu")
    assert sch.add_noise_table(bf16).data_ptr() == ptr           # refreshed in place: a captured graph keeps the address
    sch.set_timesteps(12, device="cpu")
    assert tuple(sch.add_noise_table(bf16).shape) == (13, 2)


def _rect_mask(H, W_):
    m = torch.zeros(H, W_)
    m[H // 4:3 * H // 4, W_ // 4:3 * W_ // 4] = 1.0
    return m


def _pipe(kind, channels):
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    return build(device="cpu", tiny=True, seed=0, inpaint=True, unet_in_channels=channels)


@pytest.mark.parametrize("kind,channels,case", [(k, c, s) for k in ("sdxl", "sd15") for c in (4, 9)
                                                for s in ("strength_1.0", "strength_0.5", "denoising_start")
                                                if k == "sdxl" or s != "denoising_start"])      # (denoising_start: SDXL only)
def test_draw_order_and_start_latents(emulated, kind, channels, case):
    pipe = _pipe(kind, channels)
    assert type(pipe) is (StableDiffusionXLInpaintPipeline if kind == "sdxl" else StableDiffusionInpaintPipeline)
    sch, steps, H, W_ = pipe.scheduler, 10, 32, 48
    img = torch.rand(1, 3, H, W_, generator=torch.Generator().manual_seed(4))
    mask = _rect_mask(H, W_)
    strength = 1.0 if case == "strength_1.0" else 0.5
    start_frac = 0.7 if case == "denoising_start" else None
    sch.set_timesteps(steps, device="cpu")
    ts, n, begin = get_timesteps(sch, steps, strength, start_frac)
    assert sch.begin_index == begin                              # set at every strength, 1.0 included
    ndt = torch.float32 if (kind == "sdxl" and pipe.vae.config.force_upcast) else bf16
    got = pipe._inpaint_prepare(img, mask, None, None, None, None, ts[:1], 1, torch.Generator().manual_seed(21), strength,
                                start_frac is None, ndt)
    st = pipe._inpaint

    # literal restatement: (1) posterior noise of the image, (2) noise, (3) posterior noise of the masked image (9 channels only)
    g = torch.Generator().manual_seed(21)
    sf = float(pipe.vae.config.scaling_factor)
    x = 2.0 * img - 1.0
    eps1 = torch.randn(1, 4, H // 2, W_ // 2, generator=g, dtype=ndt).to(bf16)
    z = pipe.vae.encode_image(x.contiguous(), nchw=True, normalize=False).latents(eps1, scale=sf)
    noise = torch.randn(1, 4, H // 2, W_ // 2, generator=g, dtype=bf16)
    assert torch.equal(st["image_latents"], z) and torch.equal(st["noise"], noise)
    if case == "strength_1.0":
        want = (noise.float() * float(sch.init_noise_sigma)).to(bf16)
    elif case == "strength_0.5":
        a, b = sch._add_noise_coeffs(ts[:1], bf16)
        want = inpaint_emulation.add_noise(z, noise, a[0], b[0])
        if kind == "sdxl":
            assert (a[0], b[0]) == (1.0, float(sch.sigmas.to(bf16)[begin]))
    else:
        want = z
    assert torch.equal(got, want)
    mlat = F.interpolate((mask >= 0.5).float()[None, None], size=(H // 2, W_ // 2)).to(bf16)
    assert torch.equal(st["mask"], mlat) and torch.equal(mlat[0, 0], mask[::2, ::2].to(bf16))
    if channels == 9:
        eps3 = torch.randn(1, 4, H // 2, W_ // 2, generator=g, dtype=ndt).to(bf16)
        zm = pipe.vae.encode_image((x * (mask[None, None] < 0.5)).contiguous(), nchw=True, normalize=False).latents(eps3, scale=sf)
        assert torch.equal(st["masked"], zm) and st["table"] is None
    else:
        assert st["masked"] is None and tuple(st["table"].shape) == (steps + 1, 2)
        # the engine does not encode the masked image for a 4-channel U-Net: the generator stands after draw (2)
        g2 = torch.Generator().manual_seed(21)
        torch.randn(1, 4, H // 2, W_ // 2, generator=g2, dtype=ndt), torch.randn(1, 4, H // 2, W_ // 2, generator=g2, dtype=bf16)


def test_second_call_refreshes_static_inputs_in_place(emulated):
    pipe = _pipe("sd15", 4)
    pipe.scheduler.set_timesteps(10, device="cpu")
    ts, _, _ = get_timesteps(pipe.scheduler, 10, 0.5)
    img = torch.rand(1, 3, 32, 48, generator=torch.Generator().manual_seed(4))
    pipe._inpaint_prepare(img, _rect_mask(32, 48), None, None, None, None, ts[:1], 1, torch.Generator().manual_seed(1), 0.5, True, bf16)
    ptrs = {k: v.data_ptr() for k, v in pipe._inpaint.items() if v is not None}
    pipe._inpaint_prepare(img, 1 - _rect_mask(32, 48), None, None, None, None, ts[:1], 1, torch.Generator().manual_seed(2), 0.5, True, bf16)
    assert ptrs == {k: v.data_ptr() for k, v in pipe._inpaint.items() if v is not None}
    assert torch.equal(pipe._inpaint["mask"][0, 0], (1 - _rect_mask(32, 48))[::2, ::2].to(bf16))


def test_whole_call_on_the_stand_ins(emulated):
    """4-channel SD1.5, eager: mask == 0 everywhere returns the scaled image latents (the last blend row un-noises), and the step
    callback sees the blended latents."""
    pipe = _pipe("sd15", 4)
    g = torch.Generator().manual_seed(3)
    pe, npe = (torch.randn(1, 7, 64, generator=g).to(bf16) for _ in range(2))
    img = torch.rand(1, 3, 32, 32, generator=g)
    seen = []
    out = pipe(image=img, mask_image=torch.zeros(32, 32), strength=0.5, num_inference_steps=10, prompt_embeds=pe,
               negative_prompt_embeds=npe, generator=torch.Generator().manual_seed(5), output_type="latent", use_graph=False,
               callback_on_step_end=lambda p, i, t, d: seen.append(d["latents"].clone()) or {}).images
    assert len(seen) == 5 and torch.equal(out, pipe._inpaint["image_latents"]) and torch.equal(seen[-1], out)
    assert not torch.equal(seen[0], out)                          # after the first step: the image latents at the next noise level


def test_refusals_and_channel_check(emulated):
    pipe9 = _pipe("sdxl", 9)
    img, mask = torch.rand(1, 3, 32, 48), _rect_mask(32, 48)
    pipe9.scheduler.set_timesteps(4, device="cpu")
    ts, _, _ = get_timesteps(pipe9.scheduler, 4, 1.0)
    args = (None, None, None, ts[:1], 1, None, 1.0, True, bf16)
    with pytest.raises(ValueError, match=r"Incorrect configuration settings! .* expects 9 but received `num_channels_latents`: 4 \+ "
                                         r"`num_channels_mask`: 1 \+ `num_channels_masked_image`: 3 = 8"):
        pipe9._inpaint_prepare(img, mask, torch.zeros(1, 3, 16, 24), *args)
    with pytest.raises(NotImplementedError, match="padding_mask_crop"):
        pipe9._inpaint_prepare(img, mask, None, *args, padding_mask_crop=32)
    with pytest.raises(ValueError, match="`mask_image` is 32 x 32 but `image` is 32 x 48"):
        pipe9._inpaint_prepare(img, torch.zeros(32, 32), None, *args)
    with pytest.raises(ValueError, match="31 x 48"):
        pipe9._inpaint_prepare(img[:, :, :31], torch.zeros(31, 48), None, *args)
    with pytest.raises(ValueError, match="does not resize"):
        pipe9._inpaint_prepare(img, mask, None, 64, 96, *args[2:])
    with pytest.raises(ValueError, match="`mask_image` input cannot be undefined"):
        pipe9._inpaint_prepare(img, None, None, *args)
    pipe9.unet.config = type(pipe9.unet.config)(dict(pipe9.unet.config, in_channels=5))
    with pytest.raises(ValueError, match="should have either 4 or 9 input channels, not 5"):
        pipe9._inpaint_prepare(img, mask, None, *args)
    pipe = _pipe("sd15", 4)
    kw = dict(image=img, mask_image=mask, prompt_embeds=torch.zeros(1, 7, 64, dtype=bf16),
              negative_prompt_embeds=torch.zeros(1, 7, 64, dtype=bf16))
    with pytest.raises(NotImplementedError, match="ip_adapter_image"):
        pipe(ip_adapter_image=img, **kw)
    with pytest.raises(NotImplementedError, match="padding_mask_crop"):
        pipe(padding_mask_crop=32, **kw)
    with pytest.raises(ValueError, match="strength"):
        pipe(strength=1.5, **kw)


def test_unet_refuses_inpaint_cond_on_a_4_channel_model(emulated):
    pipe = _pipe("sd15", 4)
    cond = pipe.unet.precompute_conditioning(torch.zeros(1, 7, 64, dtype=bf16), None)
    with pytest.raises(ValueError, match="9 input channels"):
        pipe.unet(torch.zeros(1, 4, 16, 16, dtype=bf16), torch.tensor(1.0), None, conditioning=cond,
                  inpaint_cond=(torch.zeros(1, 1, 16, 16, dtype=bf16), torch.zeros(1, 4, 16, 16, dtype=bf16)))


def test_exports_and_factory():
    import diffusers_amd
    assert diffusers_amd.StableDiffusionInpaintPipeline is StableDiffusionInpaintPipeline
    assert diffusers_amd.StableDiffusionXLInpaintPipeline is StableDiffusionXLInpaintPipeline
    assert _pipe("sdxl", 9).unet.config.in_channels == 9 and _pipe("sd15", 4).unet.config.in_channels == 4
    assert _pipe("sdxl", 9).unet.conv_in_w.shape[1] == 81
    with pytest.raises(ValueError, match="unet_in_channels"):
        _pipe("sdxl", 5)
    import inspect
    sd = inspect.signature(StableDiffusionInpaintPipeline.__call__).parameters
    xl = inspect.signature(StableDiffusionXLInpaintPipeline.__call__).parameters
    assert sd["strength"].default == 1.0 and sd["guidance_scale"].default == 7.5
    assert xl["strength"].default == 0.9999 and xl["guidance_scale"].default == 7.5
    for p in (sd, xl):
        assert all(k in p for k in ("mask_image", "masked_image_latents", "height", "width", "latents", "padding_mask_crop"))
