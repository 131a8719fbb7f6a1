"""CPU: image resizing -- ops.resample_tables through the restated two passes against PIL.Image.resize to the bit, the nearest index
table against F.interpolate, and the pipelines' switch: off, the pinned refusals stand; on, the prepared tensors are Pillow's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import image_resize_emulation as RE
import pix2pix_emulation as PE
from diffusers_amd import _lib as L, factory, ops
from diffusers_amd.pipelines import prepare_control_image, prepare_image, prepare_mask

bf16 = torch.bfloat16
PIL_FILTER = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def _bytes(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


@pytest.fixture
def emulated(monkeypatch):
    PE.install(monkeypatch, ops)
    RE.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "TUNING", False)


@pytest.mark.parametrize("filter", list(PIL_FILTER))
@pytest.mark.parametrize("shape", RE.SHAPES + [((400, 300), (7, 300)), ((667, 1000), (512, 768))], ids=str)
def test_tables_through_the_restated_passes_equal_pillow(shape, filter):
    (hi, wi), (ho, wo) = shape
    for a in (_bytes((hi, wi, 3)), _bytes((hi, wi)), np.indices((hi, wi)).sum(0).astype(np.uint8) % 2 * 255):
        want = np.asarray(Image.fromarray(a).resize((wo, ho), PIL_FILTER[filter]))
        got = RE.resample_u8(torch.from_numpy(a.reshape(1, hi, wi, -1)), (ho, wo), filter)[0].numpy().reshape(want.shape)
        assert np.array_equal(got, want)


def test_nearest_indices_and_entries_without_a_plan_number():
    for i, o in ((5, 16), (37, 16), (1000, 768), (7, 3), (1023, 511), (100, 99)):
        want = F.interpolate(torch.arange(i, dtype=torch.float32)[None, None, None], size=(1, o))[0, 0, 0]
        assert torch.equal(ops.nearest_indices(i, o), want.to(torch.int32))
    for name in ("da_resample_u8", "da_gather_resize"):
        assert name in L.PASS_THROUGH and name not in L.FN_IDS and name not in L.NOT_PLANNABLE


def test_switch_off_keeps_the_pinned_refusals(emulated):
    img = torch.rand(1, 3, 32, 32)
    with pytest.raises(ValueError, match=r"\(the engine does not resize images\)"):
        prepare_control_image(img[:, :, :31], 2, "cpu")
    cn = factory.build_sd15_pipeline(device="cpu", tiny=True, controlnet=True)
    with pytest.raises(ValueError, match="does not resize"):
        cn._arm_controlnet(img, 64, 64, 1.0, False, 0.0, 1.0, 1)
    inp = factory.build_sdxl_pipeline(device="cpu", tiny=True, seed=0, inpaint=True, unet_in_channels=9)
    with pytest.raises(ValueError, match="does not resize"):
        inp._inpaint_prepare(img, torch.zeros(32, 32), None, 64, 96, None, None, 1, None, 1.0, True, bf16)
    p2p = factory.build_sd15_pipeline(device="cpu", tiny=True, seed=0, pix2pix=True)
    with pytest.raises(ValueError, match="does not resize"):
        p2p._prepare_image_latents(img, 64, 64, 1)
    flux = factory.build_flux_pipeline(device="cpu", tiny=True, seed=5, img2img=True)
    with pytest.raises(ValueError, match="does not resize"):
        flux(image=torch.rand(1, 3, 64, 64), height=128, width=64, prompt_embeds=torch.zeros(1, 16, 64, dtype=bf16),
             pooled_prompt_embeds=torch.zeros(1, 64, dtype=bf16), num_inference_steps=4, output_type="latent", use_graph=False,
             max_sequence_length=16)
    for pipe in (cn, inp, p2p, flux):
        assert pipe._resize_spec(None, None) is None
        with pytest.raises(ValueError, match="'lanczos', 'bicubic', 'bilinear'"):
            pipe.enable_image_resize("box")


@pytest.mark.parametrize("filter", ["lanczos", "bicubic"])
def test_switch_on_prepares_what_pillow_resizes(emulated, filter):
    photo, grey = Image.fromarray(_bytes((45, 61, 3), 1)), Image.fromarray(_bytes((45, 61), 2))
    pil = lambda im, h, w: torch.from_numpy(np.array(im.resize((w, h), PIL_FILTER[filter])))  # noqa: E731
    # no size given: the image's own, rounded down to the multiple; a list of PIL images; height / width given
    assert torch.equal(prepare_image(photo, 8, 4, "cpu", (filter, None, None, 8))[1], pil(photo, 40, 56)[None])
    kind, t, nchw, normalize = prepare_image([photo, photo], 8, 4, "cpu", (filter, 32, 64, 8))
    assert (kind, nchw, normalize) == ("image", False, True) and torch.equal(t, torch.stack([pil(photo, 32, 64)] * 2))
    t, nchw = prepare_control_image(photo, 8, "cpu", (filter, 24, 16, 8))
    assert not nchw and torch.equal(t, pil(photo, 24, 16)[None])
    # masks go to "L", are resized, then binarised
    want = (pil(grey, 40, 56).float() / 255.0 >= 0.5).float()[None, None]
    assert torch.equal(prepare_mask(grey, 8, "cpu", (filter, 40, 56)), want)
    # tensors and arrays: nearest, as F.interpolate
    x = torch.rand(2, 3, 45, 61)
    assert torch.equal(prepare_image(x, 8, 4, "cpu", (filter, None, 48, 8))[1], F.interpolate(x, size=(40, 48)))
    a = _bytes((45, 61, 3), 3)
    want = F.interpolate(torch.from_numpy(a).permute(2, 0, 1)[None].float(), size=(40, 56))[0].permute(1, 2, 0).to(torch.uint8)
    assert torch.equal(prepare_image(a, 8, 4, "cpu", (filter, None, None, 8))[1][0], want)
    m = torch.rand(45, 61)
    assert torch.equal(prepare_mask(m, 8, "cpu", (filter, 40, 56)), (F.interpolate(m[None, None], size=(40, 56)) >= 0.5).float())
    # still refused, by name
    with pytest.raises(ValueError, match="taken as latents, which are not resized"):
        prepare_image(torch.zeros(1, 4, 8, 8), 8, 4, "cpu", (filter, None, None, 8))
    with pytest.raises(ValueError, match="`height` = 36.*multiples of 8"):
        prepare_image(photo, 8, 4, "cpu", (filter, 36, 64, 8))
    # through the pipelines: the control image goes to the output size, FLUX rounds to twice the factor
    cn = factory.build_sd15_pipeline(device="cpu", tiny=True, controlnet=True)
    cn.enable_image_resize(filter)
    f = cn.vae_scale_factor
    assert cn._arm_controlnet(photo, None, None, 1.0, False, 0.0, 1.0, 1) == (45 - 45 % f, 61 - 61 % f)
    assert torch.equal(cn._cn_call[0], pil(photo, 45 - 45 % f, 61 - 61 % f)[None])
    flux = factory.build_flux_pipeline(device="cpu", tiny=True, seed=5, img2img=True)
    flux.enable_image_resize(filter)
    assert flux._resize_spec(None, 64) == (filter, None, 64, 2 * flux.vae_scale_factor)
