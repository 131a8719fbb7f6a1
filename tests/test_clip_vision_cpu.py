"""CPU: the host side of the CLIP vision encoder -- the packed patch weight, ``state_dict`` keys, CLIPImageProcessor's geometry and pixel
rounding, and the ABI facts of da_clip_patch_embed."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

bf16 = torch.bfloat16
CFG = dict(hidden_size=128, intermediate_size=256, projection_dim=64, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14)


def test_patch_weight_keeps_the_c_i_j_order_and_pads_with_zeros():
    from diffusers_amd import ops
    w = torch.arange(4 * 3 * 14 * 14, dtype=torch.float32).reshape(4, 3, 14, 14).remainder(251).to(bf16)
    p = ops.pack_clip_patch_weight(w)
    assert p.shape == (4, 608) and p.dtype == bf16 and not bool(p[:, 588:].any())
    assert p[2, (1 * 14 + 5) * 14 + 9] == w[2, 1, 5, 9] and torch.equal(p[:, :588], w.reshape(4, 588))
    assert ops.pack_clip_patch_weight(torch.zeros(8, 3, 16, 16, dtype=bf16)).shape == (8, 768)


@pytest.mark.parametrize("prefix", ["vision_model.", ""])
def test_state_dict_keys_with_and_without_the_prefix(prefix):
    from diffusers_amd import init as dinit
    from diffusers_amd.vision_encoders import CLIPVisionModelWithProjection, clip_vision_param_shapes
    import transformers
    shapes = clip_vision_param_shapes(CFG)
    theirs = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**CFG)).state_dict()
    assert {k: tuple(v.shape) for k, v in theirs.items()} == shapes
    sd = {k.replace("vision_model.", prefix): v for k, v in dinit.random_state_dict(shapes, seed=1).items()}
    m = CLIPVisionModelWithProjection(CFG).load_state_dict(sd, device="cpu")
    assert m.patch_w.shape == (128, 608) and len(m.layers) == 1 and m.visual_projection.shape == (64, 128)
    with pytest.raises(RuntimeError, match="unexpected keys"):
        CLIPVisionModelWithProjection(CFG).load_state_dict(dict(sd, stray=torch.zeros(1)), device="cpu")
    with pytest.raises(KeyError, match="pre_layrnorm"):
        CLIPVisionModelWithProjection(CFG).load_state_dict({k: v for k, v in sd.items() if "pre_layrnorm.weight" not in k}, device="cpu")


@pytest.mark.parametrize("h,w", [(300, 200), (200, 300), (224, 224), (57, 1001), (640, 481)])
def test_resize_and_crop_geometry_is_the_image_processors(h, w):
    from transformers.image_transforms import center_crop, get_resize_output_image_size
    from diffusers_amd.vision_encoders import resize_crop_geometry
    size, (top, left) = resize_crop_geometry(h, w, 56)
    assert size == tuple(get_resize_output_image_size(np.zeros((h, w, 3), np.uint8), size=56, default_to_square=False, input_data_format="channels_last"))
    marked = np.arange(size[0] * size[1], dtype=np.float32).reshape(size[0], size[1], 1).repeat(3, 2)
    want = center_crop(marked, (56, 56), input_data_format="channels_last", data_format="channels_last")
    assert np.array_equal(want, marked[top:top + 56, left:left + 56])


@pytest.mark.parametrize("h,w", [(300, 200), (200, 300)])
def test_the_kernels_pixel_rounds_to_the_image_processors_bf16(h, w):
    """fp32 ``(u8 / 255 - mean) * inv_std`` and CLIPImageProcessor's pixel_values may differ in the last fp32 bit; rounded to bf16 (the
    MFMA operand of either mode) they are the same for the images tests/test_clip_vision_gpu.py compares to the bit."""
    from PIL import Image
    from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil
    from diffusers_amd.vision_encoders import CLIP_IMAGE_MEAN, CLIP_IMAGE_STD, resize_crop_geometry
    g = torch.Generator("cpu").manual_seed(h)
    img = Image.fromarray(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy())
    pv = CLIPImageProcessorPil(size={"shortest_edge": 56}, crop_size={"height": 56, "width": 56})(images=img, return_tensors="pt").pixel_values
    (nh, nw), (top, left) = resize_crop_geometry(h, w, 56)
    u8 = torch.from_numpy(np.asarray(img.resize((nw, nh), Image.BICUBIC))[top:top + 56, left:left + 56].copy()).float()
    inv = torch.tensor([1.0 / s for s in CLIP_IMAGE_STD], dtype=torch.float32)
    mine = ((u8 / 255.0 - torch.tensor(CLIP_IMAGE_MEAN)) * inv).permute(2, 0, 1)
    assert float((mine - pv[0]).abs().max()) <= 2.0 ** -22 and torch.equal(mine.to(bf16), pv[0].to(bf16))


def test_abi_facts_of_the_new_entry():
    import diffusers_amd as da
    from diffusers_amd import _lib as L
    header = re.sub(r"/\*.*?\*/", "", (Path(da.__file__).parent.parent / "include" / "diffusers_amd.h").read_text(), flags=re.S)
    proto = re.search(r"int da_clip_patch_embed\((.*?)\);", header, flags=re.S).group(1)
    params = [" ".join(p.split()) for p in proto.split(",")]
    assert params[0] == "const void* image" and params[-1] == "void* stream" and len(params) == len(L.SIGNATURES["da_clip_patch_embed"][1])
    letters = {"int": L._i, "float": L._f}
    assert [letters.get(p.rsplit(" ", 1)[0], L._vp) for p in params] == L.SIGNATURES["da_clip_patch_embed"][1]
    assert "da_clip_patch_embed" in L.PASS_THROUGH and "da_clip_patch_embed" not in L.FN_IDS and L.ABI_VERSION == 9
    assert "CLIPVisionModelWithProjection" in da.__all__ and da.CLIPVisionModelWithProjection.__module__ == "diffusers_amd.vision_encoders"
