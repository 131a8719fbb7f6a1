"""Tiled / sliced AutoencoderKL.decode, the parts that need no GPU: the blend arithmetic against torch's own bf16 ops, the host
tiling logic of AutoencoderKL (run on the torch stand-in of the tile-blend op and a stand-in decoder) against a literal
transcription of the reference's tiled_decode, the tile grid against hand-written lists, the refusals, the attribute surface of the
VAE and of the pipelines, and the ABI facts of da_vae_tile_blend."""
from __future__ import annotations

import inspect
import re
from pathlib import Path

import pytest
import torch

import vae_tiling_emulation as VE
from diffusers_amd import _lib as L
from diffusers_amd import init as dinit
from diffusers_amd import ops
from diffusers_amd import pipelines as P
from diffusers_amd.autoencoder_kl import AutoencoderKL
from diffusers_amd.autoencoder_kl_wan import AutoencoderKLWan
from diffusers_amd.autoencoder_tiny import AutoencoderTiny

bf16 = torch.bfloat16
HEADER = (Path(__file__).resolve().parents[1] / "include" / "diffusers_amd.h").read_text()
# two decoder stages (2 x), sample_size 16: tl = 8 latent / 16 px, overlap_size 6, blend_extent 4, row_limit 12
SMALL_VAE = dict(dinit.TINY_VAE, sample_size=16)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ---- the arithmetic ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 3, 5, 8, 12, 128])
def test_emulated_blend_equals_torch_bf16_ops_to_the_bit(E):
    g = torch.Generator().manual_seed(E)
    n = 4096
    a = (torch.randn(n, generator=g) * 3).to(bf16)
    b = (torch.randn(n, generator=g) * 3).to(bf16)
    a[:4] = torch.tensor([0.0, -0.0, 3.3895313892515355e38, -1e-40]).to(bf16)      # zeros, bf16 max, a denormal
    wt = VE.weights(E)
    assert wt.shape == (E, 2) and wt.dtype == torch.float32
    for y in range(E):
        ref = a * (1 - y / E) + b * (y / E)                     # the reference's line, torch's own bf16 ops
        assert same_bits(VE.blend(a, b, wt[y, 0], wt[y, 1]), ref), (E, y)


def test_fp32_evaluated_weights_are_not_the_table():
    """1.0f - (float)y / E differs from float32(1 - y / E) for some E that is no power of two: why the table comes from float64."""
    differ = 0
    for E in (3, 5, 7, 12, 24, 96):
        wt = VE.weights(E)
        for y in range(E):
            f32 = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(float(y), dtype=torch.float32) / torch.tensor(float(E), dtype=torch.float32)
            differ += int(f32.item() != wt[y, 0].item())
    assert differ > 0
    assert torch.equal(ops.tile_blend_weights(12, "cpu"), VE.weights(12))
    assert ops.tile_blend_weights(12, "cpu") is ops.tile_blend_weights(12, "cpu")          # cached per E
    with pytest.raises(ValueError):
        ops.tile_blend_weights(0, "cpu")


# ---- the host tiling logic on stand-ins ---------------------------------------------------------------------------------
def standin_vae(monkeypatch, cfg=SMALL_VAE, **attrs):
    """An AutoencoderKL without weights whose per-tile decoder is VE.standin_decoder and whose tile-blend op is the torch stand-in."""
    vae = AutoencoderKL(**cfg)
    vae._built = True
    for k, v in attrs.items():
        setattr(vae, k, v)
    C = vae.config.out_channels
    dec = VE.standin_decoder(2 ** (len(vae.config.block_out_channels) - 1), C)
    calls = {"tile": [], "whole": []}

    def decode_tile(z, div, add):
        calls["tile"].append(tuple(z.shape))
        y = dec(z)
        return y, (C * y.shape[2] * y.shape[3], y.shape[2] * y.shape[3], 1)

    def decode_whole(z, div, add, pp):
        calls["whole"].append(tuple(z.shape))
        return VE.postprocess_image(dec(z), pp)

    vae._decode_tile, vae._decode = decode_tile, decode_whole
    monkeypatch.setattr(ops, "vae_tile_blend", VE.vae_tile_blend)
    monkeypatch.setattr(ops, "require_hip", lambda *a, **k: None)
    return vae, dec, calls


def latents(B, H, W, seed=0, L_=4):
    return torch.randn(B, L_, H, W, generator=torch.Generator().manual_seed(seed)).to(bf16)


GRIDS = [(8, 8), (9, 9), (16, 16), (13, 20), (8, 20)]      # = tl (untiled), tl + 1, 2 tl, short upper tile + 1-row last tile, wide


@pytest.mark.parametrize("mode", VE.MODES)
@pytest.mark.parametrize("H,W", GRIDS)
def test_host_tiling_equals_the_transcribed_reference(monkeypatch, H, W, mode):
    vae, dec, calls = standin_vae(monkeypatch)
    vae.enable_tiling()
    z = latents(2, H, W, seed=H * 100 + W)
    got = vae.decode(z, postprocess=mode).sample
    if H <= 8 and W <= 8:
        assert calls["tile"] == [] and calls["whole"] == [(2, 4, H, W)]
        want = VE.postprocess_image(dec(z), mode)
    else:
        assert calls["whole"] == []
        want = VE.postprocess_image(VE.reference_tiled_decode(z, dec, tile_latent_min_size=8, tile_sample_min_size=16), mode)
    assert same_bits(got, want)
    assert vae.decode(z, return_dict=False, postprocess=mode)[0].shape == want.shape


def test_short_upper_tile_blends_rows_that_do_not_line_up(monkeypatch):
    """Latent height 13 with tl 8: tiles of 8, 7 and 1 rows.  The last tile's two pixel rows blend with rows -4, -3 of the 14-row
    tile above it (its rows 10, 11), although only its rows 12, 13 overlap them geometrically -- the reference's a[-E + y]."""
    vae, dec, _ = standin_vae(monkeypatch)
    vae.enable_tiling()
    z = latents(1, 13, 8, seed=5)
    E, rows, IH, IW = vae._tile_plan(13, 8)
    assert [r[0]["h"] for r in rows] == [16, 14, 2] and E == 4
    got = vae.decode(z).sample
    mid = dec(z[:, :, 6:14]).clone()
    VE.blend_v(dec(z[:, :, 0:8]), mid, 4)
    last = dec(z[:, :, 12:13]).clone()
    wt = VE.weights(4)
    for y in range(2):
        want = VE.blend(mid[:, :, 10 + y, :12], last[:, :, y, :12], wt[y, 0], wt[y, 1])
        assert same_bits(got[:, :, 24 + y, :12], want)


def plan_lists(vae, H, W):
    E, rows, IH, IW = vae._tile_plan(H, W)
    return (E, [[(t["i"], t["j"], t["lh"], t["lw"]) for t in r] for r in rows],
            [[(t["y0"], t["x0"], t["keep_h"], t["keep_w"]) for t in r] for r in rows], (IH, IW))


def test_tile_grid_and_piece_positions():
    vae = AutoencoderKL(**SMALL_VAE)
    assert plan_lists(vae, 9, 9) == (4, [[(0, 0, 8, 8), (0, 6, 8, 3)], [(6, 0, 3, 8), (6, 6, 3, 3)]],
                                     [[(0, 0, 12, 12), (0, 12, 12, 6)], [(12, 0, 6, 12), (12, 12, 6, 6)]], (18, 18))
    E, tiles, pieces, size = plan_lists(vae, 16, 16)
    assert E == 4 and size == (32, 32)
    assert [t[0] for t in tiles] == [(0, 0, 8, 8), (6, 0, 8, 8), (12, 0, 4, 8)] and tiles[0] == [(0, 0, 8, 8), (0, 6, 8, 8), (0, 12, 8, 4)]
    assert [p[0] for p in pieces] == [(0, 0, 12, 12), (12, 0, 12, 12), (24, 0, 8, 12)] and pieces[2] == [(24, 0, 8, 12), (24, 12, 8, 12), (24, 24, 8, 8)]
    E, tiles, pieces, size = plan_lists(vae, 13, 20)
    assert size == (26, 40)
    assert [t[0][:3:2] for t in tiles] == [(0, 8), (6, 7), (12, 1)]                       # (i, lh): 8, 7 and 1 latent rows
    assert [t[1::2] for t in tiles[0]] == [(0, 8), (6, 8), (12, 8), (18, 2)]              # (j, lw)
    assert [p[0][0::2] for p in pieces] == [(0, 12), (12, 12), (24, 2)]                   # (y0, keep_h)
    assert [p[1::2] for p in pieces[0]] == [(0, 12), (12, 12), (24, 12), (36, 4)]         # (x0, keep_w)
    E, tiles, pieces, size = plan_lists(vae, 8, 20)
    assert size == (16, 40) and [t[0][:3:2] for t in tiles] == [(0, 8), (6, 2)] and [p[0][0::2] for p in pieces] == [(0, 12), (12, 4)]


def test_only_tiles_with_a_later_reader_keep_their_blended_copy(monkeypatch):
    vae, _, _ = standin_vae(monkeypatch)
    vae.enable_tiling()
    seen = []
    real = VE.vae_tile_blend

    def spy(src, strides, **kw):
        seen.append((kw["y0"], kw["x0"], kw["up"] is not None, kw["left"] is not None, kw["want_fin"], kw["extent"]))
        return real(src, strides, **kw)

    monkeypatch.setattr(ops, "vae_tile_blend", spy)
    vae.decode(latents(1, 9, 9))
    assert seen == [(0, 0, False, False, True, 4), (0, 12, False, True, True, 4), (12, 0, True, False, True, 4), (12, 12, True, True, False, 4)]


def test_refusals_name_the_attribute():
    vae = AutoencoderKL(**SMALL_VAE)
    vae.tile_overlap_factor = 0.9                             # int(8 * 0.1) = 0
    with pytest.raises(ValueError, match=r"tile_latent_min_size = 8 with tile_overlap_factor = 0.9 gives overlap_size = 0"):
        vae._tile_plan(20, 20)
    vae.tile_overlap_factor = 0.25
    vae.tile_latent_min_size = 1                              # int(0.75) = 0
    with pytest.raises(ValueError, match="tile_latent_min_size = 1"):
        vae._tile_plan(20, 20)
    vae.tile_latent_min_size = 8
    vae.tile_sample_min_size = 128                            # blend_extent 32 > the 16 pixel rows of a full tile
    with pytest.raises(ValueError, match=r"tile_sample_min_size = 128 .* blend_extent = 32"):
        vae._tile_plan(20, 20)
    vae.tile_sample_min_size = 16
    assert vae._tile_plan(20, 20)[0] == 4


def test_attribute_defaults():
    sdxl = AutoencoderKL(**dinit.SDXL_VAE)
    assert (sdxl.tile_sample_min_size, sdxl.tile_latent_min_size, sdxl.tile_overlap_factor) == (1024, 128, 0.25)
    tiny = AutoencoderKL(**dinit.TINY_VAE)
    assert (tiny.tile_sample_min_size, tiny.tile_latent_min_size, tiny.tile_overlap_factor) == (32, 16, 0.25)
    assert AutoencoderKL(**dict(dinit.TINY_VAE, sample_size=[64, 48])).tile_sample_min_size == 64
    for v in (sdxl, tiny):
        assert v.use_tiling is False and v.use_slicing is False
        v.enable_tiling(); assert v.use_tiling is True
        v.enable_tiling(False); assert v.use_tiling is False
        v.enable_tiling(); v.disable_tiling(); assert v.use_tiling is False
        v.enable_slicing(); assert v.use_slicing is True
        v.disable_slicing(); assert v.use_slicing is False
    sig = inspect.signature(AutoencoderKL.decode)
    assert list(sig.parameters) == ["self", "z", "return_dict", "generator", "latents_div", "latents_add", "postprocess"]


@pytest.mark.parametrize("mode", VE.MODES)
@pytest.mark.parametrize("H,W,tiling", [(8, 8, False), (13, 20, True), (8, 8, True)])
def test_slicing_decodes_sample_by_sample_into_one_output(monkeypatch, H, W, tiling, mode):
    vae, dec, calls = standin_vae(monkeypatch)
    vae.enable_slicing()
    vae.enable_tiling(tiling)
    z = latents(3, H, W, seed=9)
    got = vae.decode(z, postprocess=mode).sample
    singles = []
    vae.disable_slicing()
    for b in range(3):
        singles.append(vae.decode(z[b:b + 1], postprocess=mode).sample)
    assert same_bits(got, torch.cat(singles, 0))
    if tiling and (H > 8 or W > 8):
        assert calls["whole"] == [] and all(s[0] == 1 for s in calls["tile"])
    else:
        assert calls["whole"][:3] == [(1, 4, H, W)] * 3
    # a single sample is not sliced
    vae.enable_slicing()
    n = len(calls["whole"]) + len(calls["tile"])
    vae.enable_tiling(False)
    vae.decode(z[:1], postprocess=mode)
    assert calls["whole"][-1] == (1, 4, H, W) and len(calls["whole"]) + len(calls["tile"]) == n + 1


# ---- pipelines ----------------------------------------------------------------------------------------------------------
VAE_PIPELINES = [c for _, c in inspect.getmembers(P, inspect.isclass)
                 if c.__module__ == P.__name__ and c.__name__.endswith("Pipeline") and "vae" in inspect.signature(c.__init__).parameters]


def test_the_pipeline_list_is_not_empty():
    names = {c.__name__ for c in VAE_PIPELINES}
    assert {"StableDiffusionPipeline", "StableDiffusionXLPipeline", "StableDiffusionXLImg2ImgPipeline", "StableDiffusionXLInpaintPipeline",
            "StableDiffusionXLControlNetPipeline", "StableDiffusionXLInstructPix2PixPipeline", "FluxPipeline", "FluxImg2ImgPipeline",
            "FluxInpaintPipeline", "WanPipeline"} <= names and "DDPMPipeline" not in names


@pytest.mark.parametrize("cls", VAE_PIPELINES, ids=lambda c: c.__name__)
def test_pipeline_methods_flip_the_flags_of_the_vae(cls):
    pipe = object.__new__(cls)
    pipe.vae = AutoencoderKL(**dinit.TINY_VAE)
    pipe.enable_vae_tiling(); assert pipe.vae.use_tiling is True and pipe.vae.use_slicing is False
    pipe.disable_vae_tiling(); assert pipe.vae.use_tiling is False
    pipe.enable_vae_slicing(); assert pipe.vae.use_slicing is True and pipe.vae.use_tiling is False
    pipe.disable_vae_slicing(); assert pipe.vae.use_slicing is False


@pytest.mark.parametrize("vae_cls,cfg", [(AutoencoderTiny, dinit.TINY_TAESD), (AutoencoderKLWan, dinit.TINY_WAN_VAE)])
def test_a_vae_without_tiling_is_refused_by_name(vae_cls, cfg):
    pipe = object.__new__(P.WanPipeline if vae_cls is AutoencoderKLWan else P.StableDiffusionXLPipeline)
    pipe.vae = vae_cls(**cfg)
    for m in ("enable_vae_tiling", "disable_vae_tiling", "enable_vae_slicing", "disable_vae_slicing"):
        with pytest.raises(NotImplementedError, match=vae_cls.__name__):
            getattr(pipe, m)()


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_facts():
    name = "da_vae_tile_blend"
    assert re.search(r"^int da_vae_tile_blend\(const void\* src, long long sB, long long sC, long long sP, const void\* up, int hu, "
                     r"const void\* left, int wl,\s+const void\* weights, int E, void\* fin, void\* image, int B, int C, int h, int w, "
                     r"int keep_h, int keep_w,\s+long long image_h, long long image_w, long long y0, long long x0, int mode, "
                     r"void\* stream\);", HEADER, re.M)
    _i, _ll, _vp = L._i, L._ll, L._vp
    assert L.SIGNATURES[name] == (_i, [_vp, _ll, _ll, _ll, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _ll, _ll, _ll,
                                       _ll, _i, _vp])
    assert name in L.PASS_THROUGH and name not in L.FN_IDS and name not in L.NOT_PLANNABLE
    assert list(L.PASS_THROUGH).index(name) == list(L.PASS_THROUGH).index("da_tiny_vae_latents_in") + 1
    assert "ops.vae_tile_blend refuses under a recording" in L.PASS_THROUGH[name]
    assert re.search(r"^#define DA_ABI_VERSION 9\b", HEADER, re.M) and L.ABI_VERSION == 9 and L.FN_COUNT == 36


def test_tile_blend_wrapper_refuses_under_a_recording(monkeypatch):
    monkeypatch.setattr(L._tls, "recorder", object(), raising=False)
    with pytest.raises(RuntimeError, match="not replayable by a launch plan"):
        ops.vae_tile_blend(torch.zeros(12, dtype=bf16), (12, 4, 1), batch=1, channels=3, height=2, width=2,
                           image=torch.zeros(1, 3, 2, 2, dtype=bf16), y0=0, x0=0, keep_h=2, keep_w=2)


def test_conv_thin_out_tile_is_for_image_channel_counts_only():
    with pytest.raises(ValueError, match="at most 4 output channels"):
        ops.conv_thin_out_tile(torch.zeros(1, 2, 2, 64, dtype=bf16), torch.zeros(8, 576, dtype=bf16), None)
