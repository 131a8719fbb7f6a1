"""Tiled / sliced AutoencoderKL.encode, the parts that need no GPU: the arithmetic of da_vae_moments_tile_blend against torch's own
bf16 ops, the tile grid against hand-written lists, the host tiling logic of AutoencoderKL (run on the torch stand-in of the op and a
stand-in encoder) against a literal transcription of the reference's _tiled_encode / encode, the refusals, the attribute surface,
the ABI facts, and the eight image-reading pipelines reaching the tiled path on the CPU stand-ins of the other kernels."""
from __future__ import annotations

import inspect
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import flux_img2img_emulation as FE
import pix2pix_emulation as PE
import vae_tiled_encode_emulation as TE
import vae_tiling_emulation as VE
from diffusers_amd import _lib as L
from diffusers_amd import factory
from diffusers_amd import init as dinit
from diffusers_amd import ops
from diffusers_amd import pipelines as P
from diffusers_amd.autoencoder_kl import AutoencoderKL, DiagonalGaussianDistribution
from diffusers_amd.autoencoder_kl_wan import AutoencoderKLWan
from diffusers_amd.autoencoder_tiny import AutoencoderTiny

bf16 = torch.bfloat16
HEADER = (Path(__file__).resolve().parents[1] / "include" / "diffusers_amd.h").read_text()
# two encoder stages (1 / 2), tiles of 16 px = 8 latent: overlap_size 12 px, blend extent 2, row_limit 6
SMALL_VAE = dict(dinit.TINY_VAE, sample_size=16)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


# ---- the arithmetic ----------------------------------------------------------------------------------------------------
def _exact_operands(C, B, h, w, seed):
    """Operands whose fp32 channel sum is exact in ANY order (multiples of 1/8 below 8 times multiples of 1/16 below 2: every partial
    sum is a multiple of 1/128 below 2^11), so F.conv2d's accumulation order cannot matter and one rounding to bf16 remains."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(-63, 64, (B, C, h, w), generator=g).float() / 8).to(bf16)
    wq = (torch.randint(-31, 32, (C, C), generator=g).float() / 16).to(bf16)
    bq = (torch.randint(-31, 32, (C,), generator=g).float() / 16).to(bf16)
    return x, wq, bq


@pytest.mark.parametrize("C", [8, 32])
def test_quant_conv_restatement_equals_torch_bf16_conv2d_to_the_bit(C):
    x, wq, bq = _exact_operands(C, 2, 9, 13, C)
    want = F.conv2d(x, wq.view(C, C, 1, 1), bq)
    assert want.dtype == bf16 and same_bits(TE.quant_conv(x, wq, bq), want)
    assert same_bits(TE.quant_conv(x, None, None), x)


@pytest.mark.parametrize("E", [1, 2, 3, 8])
@pytest.mark.parametrize("quant", [True, False])
def test_standin_op_equals_torch_bf16_ops_to_the_bit(E, quant):
    """quant_conv (F.conv2d in bf16), blend_v, then blend_h on its result -- the reference's lines with torch's own bf16 ops -- against
    the stand-in of the op, from every source layout, with neighbours of another size than the tile."""
    B, C, h, w, hu, wl = 2, 8, 9, 7, E + 2, E + 1
    x, wq, bq = _exact_operands(C, B, h, w, E)
    g = torch.Generator().manual_seed(100 + E)
    up = (torch.randn(B, C, hu, w, generator=g) * 3).to(bf16)
    left = (torch.randn(B, C, h, wl, generator=g) * 3).to(bf16)
    tile = F.conv2d(x, wq.view(C, C, 1, 1), bq) if quant else x.clone()
    tile = VE.blend_v(up, tile, E)
    tile = VE.blend_h(left, tile, E)
    for layout in TE.LAYOUTS:
        src, strides = TE.layout_source(x, layout)
        moments = torch.full((B, C, 12, 11), 5.0, dtype=bf16)
        fin = TE.vae_moments_tile_blend(src, strides, batch=B, latent_channels=C // 2, height=h, width=w, moments=moments, y0=2, x0=3,
                                        keep_h=6, keep_w=5, wq=wq if quant else None, bq=bq if quant else None, extent=E, up=up,
                                        left=left)
        assert same_bits(fin, tile), layout
        want = torch.full((B, C, 12, 11), 5.0, dtype=bf16)
        want[:, :, 2:8, 3:8] = tile[:, :, :6, :5]
        assert same_bits(moments, want), layout


# ---- the tile grid --------------------------------------------------------------------------------------------------------
def plan_lists(vae, H, W):
    E, rows, Hl, Wl = vae._encode_tile_plan(H, W)
    return (E, [[(t["i"], t["j"], t["ph"], t["pw"]) for t in r] for r in rows], [[(t["h"], t["w"]) for t in r] for r in rows],
            [[(t["y0"], t["x0"], t["keep_h"], t["keep_w"]) for t in r] for r in rows], (Hl, Wl))


def test_tile_grid_and_piece_positions():
    vae = AutoencoderKL(**SMALL_VAE)
    assert (vae.tile_sample_min_size, vae.tile_latent_min_size) == (16, 8)
    # 18 x 18 px: 2 x 2 tiles, the last ones a single latent line
    assert plan_lists(vae, 18, 18) == (2, [[(0, 0, 16, 16), (0, 12, 16, 6)], [(12, 0, 6, 16), (12, 12, 6, 6)]],
                                       [[(8, 8), (8, 3)], [(3, 8), (3, 3)]],
                                       [[(0, 0, 6, 6), (0, 6, 6, 3)], [(6, 0, 3, 6), (6, 6, 3, 3)]], (9, 9))
    # 26 x 40 px: tiles of 16, 14 and 2 px down (8, 7 and ONE latent line), 16, 16, 16 and 4 px across
    E, tiles, sizes, pieces, size = plan_lists(vae, 26, 40)
    assert E == 2 and size == (13, 20)
    assert [t[0][0::2] for t in tiles] == [(0, 16), (12, 14), (24, 2)] and [s[0][0] for s in sizes] == [8, 7, 1]
    assert [t[1::2] for t in tiles[0]] == [(0, 16), (12, 16), (24, 16), (36, 4)] and [s[1] for s in sizes[0]] == [8, 8, 8, 2]
    assert [p[0][0::2] for p in pieces] == [(0, 6), (6, 6), (12, 1)]                      # (y0, keep_h)
    assert [p[1::2] for p in pieces[2]] == [(0, 6), (6, 6), (12, 6), (18, 2)]             # (x0, keep_w)
    # tiles of 24 px = 12 latent: overlap_size 18, E = 3 (weights 1/3, 2/3: no powers of two), row_limit 9
    vae.tile_sample_min_size, vae.tile_latent_min_size = 24, 12
    E, tiles, sizes, pieces, size = plan_lists(vae, 40, 28)
    assert E == 3 and size == (20, 14)
    assert [t[0][0::2] for t in tiles] == [(0, 24), (18, 22), (36, 4)] and [s[0][0] for s in sizes] == [12, 11, 2]
    assert [t[1::2] for t in tiles[0]] == [(0, 24), (18, 10)] and [s[1] for s in sizes[0]] == [12, 5]
    assert [p[0][0::2] for p in pieces] == [(0, 9), (9, 9), (18, 2)] and [p[1::2] for p in pieces[0]] == [(0, 9), (9, 5)]
    vae.tile_sample_min_size, vae.tile_latent_min_size = 16, 8
    # factor 0: the tiles abut, nothing blends, whole tiles are kept
    vae.tile_overlap_factor = 0.0
    E, tiles, sizes, pieces, size = plan_lists(vae, 32, 40)
    assert E == 0 and size == (16, 20) and [t[0][0::2] for t in tiles] == [(0, 16), (16, 16)]
    assert [t[1::2] for t in tiles[0]] == [(0, 16), (16, 16), (32, 8)] and [p[1::2] for p in pieces[1]] == [(0, 8), (8, 8), (16, 4)]
    # factor 0.5: overlap_size 8, E = 4, row_limit 4
    vae.tile_overlap_factor = 0.5
    E, tiles, sizes, pieces, size = plan_lists(vae, 24, 20)
    assert E == 4 and size == (12, 10)
    assert [t[0][0::2] for t in tiles] == [(0, 16), (8, 16), (16, 8)] and [t[1::2] for t in tiles[0]] == [(0, 16), (8, 12), (16, 4)]
    assert [p[0][0::2] for p in pieces] == [(0, 4), (4, 4), (8, 4)] and [p[1::2] for p in pieces[0]] == [(0, 4), (4, 4), (8, 2)]


# ---- the host tiling logic on stand-ins ---------------------------------------------------------------------------------
def standin_vae(monkeypatch, cfg=SMALL_VAE, *, quant=True, layout="nchw", **attrs):
    """An AutoencoderKL without weights whose encoder is TE.StandinEncoder and whose tile op is the torch stand-in."""
    vae = AutoencoderKL(**cfg)
    vae._built = True
    for k, v in attrs.items():
        setattr(vae, k, v)
    enc = TE.StandinEncoder(vae.config.latent_channels, 2 ** (len(vae.config.block_out_channels) - 1), quant, layout)
    vae.encoder = enc
    seen = []

    def op(src, strides, **kw):
        seen.append(dict(kw, strides=tuple(strides)))
        return TE.vae_moments_tile_blend(src, strides, **kw)

    monkeypatch.setattr(ops, "vae_moments_tile_blend", op)
    monkeypatch.setattr(ops, "require_hip", lambda *a, **k: None)
    return vae, enc, seen


def image01(B, H, W, seed=0):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


def transcribed(vae, enc, src, nchw, normalize, tiling, slicing):
    return TE.reference_encode(src, lambda t: enc.moments(t, nchw, normalize), use_tiling=tiling, use_slicing=slicing,
                               tile_sample_min_size=vae.tile_sample_min_size, tile_latent_min_size=vae.tile_latent_min_size,
                               tile_overlap_factor=vae.tile_overlap_factor, nchw=nchw)


SIZES = [(18, 18), (40, 28), (26, 40), (32, 16)]


@pytest.mark.parametrize("source", TE.SOURCES)
@pytest.mark.parametrize("B,slicing", [(1, False), (2, False), (2, True)])
@pytest.mark.parametrize("cfg,quant", [(SMALL_VAE, True), (SMALL_VAE, False), (dict(dinit.TINY_FLUX_VAE, sample_size=16), False)],
                         ids=["L4_quant", "L4_plain", "L16"])
def test_host_tiling_equals_the_transcribed_reference(monkeypatch, cfg, quant, B, slicing, source):
    for n, (H, W) in enumerate(SIZES):
        layouts = TE.LAYOUTS if cfg["latent_channels"] == 4 else ("nchw", "nhwc")     # (16 padded channels cannot hold 32)
        layout = layouts[(n + B + len(source)) % len(layouts)]
        vae, enc, seen = standin_vae(monkeypatch, cfg, quant=quant, layout=layout)
        vae.enable_tiling()
        if slicing:
            vae.enable_slicing()
        nchw, normalize = source == "f32_nchw", (n + B) % 2 == 0
        src = TE.image_source(image01(B, H, W, seed=H * 100 + W), source)
        dist = vae.encode_image(src, nchw=nchw, normalize=normalize)
        want = transcribed(vae, enc, src, nchw, normalize, True, slicing)
        Lc = vae.config.latent_channels
        assert tuple(want.shape) == (B, 2 * Lc, H // 2, W // 2)
        assert isinstance(dist, DiagonalGaussianDistribution) and same_bits(dist.parameters, want), (H, W, layout)
        assert dist.latent_shape == (B, Lc, H // 2, W // 2) and dist._strides == (2 * Lc * (H // 2) * (W // 2), (H // 2) * (W // 2), 1)
        assert dist._wq is None and dist._bq is None                              # no quant_conv left to apply
        assert same_bits(dist.mean, want[:, :Lc]) and same_bits(dist.logvar, torch.clamp(want[:, Lc:], -30.0, 20.0))
        assert all(s["batch"] == (1 if slicing else B) for s in seen) and all((s["wq"] is not None) == quant for s in seen)
        E, rows, _, _ = vae._encode_tile_plan(H, W)
        assert len(seen) == (B if slicing else 1) * sum(len(r) for r in rows) and all(s["extent"] == E for s in seen)


def test_nonpower_of_two_weights_and_other_factors(monkeypatch):
    for S, tl, factor in ((24, 12, 0.25), (16, 8, 0.0), (16, 8, 0.5)):
        vae, enc, seen = standin_vae(monkeypatch, tile_sample_min_size=S, tile_latent_min_size=tl, tile_overlap_factor=factor)
        vae.enable_tiling()
        src = image01(1, 40, 52, seed=S)
        want = transcribed(vae, enc, src, True, True, True, False)
        assert same_bits(vae.encode_image(src, nchw=True, normalize=True).parameters, want), (S, factor)
        assert tuple(want.shape) == (1, 8, 20, 26) and {s["extent"] for s in seen} == {int(tl * factor)}


def test_only_tiles_with_a_later_reader_keep_their_blended_copy(monkeypatch):
    vae, _, seen = standin_vae(monkeypatch)
    vae.enable_tiling()
    vae.encode_image(image01(1, 18, 18), nchw=True, normalize=True)
    assert [(s["y0"], s["x0"], s["up"] is not None, s["left"] is not None, s["want_fin"]) for s in seen] == \
        [(0, 0, False, False, True), (0, 6, False, True, True), (6, 0, True, False, True), (6, 6, True, True, False)]


def test_single_line_edge_tile_blends_with_rows_that_do_not_line_up(monkeypatch):
    """26 px down: tiles of 8, 7 and 1 latent lines.  The last tile's only line blends with line -2 of the 7-line tile above it (its
    line 5), although line 6 is the one that overlaps it geometrically -- the reference's a[-E + y]."""
    vae, enc, _ = standin_vae(monkeypatch, quant=False)
    vae.enable_tiling()
    src = image01(1, 26, 16, seed=3)
    got = vae.encode_image(src, nchw=True, normalize=True).parameters
    mid = enc.moments(src[:, :, 12:26], True, True).clone()
    VE.blend_v(enc.moments(src[:, :, 0:16], True, True), mid, 2)
    last = enc.moments(src[:, :, 24:26], True, True)
    wt = VE.weights(2)
    assert tuple(mid.shape[2:]) == (7, 8) and tuple(last.shape[2:]) == (1, 8) and tuple(got.shape[2:]) == (13, 8)
    assert same_bits(got[:, :, 12, :6], VE.blend(mid[:, :, 5, :6], last[:, :, 0, :6], wt[0, 0], wt[0, 1]))


@pytest.mark.parametrize("H,W", [(16, 16), (8, 16), (16, 10)])
def test_an_image_no_larger_than_a_tile_is_not_tiled(monkeypatch, H, W):
    vae, enc, seen = standin_vae(monkeypatch)
    vae.enable_tiling()
    src = image01(2, H, W)
    dist = vae.encode_image(src, nchw=True, normalize=True)
    assert enc.calls == [(2, 3, H, W)] and seen == []                             # today's path: one call, the posterior kernel's strides
    assert dist._strides == (8 * (H // 2) * (W // 2), (H // 2) * (W // 2), 1) and dist._wq is enc.quant_w and dist._params is None
    # sliced, untiled: sample by sample through the "quant_conv and place" launch
    vae.enable_slicing()
    enc.calls.clear()
    got = vae.encode_image(src, nchw=True, normalize=True).parameters
    assert enc.calls == [(1, 3, H, W)] * 2 and [(s["extent"], s["up"], s["left"], s["want_fin"]) for s in seen] == [(0, None, None, False)] * 2
    assert same_bits(got, transcribed(vae, enc, src, True, True, True, True)) and same_bits(got, enc.moments(src, True, True))
    # a single sample is not sliced
    enc.calls.clear(), seen.clear()
    vae.encode_image(src[:1], nchw=True, normalize=True)
    assert enc.calls == [(1, 3, H, W)] and seen == []


def test_encode_goes_through_the_same_rule(monkeypatch):
    vae, enc, seen = standin_vae(monkeypatch)
    vae.enable_tiling()
    x = 2.0 * image01(1, 26, 40, seed=8) - 1.0
    out = vae.encode(x)
    assert same_bits(out.latent_dist.parameters, transcribed(vae, enc, x, True, False, True, False)) and len(seen) == 12
    assert vae.encode(x, return_dict=False)[0].latent_shape == (1, 4, 13, 20)


def test_refusals_name_the_numbers():
    vae = AutoencoderKL(**SMALL_VAE)
    vae.tile_overlap_factor = 0.95                            # int(16 * 0.05) = 0
    with pytest.raises(ValueError, match=r"tile_sample_min_size = 16 with tile_overlap_factor = 0.95 gives overlap_size = 0 < 1"):
        vae._encode_tile_plan(40, 40)
    vae.tile_overlap_factor = 0.25
    vae.tile_latent_min_size = 0
    with pytest.raises(ValueError, match=r"tile_latent_min_size = 0 .* blend_extent = 0 and row_limit = 0"):
        vae._encode_tile_plan(40, 40)
    vae.tile_latent_min_size = 8
    vae.tile_overlap_factor = 0.3                             # int(16 * 0.7) = 11: an odd tile start under a 1 / 2 encoder
    with pytest.raises(ValueError, match=r"overlap_size = 11: both must be multiples of 2"):
        vae._encode_tile_plan(40, 40)
    vae.tile_overlap_factor = 0.25
    vae.tile_sample_min_size = 14                             # overlap_size int(10.5) = 10 and S = 14: both even, legal
    assert vae._encode_tile_plan(40, 40)[0] == 2
    vae.tile_sample_min_size, vae.tile_overlap_factor = 15, 0.2   # overlap_size 12, S = 15 odd
    with pytest.raises(ValueError, match=r"tile_sample_min_size = 15 .* multiples of 2"):
        vae._encode_tile_plan(40, 40)
    vae.tile_sample_min_size, vae.tile_overlap_factor = 16, 0.25
    vae.tile_latent_min_size = 64                             # blend extent 16 > the 8 latent lines of a full tile
    with pytest.raises(ValueError, match=r"tile_latent_min_size = 64 .* blend_extent = 16, more than the 8 latent rows"):
        vae._encode_tile_plan(40, 40)
    vae.tile_latent_min_size = 8
    assert vae._encode_tile_plan(40, 40)[0] == 2


def test_attribute_defaults_and_surface():
    sdxl = AutoencoderKL(**dinit.SDXL_VAE)
    assert (sdxl.tile_sample_min_size, sdxl.tile_latent_min_size, sdxl.tile_overlap_factor) == (1024, 128, 0.25)
    E, rows, Hl, Wl = sdxl._encode_tile_plan(2048, 2048)
    assert (E, len(rows), len(rows[0]), Hl, Wl) == (32, 3, 3, 256, 256)
    assert list(inspect.signature(AutoencoderKL.encode_image).parameters) == ["self", "img", "nchw", "normalize"]
    assert list(inspect.signature(AutoencoderKL.encode).parameters) == ["self", "x", "return_dict"]
    for other in (AutoencoderTiny, AutoencoderKLWan):
        assert not hasattr(other, "_encode_tile_plan")


@pytest.mark.parametrize("vae_cls,cfg", [(AutoencoderTiny, dinit.TINY_TAESD), (AutoencoderKLWan, dinit.TINY_WAN_VAE)])
def test_the_other_vaes_keep_their_refusal(vae_cls, cfg):
    pipe = object.__new__(P.WanPipeline if vae_cls is AutoencoderKLWan else P.StableDiffusionXLPipeline)
    pipe.vae = vae_cls(**cfg)
    with pytest.raises(NotImplementedError, match=vae_cls.__name__):
        pipe.enable_vae_tiling()


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_facts():
    name = "da_vae_moments_tile_blend"
    assert re.search(r"^int da_vae_moments_tile_blend\(const void\* src, long long sB, long long sC, long long sP, const void\* wq, "
                     r"const void\* bq,\s+const void\* up, int hu, const void\* left, int wl, const void\* weights, int E, void\* fin, "
                     r"void\* moments,\s+int B, int L, int h, int w, int keep_h, int keep_w, long long moments_h, long long moments_w,\s+"
                     r"long long y0, long long x0, void\* stream\);", HEADER, re.M)
    _i, _ll, _vp = L._i, L._ll, L._vp
    assert L.SIGNATURES[name] == (_i, [_vp, _ll, _ll, _ll, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _ll,
                                       _ll, _ll, _ll, _vp])
    assert name in L.PASS_THROUGH and name not in L.FN_IDS and name not in L.NOT_PLANNABLE
    assert "ops.vae_moments_tile_blend refuses under a recording" in " ".join(L.PASS_THROUGH[name].split())
    assert re.search(r"^#define DA_ABI_VERSION 9\b", HEADER, re.M) and L.ABI_VERSION == 9 and L.FN_COUNT == 36


def test_wrapper_refuses_under_a_recording(monkeypatch):
    monkeypatch.setattr(L._tls, "recorder", object(), raising=False)
    with pytest.raises(RuntimeError, match="not replayable by a launch plan"):
        ops.vae_moments_tile_blend(torch.zeros(32, dtype=bf16), (32, 4, 1), batch=1, latent_channels=4, height=2, width=2,
                                   moments=torch.zeros(1, 8, 2, 2, dtype=bf16), y0=0, x0=0, keep_h=2, keep_w=2)


def test_torch_library_op_is_registered_functional_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import diffusers_amd.torch_ops as T
    assert "vae_moments_tile_blend" in T.OPS and not torch.ops.mi355x.vae_moments_tile_blend.default._schema.is_mutable
    with FakeTensorMode():
        e = lambda *s: torch.empty(s, dtype=bf16, device="cuda")                  # noqa: E731
        fin, mom = torch.ops.mi355x.vae_moments_tile_blend(e(2 * 8 * 63), 8 * 63, 63, 1, e(8, 8), e(8), e(2, 8, 5, 9), None, e(2, 8, 20, 30), 4, 7, 9,
                                                           2, 3, 4, 6, 6)
        assert fin.shape == (2, 8, 7, 9) and mom.shape == (2, 8, 20, 30) and fin.dtype == mom.dtype == bf16


# ---- pipelines ----------------------------------------------------------------------------------------------------------
def _sd_embeds(kind):
    g = torch.Generator().manual_seed(3)
    pe, npe = (torch.randn(1, 7, 64, generator=g).to(bf16) for _ in range(2))
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=npe)
    if kind == "sdxl":
        te, nte = (torch.randn(1, 64, generator=g).to(bf16) for _ in range(2))
        kw.update(pooled_prompt_embeds=te, negative_pooled_prompt_embeds=nte)
    return kw


def _flux_embeds():
    g = torch.Generator().manual_seed(3)
    return dict(prompt_embeds=torch.randn(1, 16, 64, generator=g).to(bf16), pooled_prompt_embeds=torch.randn(1, 64, generator=g).to(bf16),
                max_sequence_length=16)


def _build(name):
    family, task = name.split("_")
    if family == "flux":
        return factory.build_flux_pipeline(device="cpu", tiny=True, seed=5, img2img=task == "img2img", inpaint=task == "inpaint")
    build = factory.build_sdxl_pipeline if family == "sdxl" else factory.build_sd15_pipeline
    kw = dict(img2img=True) if task == "img2img" else dict(inpaint=True, unet_in_channels=9) if task == "inpaint" else dict(pix2pix=True)
    return build(device="cpu", tiny=True, seed=0, **kw)


EIGHT = ["sd15_img2img", "sdxl_img2img", "sd15_inpaint", "sdxl_inpaint", "sd15_pix2pix", "sdxl_pix2pix", "flux_img2img", "flux_inpaint"]


@pytest.mark.parametrize("name", EIGHT)
def test_the_eight_pipelines_reach_the_tiled_path(monkeypatch, name):
    """The image of each pipeline goes through AutoencoderKL's tiling rule: one launch of the tile op per tile and encode, the start
    of the loop is another one than untiled, and a tile setting that assembles another grid is refused with both sizes."""
    FE.install(monkeypatch, ops)
    PE.install(monkeypatch, ops)
    FE.install(monkeypatch, ops)                                                  # (its conv_thin_out_moments: the 16-channel one)
    monkeypatch.setattr(ops, "TUNING", False)
    launches = []

    def op(src, strides, **kw):
        launches.append((kw["y0"], kw["x0"]))
        return TE.vae_moments_tile_blend(src, strides, **kw)

    monkeypatch.setattr(ops, "vae_moments_tile_blend", op)
    family, task = name.split("_")
    pipe = _build(name)
    pipe.vae.tile_sample_min_size, pipe.vae.tile_latent_min_size = 16, 8
    starts = []
    monkeypatch.setattr(type(pipe), "_denoise", lambda self, x, step_args, n, ug, begin=0: starts.append(x.clone()) or x)
    H, W = (32, 64) if family == "flux" else (32, 48)
    img = image01(1, H, W, seed=4)
    kw = dict(image=img, num_inference_steps=4, output_type="latent", use_graph=False, generator=None)
    kw.update(_flux_embeds() if family == "flux" else _sd_embeds(family))
    if task != "pix2pix":
        kw["strength"] = 0.6
    if task == "inpaint":
        m = torch.zeros(H, W)
        m[H // 4:3 * H // 4, W // 4:W // 2] = 1.0
        kw["mask_image"] = m

    def run():
        kw["generator"] = torch.Generator().manual_seed(21)
        pipe(**kw)
        return starts.pop()

    untiled = run()
    assert launches == []
    pipe.enable_vae_tiling()
    tiled = run()
    tiles = sum(len(r) for r in pipe.vae._encode_tile_plan(H, W)[1])
    encodes = 2 if name in ("sd15_inpaint", "sdxl_inpaint") else 1               # image and masked image (9-channel U-Net)
    assert len(launches) == tiles * encodes and tiles > 1
    assert tiled.shape == untiled.shape
    if task != "pix2pix":                                                         # (pix2pix starts from noise: the image conditions the step)
        assert not torch.equal(tiled, untiled)
    pipe.vae.tile_latent_min_size = 4                                             # crops of 3 latent lines out of tiles of 8
    with pytest.raises(ValueError, match=rf"assembles \d+ x \d+ latents, the pipeline needs {H // 2} x {W // 2}"):
        run()
    pipe.vae.tile_latent_min_size = 8
    pipe.disable_vae_tiling()
    launches.clear()
    assert torch.equal(run(), untiled) and launches == []
