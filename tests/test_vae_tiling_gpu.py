"""Tiled / sliced AutoencoderKL.decode on the GPU: da_vae_tile_blend against its torch restatement (tests/vae_tiling_emulation.py) to
the bit -- shapes, neighbours, layouts, modes, the bf16 value domain, its memory footprint and its refusals -- then the engine's tiled
decode against a transcription of the reference's tiled_decode over the engine's own untiled decodes of each tile slice, the untiled
identities, and the SDXL / FLUX pipelines with enable_vae_tiling().  The restatement runs on the CPU and stores a NaN result as
0x7FC0, which is the kernel's contract (torch's own bf16 ops give 0x7FC0 or 0xFFFF there, depending on the conversion path)."""
from __future__ import annotations

import itertools

import pytest
import torch

import footprint as FP
import value_domain as VD
import vae_tiling_emulation as VE
from diffusers_amd import _lib as L
from diffusers_amd import init as dinit
from diffusers_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf16 = torch.bfloat16
MODE_CODE = {None: -1, "pt": 0, "np": 1, "uint8": 2}
IMG_DTYPE = {None: bf16, "pt": torch.float32, "np": torch.float32, "uint8": torch.uint8}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(_INT[a.element_size()]), b.view(_INT[b.element_size()])))


def explain(got: torch.Tensor, want: torch.Tensor, **operands) -> str:
    """The first mismatching elements as bit patterns, with the same elements of any operand of the same shape."""
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    it = _INT[got.element_size()]
    g, w = got.view(it).reshape(-1).long(), want.view(it).reshape(-1).long()
    idx = torch.nonzero(g != w).flatten()
    mask = (1 << 8 * got.element_size()) - 1
    lines = [f"{idx.numel()} of {g.numel()} elements differ"]
    for i in idx[:8].tolist():
        ops_ = " ".join(f"{k}={int(v.cpu().contiguous().view(_INT[v.element_size()]).reshape(-1)[i]) & 0xffff:#06x}"
                        for k, v in operands.items() if v is not None and v.numel() == g.numel())
        lines.append(f"[{i}] got {int(g[i]) & mask:#x} want {int(w[i]) & mask:#x} {ops_}")
    return "; ".join(lines)


def _rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(bf16)


def _offset(t: torch.Tensor, off: int) -> torch.Tensor:
    """A device copy of ``t`` (contiguous) whose first element sits ``off`` elements past an allocation's start."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def _source(tile: torch.Tensor, layout: str, seed: int):
    """The tile [B][C][h][w] as the conv would have left it: ("nchw") planes, or ("nhwc16") pixels of 16 channels whose channels >= C
    hold other values.  Returns the flat CPU buffer (element 0 = the tile's first element) and the strides."""
    B, C, h, w = tile.shape
    if layout == "nchw":
        return tile.reshape(-1).clone(), (C * h * w, h * w, 1)
    pad = _rnd((B, h * w, 16), seed + 77, 50.0)
    pad[:, :, :C] = tile.permute(0, 2, 3, 1).reshape(B, h * w, C)
    return pad.reshape(-1), (h * w * 16, 1, 16)


def _image_poison(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return (torch.randn(shape, generator=g) * 7).to(dtype)


def run_case(lib, *, B, C, h, w, E, hu, wl, layout, mode, keep, off, fin_null, seed, tile=None, up=None, left=None):
    """One launch against the stand-in; hu / wl None: no such neighbour.  Everything is compared to the bit: the blended tile, the
    WHOLE image (so what lies outside the placed rectangle keeps its poison) and the inputs."""
    tile = _rnd((B, C, h, w), seed, 2.0) if tile is None else tile
    up = (_rnd((B, C, hu, w), seed + 1, 2.0) if up is None else up) if hu is not None else None
    left = (_rnd((B, C, h, wl), seed + 2, 2.0) if left is None else left) if wl is not None else None
    keep_h, keep_w = keep
    y0, x0 = seed % 3, (seed // 3) % 4
    IH, IW = y0 + keep_h + seed % 2, x0 + keep_w + (seed // 2) % 3
    ishape = (B, IH, IW, C) if mode in ("np", "uint8") else (B, C, IH, IW)
    img0 = _image_poison(ishape, IMG_DTYPE[mode], seed + 3)
    flat, strides = _source(tile, layout, seed)
    # the stand-in, on the CPU
    want_img = img0.clone()
    want_fin = VE.vae_tile_blend(flat, strides, batch=B, channels=C, height=h, width=w, image=want_img, y0=y0, x0=x0, keep_h=keep_h,
                                 keep_w=keep_w, postprocess=mode, extent=E, up=up, left=left)
    # the kernel
    d_src, d_img = _offset(flat, off), _offset(img0, off)
    d_up = _offset(up, off) if up is not None else None
    d_left = _offset(left, off) if left is not None else None
    d_fin = None if fin_null else _offset(torch.full((B, C, h, w), 9.0, dtype=bf16), off)
    wt = ops.tile_blend_weights(E, DEV) if E > 0 and (up is not None or left is not None) else None
    rc = lib.da_vae_tile_blend(d_src.data_ptr(), *strides, ops._ptr(d_up), hu or 0, ops._ptr(d_left), wl or 0, ops._ptr(wt), E,
                               ops._ptr(d_fin), d_img.data_ptr(), B, C, h, w, keep_h, keep_w, IH, IW, y0, x0, MODE_CODE[mode],
                               torch.cuda.current_stream().cuda_stream)
    what = dict(B=B, C=C, h=h, w=w, E=E, hu=hu, wl=wl, layout=layout, mode=mode, keep=keep, off=off, fin_null=fin_null, seed=seed)
    assert rc == L.DA_OK, what
    torch.cuda.synchronize()
    if not fin_null:
        assert same_bits(d_fin, want_fin), (what, explain(d_fin, want_fin, tile=tile, up=up, left=left))
    assert same_bits(d_img, want_img), (what, explain(d_img, want_img))
    assert same_bits(d_src, flat) and (up is None or same_bits(d_up, up)) and (left is None or same_bits(d_left, left)), what


SIZES = [(1, 1), (1, 67), (2, 7), (7, 2), (16, 16), (33, 67), (67, 33), (67, 67), (7, 16), (16, 1)]      # h, w from {1, 2, 7, 16, 33, 67}


def sweep_cases(start: int = 0):
    """(h, w) x E x neighbours, the other dimensions cycling with the case number; ``start`` shifts the cycles, so that the eight
    (layout, mode) runs do not repeat one another."""
    n = start
    for (h, w), E, neigh in itertools.product(SIZES, (0, 1, 3, 8), ("none", "up", "left", "both")):
        n += 1
        k = (n + n // 4 + n // 16) % 4                                              # (n % 4 alone is tied to `neigh`)
        hu = (E, E + 2, max(h, E), 67)[k] if neigh in ("up", "both") else None  # hu != h in most, hu >= E always
        wl = (67, max(w, E), E + 1, E)[k] if neigh in ("left", "both") else None
        hu, wl = (5 if hu == 0 else hu), (4 if wl == 0 else wl)
        keep = (h, w) if n % 3 == 0 else (max(1, h - h // 4 - n % 2), max(1, w - w // 3))
        yield dict(h=h, w=w, E=E, hu=hu, wl=wl, C=(1, 3, 4)[n % 3], B=(1, 2)[(n // 3) % 2], keep=keep, off=(n // 2) % 2,
                   fin_null=n % 5 == 0, seed=n)


SWEEPS = [(layout, mode) for layout in ("nchw", "nhwc16") for mode in VE.MODES]


@pytest.mark.parametrize("start", range(len(SWEEPS)))
def test_the_sweep_reaches_what_it_claims(start):
    cases = list(sweep_cases(start))
    assert len(cases) == 160
    assert any(c["hu"] is not None and c["E"] > c["h"] for c in cases) and any(c["wl"] is not None and c["E"] > c["w"] for c in cases)
    assert any(c["hu"] not in (None, c["h"]) for c in cases) and any(c["wl"] not in (None, c["w"]) for c in cases)
    assert any(c["hu"] == c["E"] > 0 for c in cases) and any(c["wl"] == c["E"] > 0 for c in cases)
    for key, vals in (("C", {1, 3, 4}), ("B", {1, 2}), ("off", {0, 1}), ("fin_null", {False, True})):
        assert {c[key] for c in cases} == vals
    assert any(c["keep"] != (c["h"], c["w"]) for c in cases) and any(c["keep"] == (c["h"], c["w"]) for c in cases)
    assert all(c["hu"] is None or c["hu"] >= max(c["E"], 1) for c in cases) and all(c["wl"] is None or c["wl"] >= max(c["E"], 1) for c in cases)


@pytest.mark.parametrize("layout,mode", SWEEPS)
def test_kernel_equals_the_emulation_to_the_bit(layout, mode):
    lib = L.load()
    for c in sweep_cases(SWEEPS.index((layout, mode))):
        run_case(lib, layout=layout, mode=mode, **c)


@pytest.mark.parametrize("E", [3, 4])
def test_value_domain(E):
    """Every finite bf16 value and +-inf as the neighbour's value and as the tile's own, under every weight pair of E = 3 (weights that
    are no binary fractions) and E = 4 (row 0 multiplies the tile's value by zero: inf * 0).  One tile of E x 65 282 pixels -- wider
    than the other tests' tiles, so that each row holds the whole domain."""
    lib = L.load()
    dom = torch.cat([VD.all_finite_bf16(), torch.tensor([float("inf"), float("-inf")]).to(bf16)])
    n = dom.numel()
    perm = (torch.arange(n) * 7919 + 13) % n                                    # 7919 is prime and does not divide n: a permutation
    assert perm.unique().numel() == n
    rows = lambda first: torch.stack([torch.roll(first, 1013 * y) for y in range(E)]).view(1, 1, E, n)
    for a, b in ((rows(dom), rows(dom[perm])), (rows(dom[perm]), rows(dom)), (rows(dom), rows(-dom))):
        for mode in (None, "pt", "uint8"):
            run_case(lib, B=1, C=1, h=E, w=n, E=E, hu=E, wl=None, layout="nchw", mode=mode, keep=(E, n), off=0, fin_null=False, seed=0,
                     tile=b, up=a)
    # the horizontal blend: the same pairs down a column of a tile that is E pixels wide
    a, b = rows(dom).transpose(2, 3).contiguous(), rows(dom[perm]).transpose(2, 3).contiguous()
    run_case(lib, B=1, C=1, h=n, w=E, E=E, hu=None, wl=E, layout="nhwc16", mode=None, keep=(n, E), off=0, fin_null=False, seed=0,
             tile=b, left=a)


@pytest.mark.parametrize("mode", VE.MODES)
@pytest.mark.parametrize("layout", ["nchw", "nhwc16"])
def test_footprint(layout, mode):
    """Guard bands round `fin` and the image stay intact, the image outside the placed rectangle keeps its poison, and poisoned
    surroundings of the inputs (NaNs before, after and between the rows of the source, the neighbours and the weights) do not reach the
    output: it equals, to the bit, the run whose surroundings are zeros, and is finite."""
    lib = L.load()
    B, C, h, w, E, hu, wl = 2, 3, 33, 19, 8, 11, 9
    keep_h, keep_w, y0, x0, IH, IW = 25, 14, 3, 5, 40, 31
    tile, up, left = _rnd((B, C, h, w), 1), _rnd((B, C, hu, w), 2), _rnd((B, C, h, wl), 3)
    if layout == "nchw":
        src = FP.poisoned(tile.reshape(B, C, h * w), ld=h * w + 5, batch_stride=C * (h * w + 5) + 3)
        strides = (src.batch_stride, src.ld, 1)
    else:
        px = torch.full((B, h * w, 16), float("nan")).to(bf16)                   # channels >= C of a pixel: poison as well
        px[:, :, :C] = tile.permute(0, 2, 3, 1).reshape(B, h * w, C)
        src = FP.poisoned(px, batch_stride=h * w * 16 + 16)
        strides = (src.batch_stride, 1, 16)
    g_up, g_left = FP.poisoned(up.reshape(B * C * hu, w)), FP.poisoned(left.reshape(B * C * h, wl))
    g_wt = FP.poisoned(VE.weights(E))
    ishape = (B, IH, IW * C) if mode in ("np", "uint8") else (B * C * IH, IW)
    outs = []
    for clean in (False, True):
        s, u, l, wt = (g.clean() if clean else g for g in (src, g_up, g_left, g_wt))
        fin = FP.guarded((B * C * h, w))
        img = FP.guarded(ishape, dtype=IMG_DTYPE[mode])
        rc = lib.da_vae_tile_blend(s.ptr(), *strides, u.ptr(), hu, l.ptr(), wl, wt.ptr(), E, fin.ptr(), img.ptr(), B, C, h, w, keep_h,
                                   keep_w, IH, IW, y0, x0, MODE_CODE[mode], torch.cuda.current_stream().cuda_stream)
        assert rc == L.DA_OK
        torch.cuda.synchronize()
        fin.check("fin"), img.check("image")
        placed = torch.zeros((B, IH, IW, C) if mode in ("np", "uint8") else (B, C, IH, IW), dtype=torch.bool, device=DEV)
        if mode in ("np", "uint8"):
            placed[:, y0:y0 + keep_h, x0:x0 + keep_w, :] = True
        else:
            placed[:, :, y0:y0 + keep_h, x0:x0 + keep_w] = True
        view_bits = img.view.contiguous().view(_INT[img.itemsize]).reshape(placed.shape)
        assert bool((view_bits[~placed] == 0).all()), "the image outside the placed rectangle was written"
        assert bool(torch.isfinite(fin.view.float()).all()) and bool(torch.isfinite(img.view.float()[placed.reshape(img.view.shape)]).all())
        outs.append((fin.view.clone(), img.view.clone()))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    want_img = torch.zeros((B, IH, IW, C) if mode in ("np", "uint8") else (B, C, IH, IW), dtype=IMG_DTYPE[mode])
    flat, st = _source(tile, layout, 0)
    want_fin = VE.vae_tile_blend(flat, st, batch=B, channels=C, height=h, width=w, image=want_img, y0=y0, x0=x0, keep_h=keep_h,
                                 keep_w=keep_w, postprocess=mode, extent=E, up=up, left=left)
    assert same_bits(outs[0][0].reshape(B, C, h, w), want_fin) and same_bits(outs[0][1].reshape(want_img.shape), want_img)


def test_refusals_launch_nothing():
    lib = L.load()
    B, C, h, w, E, hu, wl = 1, 3, 8, 8, 4, 6, 5
    src, up, left = (_rnd(s, i).to(DEV) for i, s in enumerate(((B, C, h, w), (B, C, hu, w), (B, C, h, wl))))
    wt = ops.tile_blend_weights(E, DEV)
    fin = torch.full((B, C, h, w), 5.0, dtype=bf16, device=DEV)
    img = torch.full((B, C, 10, 12), 7.0, dtype=bf16, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    good = dict(src=src.data_ptr(), sB=C * h * w, sC=h * w, sP=1, up=up.data_ptr(), hu=hu, left=left.data_ptr(), wl=wl, wt=wt.data_ptr(),
                E=E, fin=fin.data_ptr(), img=img.data_ptr(), B=B, C=C, h=h, w=w, keep_h=6, keep_w=7, IH=10, IW=12, y0=2, x0=3, mode=-1)
    bad = [dict(src=None), dict(img=None), dict(wt=None), dict(C=0), dict(C=5), dict(E=-1), dict(hu=3), dict(wl=3), dict(keep_h=9),
           dict(keep_w=9), dict(keep_h=0), dict(y0=5), dict(x0=6), dict(y0=-1), dict(x0=-1), dict(mode=-2), dict(mode=3), dict(B=0),
           dict(h=0), dict(w=0), dict(sB=-1), dict(sC=-1), dict(sP=-1), dict(IH=7), dict(IW=9), dict(B=65536), dict(h=1 << 16, w=1 << 15)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.da_vae_tile_blend(a["src"], a["sB"], a["sC"], a["sP"], a["up"], a["hu"], a["left"], a["wl"], a["wt"], a["E"], a["fin"],
                                   a["img"], a["B"], a["C"], a["h"], a["w"], a["keep_h"], a["keep_w"], a["IH"], a["IW"], a["y0"], a["x0"],
                                   a["mode"], st)
        assert rc == 1, change                                                   # DA_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((fin == 5.0).all()) and bool((img == 7.0).all())
    a = good                                                                     # ... and the unchanged arguments are accepted
    assert lib.da_vae_tile_blend(a["src"], a["sB"], a["sC"], a["sP"], a["up"], a["hu"], a["left"], a["wl"], a["wt"], a["E"], a["fin"],
                                 a["img"], a["B"], a["C"], a["h"], a["w"], a["keep_h"], a["keep_w"], a["IH"], a["IW"], a["y0"], a["x0"],
                                 a["mode"], st) == L.DA_OK
    torch.cuda.synchronize()
    assert not bool((fin == 5.0).all()) and bool((img[:, :, :2] == 7.0).all()) and not bool((img[:, :, 2:8, 3:10] == 7.0).any())
    with pytest.raises(ValueError, match="up must be contiguous"):
        ops.vae_tile_blend(src, (C * h * w, h * w, 1), batch=B, channels=C, height=h, width=w, image=img, y0=0, x0=0, keep_h=6, keep_w=7,
                           extent=8, up=up)
    # a channels-last source is read four channels at a time: slots of 4 holding 3 channels, trimmed after the last one, are refused
    trimmed = torch.zeros(h * w * 4 - 1, dtype=bf16, device=DEV)
    with pytest.raises(ValueError, match="strides"):
        ops.vae_tile_blend(trimmed, (h * w * 4, 1, 4), batch=B, channels=C, height=h, width=w, image=img, y0=0, x0=0, keep_h=6, keep_w=7)
    ops.vae_tile_blend(torch.zeros(h * w * 4, dtype=bf16, device=DEV), (h * w * 4, 1, 4), batch=B, channels=C, height=h, width=w,
                       image=img, y0=0, x0=0, keep_h=6, keep_w=7)
    with pytest.raises(ValueError, match="strides"):
        ops.vae_tile_blend(src, (C * h * w, h * w, 2), batch=B, channels=C, height=h, width=w, image=img, y0=0, x0=0, keep_h=6, keep_w=7)


# ---- the engine's tiled decode ---------------------------------------------------------------------------------------------------
def _engine_reference(vae, z, div=1.0, add=0.0):
    """The reference's tiled_decode, transcribed, over the engine's own UNTILED decode of each tile slice; blends on the CPU."""
    def decode_tile(zt):
        return vae._decode(zt.contiguous(), div, add, None).cpu()
    return VE.reference_tiled_decode(z, decode_tile, tile_latent_min_size=vae.tile_latent_min_size,
                                     tile_sample_min_size=vae.tile_sample_min_size, tile_overlap_factor=vae.tile_overlap_factor)


ENGINE_CASES = {
    # TINY_VAE: tile 16 latent / 32 px, E = 8; 40 x 28 latents: a 4 x 3 grid with short last tiles both ways (per-pixel conv_out route)
    "tiny_4x3": (dinit.TINY_VAE, {}, (2, 4, 40, 28), {}),
    # tiles of 32 latent / 64 px, B = 2: 8192 pixels a tile, the implicit-GEMM route of the tile's conv_out
    "tiny_tile64": (dinit.TINY_VAE, dict(tile_sample_min_size=64, tile_latent_min_size=32), (2, 4, 72, 40), {}),
    "tiny_flux": (dinit.TINY_FLUX_VAE, {}, (1, 16, 24, 40), dict(latents_div=0.3611, latents_add=0.1159)),
}


@pytest.fixture(scope="module", params=list(ENGINE_CASES))
def engine_case(request):
    from diffusers_amd import factory
    cfg, attrs, zshape, kw = ENGINE_CASES[request.param]
    vae, _ = factory.build_vae(cfg, seed=1, device=DEV)
    for k, v in attrs.items():
        setattr(vae, k, v)
    z = _rnd(zshape, 17, 1.5).to(DEV)
    want = _engine_reference(vae, z, kw.get("latents_div", 1.0), kw.get("latents_add", 0.0))
    torch.cuda.synchronize()
    return request.param, vae, z, kw, want


@pytest.mark.parametrize("mode", VE.MODES)
def test_tiled_decode_equals_the_transcribed_reference(engine_case, mode, monkeypatch):
    name, vae, z, kw, want = engine_case
    routes, real = set(), ops.conv_thin_out_tile

    def spy(x, w, b):
        y, strides = real(x, w, b)
        routes.add(tuple(strides[1:]))                                           # (sC, sP)
        return y, strides

    monkeypatch.setattr(ops, "conv_thin_out_tile", spy)
    vae.enable_tiling()
    try:
        got = vae.decode(z, postprocess=mode, **kw).sample
    finally:
        vae.disable_tiling()
    up = 2 ** (len(vae.config.block_out_channels) - 1)
    assert tuple(want.shape) == (z.shape[0], 3, z.shape[2] * up, z.shape[3] * up) and bool(torch.isfinite(want.float()).all())
    assert same_bits(got, VE.postprocess_image(want, mode)), (name, mode)
    # which conv_out route the tiles took, as the strides handed to the blend kernel show: the 64 px tiles the implicit-GEMM one
    # (16-padded NHWC), their smaller edge tiles and the 32 px tiles the per-pixel one (NCHW)
    nhwc16, nchw = (1, ops.THIN_OUT_PAD) in routes, any(sP == 1 for _, sP in routes)
    assert (nhwc16, nchw) == ((True, True) if name == "tiny_tile64" else (False, True)), (name, routes)


def test_tiled_differs_from_untiled_and_the_seams_are_blended(engine_case):
    """Not a tolerance: the tiled result is another image than the untiled one (tile-wise GroupNorm), which is what the reference gives."""
    name, vae, z, kw, want = engine_case
    whole = vae.decode(z, **kw).sample
    assert whole.shape == want.shape and not same_bits(whole, want)


# ---- untiled identities ----------------------------------------------------------------------------------------------------------
def parent_decode(vae, z, latents_div, latents_add, postprocess):
    """AutoencoderKL.decode as it was before tiling existed, restated from the layers."""
    z = z.contiguous()
    if vae.post_quant_conv:
        x = ops.conv_thin_in(z, vae.pqc_w, vae.pqc_b, ksize=1, in_nchw=True, in_div=latents_div, in_add=latents_add)
        x = ops.conv_thin_in(x, vae.conv_in_w, vae.conv_in_b, ksize=3, in_nchw=False)
    else:
        x = ops.conv_thin_in(z, vae.conv_in_w, vae.conv_in_b, ksize=3, in_nchw=True, in_div=latents_div, in_add=latents_add)
    x = vae.mid_res0(x)
    if vae.mid_attn is not None:
        x = vae.mid_attn(x)
    x = vae.mid_res1(x)
    for st in vae.up:
        for rn in st["resnets"]:
            x = rn(x)
        if st["up"] is not None:
            x = st["up"](x)
    x = vae.conv_norm_out(x, silu=True)
    return ops.conv_thin_out(x, vae.conv_out_w, vae.conv_out_b, postprocess=postprocess)


@pytest.mark.parametrize("mode", VE.MODES)
def test_untiled_identities(mode):
    from diffusers_amd import factory
    vae, _ = factory.build_vae(dinit.TINY_VAE, seed=1, device=DEV)
    z = _rnd((3, 4, 16, 12), 5, 1.5).to(DEV)                                    # no larger than the 16-latent tile
    kw = dict(latents_div=0.13025, postprocess=mode)
    off = vae.decode(z, **kw).sample
    assert same_bits(off, parent_decode(vae, z, 0.13025, 0.0, mode))              # tiling off = the parent's decode
    vae.enable_tiling()
    assert same_bits(vae.decode(z, **kw).sample, off)                            # latents no larger than the tile: untiled
    vae.disable_tiling()
    vae.enable_slicing()
    sliced = vae.decode(z, **kw).sample
    vae.disable_slicing()
    singles = torch.cat([vae.decode(z[b:b + 1], **kw).sample for b in range(3)], 0)
    assert same_bits(sliced, singles)
    # sliced AND tiled: sample by sample through the tiling rule, into one output
    zt = _rnd((3, 4, 20, 28), 6, 1.5).to(DEV)
    vae.enable_tiling()
    singles = torch.cat([vae.decode(zt[b:b + 1], **kw).sample for b in range(3)], 0)
    vae.enable_slicing()
    assert same_bits(vae.decode(zt, **kw).sample, singles)


# ---- pipelines -------------------------------------------------------------------------------------------------------------------
def _sdxl_embeds(seed=3):
    g = torch.Generator().manual_seed(seed)
    pe, npe = (torch.randn(1, 7, 64, generator=g).to(bf16).to(DEV) for _ in range(2))
    te, nte = (torch.randn(1, 64, generator=g).to(bf16).to(DEV) for _ in range(2))
    return dict(prompt_embeds=pe, negative_prompt_embeds=npe, pooled_prompt_embeds=te, negative_pooled_prompt_embeds=nte)


def _flux_embeds(seed=3):
    g = torch.Generator().manual_seed(seed)
    return dict(prompt_embeds=torch.randn(1, 16, 64, generator=g).to(bf16).to(DEV),
                pooled_prompt_embeds=torch.randn(1, 64, generator=g).to(bf16).to(DEV))


@pytest.mark.parametrize("family", ["sdxl", "flux"])
def test_pipeline_with_vae_tiling(family):
    """48 x 64 pixels = 24 x 32 latents with the tiny VAEs' 16-latent tiles: 2 x 3 tiles."""
    from diffusers_amd import factory
    from diffusers_amd.pipelines import decode_postprocessed
    if family == "sdxl":
        pipe = factory.build_sdxl_pipeline(device=DEV, tiny=True, seed=0)
        kw = dict(num_inference_steps=2, guidance_scale=5.0, **_sdxl_embeds())
    else:
        pipe = factory.build_flux_pipeline(device=DEV, tiny=True, seed=5)
        kw = dict(num_inference_steps=2, max_sequence_length=16, **_flux_embeds())
    assert [len(r) for r in pipe.vae._tile_plan(24, 32)[1]] == [3, 3]

    def run(use_graph, output_type="pt"):
        out = pipe(height=48, width=64, generator=torch.Generator().manual_seed(21), use_graph=use_graph, output_type=output_type, **kw).images
        torch.cuda.synchronize()
        return out.clone()
    untiled = run(True)
    graph = pipe._graph
    pipe.enable_vae_tiling()
    assert pipe.vae.use_tiling is True
    tiled = run(True)
    assert pipe._graph is graph, "enabling VAE tiling recaptured the step"
    assert tuple(tiled.shape) == (1, 3, 48, 64) and bool(torch.isfinite(tiled).all()) and not torch.equal(tiled, untiled)
    assert torch.equal(run(False), tiled), "eager != HIP graph"
    lat = run(True, output_type="latent")
    vc = pipe.vae.config
    if family == "flux":
        lat = pipe._unpack_latents(lat, 48, 64, pipe.vae_scale_factor).contiguous()
        dkw = dict(latents_div=float(vc.scaling_factor), latents_add=float(vc.shift_factor))
    else:
        dkw = dict(latents_div=float(vc.scaling_factor))
    assert tuple(lat.shape[2:]) == (24, 32)
    assert torch.equal(decode_postprocessed(pipe.vae, lat, "pt", **dkw), tiled), "the image is not the tiled vae.decode of the pipeline's latents"
    want = VE.postprocess_image(_engine_reference(pipe.vae, lat, dkw["latents_div"], dkw.get("latents_add", 0.0)), "pt")
    assert same_bits(tiled, want)
    pipe.disable_vae_tiling()
    assert torch.equal(run(True), untiled) and pipe._graph is graph, "disabling VAE tiling recaptured the step or left a trace"
