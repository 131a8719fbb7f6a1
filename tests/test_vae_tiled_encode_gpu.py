"""Tiled / sliced AutoencoderKL.encode on the GPU: da_vae_moments_tile_blend against its torch restatement
(tests/vae_tiled_encode_emulation.py) to the bit -- shapes, neighbours, layouts, channel counts, quant_conv, the bf16 value domain, its
memory footprint and its refusals -- then the engine's tiled encode against a transcription of the reference's _tiled_encode over the
engine's own untiled encodes of each tile, the posterior calls on the tiled distribution, and four image-reading pipelines with
enable_vae_tiling().  The restatement runs on the CPU and stores a NaN blend result as 0x7FC0, which is the kernel's contract."""
from __future__ import annotations

import itertools

import pytest
import torch

import footprint as FP
import value_domain as VD
import vae_tiled_encode_emulation as TE
import vae_tiling_emulation as VE
from diffusers_amd import _lib as L
from diffusers_amd import init as dinit
from diffusers_amd import ops
from diffusers_amd.autoencoder_kl import DiagonalGaussianDistribution

pytestmark = pytest.mark.gpu
DEV = "cuda"
bf16 = torch.bfloat16
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(_INT[a.element_size()]), b.view(_INT[b.element_size()])))


def explain(got: torch.Tensor, want: torch.Tensor) -> str:
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    g, w = got.view(torch.int16).reshape(-1).long() & 0xffff, want.view(torch.int16).reshape(-1).long() & 0xffff
    idx = torch.nonzero(g != w).flatten()
    return "; ".join([f"{idx.numel()} of {g.numel()} elements differ"] + [f"[{i}] got {int(g[i]):#06x} want {int(w[i]):#06x}" for i in idx[:8].tolist()])


def _rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(bf16)


def _offset(t: torch.Tensor, off: int) -> torch.Tensor:
    """A device copy of ``t`` (contiguous) whose first element sits ``off`` elements past an allocation's start."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def _quant(C, seed):
    return _rnd((C, C), seed + 11, 0.5), _rnd((C,), seed + 12, 0.1)


def launch(lib, src, strides, wq, bq, up, hu, left, wl, wt, E, fin, mom, B, Lc, h, w, keep_h, keep_w, HL, WL, y0, x0):
    return lib.da_vae_moments_tile_blend(ops._ptr(src), *strides, ops._ptr(wq), ops._ptr(bq), ops._ptr(up), hu or 0, ops._ptr(left), wl or 0,
                                         ops._ptr(wt), E, ops._ptr(fin), ops._ptr(mom), B, Lc, h, w, keep_h, keep_w, HL, WL, y0, x0,
                                         torch.cuda.current_stream().cuda_stream)


def run_case(lib, *, B, Lc, h, w, E, hu, wl, layout, quant, keep, off, fin_null, seed, tile=None, up=None, left=None, wq=None, bq=None):
    """One launch against the stand-in; hu / wl None: no such neighbour.  Everything is compared to the bit: the blended tile, the
    WHOLE moments tensor (so what lies outside the placed rectangle keeps its poison) and the inputs."""
    C = 2 * Lc
    tile = _rnd((B, C, h, w), seed, 2.0) if tile is None else tile
    up = (_rnd((B, C, hu, w), seed + 1, 2.0) if up is None else up) if hu is not None else None
    left = (_rnd((B, C, h, wl), seed + 2, 2.0) if left is None else left) if wl is not None else None
    if quant and wq is None:
        wq, bq = _quant(C, seed)
    keep_h, keep_w = keep
    y0, x0 = seed % 3, (seed // 3) % 4
    HL, WL = y0 + keep_h + seed % 2, x0 + keep_w + (seed // 2) % 3
    mom0 = _rnd((B, C, HL, WL), seed + 3, 7.0)
    flat, strides = TE.layout_source(tile, layout, pad=_rnd((B, h * w, 16), seed + 77, 50.0) if layout == "nhwc16" else None)
    want_mom = mom0.clone()
    want_fin = TE.vae_moments_tile_blend(flat, strides, batch=B, latent_channels=Lc, height=h, width=w, moments=want_mom, y0=y0, x0=x0,
                                         keep_h=keep_h, keep_w=keep_w, wq=wq, bq=bq, extent=E, up=up, left=left)
    d = lambda t: None if t is None else _offset(t, off)                          # noqa: E731
    d_src, d_mom, d_up, d_left, d_wq, d_bq = d(flat), d(mom0), d(up), d(left), d(wq), d(bq)
    d_fin = None if fin_null else _offset(torch.full((B, C, h, w), 9.0, dtype=bf16), off)
    wt = ops.tile_blend_weights(E, DEV) if E > 0 and (up is not None or left is not None) else None
    rc = launch(lib, d_src, strides, d_wq, d_bq, d_up, hu, d_left, wl, wt, E, d_fin, d_mom, B, Lc, h, w, keep_h, keep_w, HL, WL, y0, x0)
    what = dict(B=B, Lc=Lc, h=h, w=w, E=E, hu=hu, wl=wl, layout=layout, quant=quant, keep=keep, off=off, fin_null=fin_null, seed=seed)
    assert rc == L.DA_OK, what
    torch.cuda.synchronize()
    if not fin_null:
        assert same_bits(d_fin, want_fin), (what, explain(d_fin, want_fin))
    assert same_bits(d_mom, want_mom), (what, explain(d_mom, want_mom))
    assert same_bits(d_src, flat) and (up is None or same_bits(d_up, up)) and (left is None or same_bits(d_left, left)), what


SIZES = [(1, 1), (1, 16), (2, 3), (3, 2), (8, 9), (9, 8), (16, 16), (3, 16), (16, 1), (9, 9), (2, 8), (8, 3)]   # h, w from {1, 2, 3, 8, 9, 16}


def sweep_cases(start: int = 0):
    """(h, w) x E x neighbours, the other dimensions cycling with the case number; ``start`` shifts the cycles, so that the sweeps do
    not repeat one another."""
    n = start
    for (h, w), E, neigh in itertools.product(SIZES, (0, 1, 2, 3, 8), ("none", "up", "left", "both")):
        n += 1
        k = (n + n // 4 + n // 16) % 4                                              # (n % 4 alone is tied to `neigh`)
        hu = (E, E + 2, max(h, E), 19)[k] if neigh in ("up", "both") else None     # hu != h in most, hu >= E always
        wl = (19, max(w, E), E + 1, E)[k] if neigh in ("left", "both") else None
        hu, wl = (5 if hu == 0 else hu), (4 if wl == 0 else wl)
        keep = (h, w) if n % 3 == 0 else (max(1, h - h // 4 - n % 2), max(1, w - w // 3))
        yield dict(h=h, w=w, E=E, hu=hu, wl=wl, B=(1, 2)[(n // 3) % 2], keep=keep, off=(n // 2) % 2, fin_null=n % 5 == 0, seed=n)


# (latent channels, quant_conv, source layout): 2 L = 8 with and without a quant_conv from the three layouts, 2 L = 32 without (16
# padded channels cannot hold 32; NHWC with sP = 2 L is what its conv_out leaves)
SWEEPS = [(4, q, lay) for q in (True, False) for lay in TE.LAYOUTS] + [(16, False, "nchw"), (16, False, "nhwc")]


@pytest.mark.parametrize("start", range(len(SWEEPS)))
def test_the_sweep_reaches_what_it_claims(start):
    cases = list(sweep_cases(start))
    assert len(cases) == 240
    assert {c["h"] for c in cases} == {c["w"] for c in cases} == {1, 2, 3, 8, 9, 16} and {c["E"] for c in cases} == {0, 1, 2, 3, 8}
    assert any(c["hu"] is not None and c["E"] > c["h"] for c in cases) and any(c["wl"] is not None and c["E"] > c["w"] for c in cases)
    assert any(c["hu"] not in (None, c["h"]) for c in cases) and any(c["wl"] not in (None, c["w"]) for c in cases)
    assert any(c["hu"] == c["E"] > 0 for c in cases) and any(c["wl"] == c["E"] > 0 for c in cases)
    for key, vals in (("B", {1, 2}), ("off", {0, 1}), ("fin_null", {False, True})):
        assert {c[key] for c in cases} == vals
    assert any(c["keep"] != (c["h"], c["w"]) for c in cases) and any(c["keep"] == (c["h"], c["w"]) for c in cases)
    assert any(c["seed"] % 3 and (c["seed"] // 3) % 4 for c in cases)                                   # placed at a non-zero (y0, x0)
    assert all(c["hu"] is None or c["hu"] >= max(c["E"], 1) for c in cases) and all(c["wl"] is None or c["wl"] >= max(c["E"], 1) for c in cases)


@pytest.mark.parametrize("Lc,quant,layout", SWEEPS)
def test_kernel_equals_the_emulation_to_the_bit(Lc, quant, layout):
    lib = L.load()
    for c in sweep_cases(SWEEPS.index((Lc, quant, layout))):
        run_case(lib, Lc=Lc, quant=quant, layout=layout, **c)


@pytest.mark.parametrize("E", [3, 4])
def test_value_domain_of_the_blends(E):
    """Every finite bf16 value, +-inf and NaNs as the neighbour's value and as the tile's own, under every weight pair of E = 3
    (weights that are no binary fractions) and E = 4 (row 0 multiplies the tile's value by zero: inf * 0).  A NaN result is 0x7FC0."""
    lib = L.load()
    nans = torch.tensor([0x7FC0, 0xFFFF, 0x7F81], dtype=torch.int32).to(torch.int16).view(bf16)
    dom = torch.cat([VD.all_finite_bf16(), torch.tensor([float("inf"), float("-inf")]).to(bf16), nans])
    n = dom.numel()
    perm = (torch.arange(n) * 7919 + 13) % n                                    # 7919 is prime and does not divide n: a permutation
    assert perm.unique().numel() == n
    rows = lambda first: torch.stack([torch.stack([torch.roll(first, 1013 * y + 97 * c) for y in range(E)]) for c in range(8)]).view(1, 8, E, n)  # noqa: E731
    for a, b in ((rows(dom), rows(dom[perm])), (rows(dom[perm]), rows(dom)), (rows(dom), rows(-dom))):
        run_case(lib, B=1, Lc=4, h=E, w=n, E=E, hu=E, wl=None, layout="nchw", quant=False, keep=(E, n), off=0, fin_null=False, seed=0,
                 tile=b, up=a)
    # the horizontal blend: the same pairs down a column of a tile that is E pixels wide, from the padded channels-last layout
    a, b = rows(dom).transpose(2, 3).contiguous(), rows(dom[perm]).transpose(2, 3).contiguous()
    run_case(lib, B=1, Lc=4, h=n, w=E, E=E, hu=None, wl=E, layout="nhwc16", quant=False, keep=(n, E), off=0, fin_null=False, seed=0,
             tile=b, left=a)


def test_value_domain_of_the_quant_conv():
    """Every finite bf16 value in one input channel (the others small, so that a sum overflows to one infinity at most and never to a
    NaN), through a quant_conv and a blend."""
    lib = L.load()
    dom = VD.all_finite_bf16()
    n = dom.numel()
    for ch in (0, 5):
        tile = _rnd((1, 8, 2, n), 40 + ch, 0.5)
        tile[0, ch, 0], tile[0, ch, 1] = dom, torch.roll(dom, 4099)
        run_case(lib, B=1, Lc=4, h=2, w=n, E=2, hu=3, wl=None, layout=("nchw", "nhwc16")[ch % 2], quant=True, keep=(2, n), off=0,
                 fin_null=False, seed=ch, tile=tile)


@pytest.mark.parametrize("Lc,quant,layout", SWEEPS)
def test_footprint(Lc, quant, layout):
    """Guard bands round `fin` and the moments stay intact, the moments outside the placed rectangle keep their fill, and poisoned
    surroundings of the inputs (NaNs before, after and between the rows of the source, the neighbours, the weights and the
    quant_conv) do not reach the output: it equals, to the bit, the run whose surroundings are zeros, and is finite."""
    lib = L.load()
    C = 2 * Lc
    B, h, w, E, hu, wl = 2, 33, 19, 8, 11, 9
    keep_h, keep_w, y0, x0, HL, WL = 25, 14, 3, 5, 40, 31
    tile, up, left = _rnd((B, C, h, w), 1), _rnd((B, C, hu, w), 2), _rnd((B, C, h, wl), 3)
    wq, bq = _quant(C, 4) if quant else (None, None)
    if layout == "nchw":
        src = FP.poisoned(tile.reshape(B, C, h * w), ld=h * w + 5, batch_stride=C * (h * w + 5) + 3)
        strides = (src.batch_stride, src.ld, 1)
    else:
        slot = 16 if layout == "nhwc16" else C
        px = torch.full((B, h * w, slot), float("nan")).to(bf16)                 # channels >= C of a padded pixel: poison as well
        px[:, :, :C] = tile.permute(0, 2, 3, 1).reshape(B, h * w, C)
        src = FP.poisoned(px, batch_stride=h * w * slot + 16)
        strides = (src.batch_stride, 1, slot)
    g_up, g_left = FP.poisoned(up.reshape(B * C * hu, w)), FP.poisoned(left.reshape(B * C * h, wl))
    g_wt = FP.poisoned(VE.weights(E))
    g_wq, g_bq = (FP.poisoned(wq), FP.poisoned(bq.view(1, C))) if quant else (None, None)
    outs = []
    for clean in (False, True):
        s, u, l, wt, q, qb = (None if g is None else (g.clean() if clean else g) for g in (src, g_up, g_left, g_wt, g_wq, g_bq))
        fin = FP.guarded((B * C * h, w))
        mom = FP.guarded((B * C * HL, WL))
        rc = lib.da_vae_moments_tile_blend(s.ptr(), *strides, q.ptr() if quant else None, qb.ptr() if quant else None, u.ptr(), hu, l.ptr(),
                                           wl, wt.ptr(), E, fin.ptr(), mom.ptr(), B, Lc, h, w, keep_h, keep_w, HL, WL, y0, x0,
                                           torch.cuda.current_stream().cuda_stream)
        assert rc == L.DA_OK
        torch.cuda.synchronize()
        fin.check("fin"), mom.check("moments")
        placed = torch.zeros((B, C, HL, WL), dtype=torch.bool, device=DEV)
        placed[:, :, y0:y0 + keep_h, x0:x0 + keep_w] = True
        view_bits = mom.view.contiguous().view(torch.int16).reshape(placed.shape)
        assert bool((view_bits[~placed] == 0).all()), "the moments outside the placed rectangle were written"
        assert bool(torch.isfinite(fin.view.float()).all()) and bool(torch.isfinite(mom.view.float()).all())
        outs.append((fin.view.clone(), mom.view.clone()))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    want_mom = torch.zeros((B, C, HL, WL), dtype=bf16)
    flat, st = TE.layout_source(tile, layout)
    want_fin = TE.vae_moments_tile_blend(flat, st, batch=B, latent_channels=Lc, height=h, width=w, moments=want_mom, y0=y0, x0=x0,
                                         keep_h=keep_h, keep_w=keep_w, wq=wq, bq=bq, extent=E, up=up, left=left)
    assert same_bits(outs[0][0].reshape(B, C, h, w), want_fin) and same_bits(outs[0][1].reshape(want_mom.shape), want_mom)


def test_refusals_launch_nothing():
    lib = L.load()
    B, Lc, C, h, w, E, hu, wl = 1, 4, 8, 8, 8, 4, 6, 5
    src, up, left = (_rnd(s, i).to(DEV) for i, s in enumerate(((B, C, h, w), (B, C, hu, w), (B, C, h, wl))))
    wq, bq = (t.to(DEV) for t in _quant(C, 0))
    wt = ops.tile_blend_weights(E, DEV)
    fin = torch.full((B, C, h, w), 5.0, dtype=bf16, device=DEV)
    mom = torch.full((B, C, 10, 12), 7.0, dtype=bf16, device=DEV)
    good = dict(src=src, strides=(C * h * w, h * w, 1), wq=wq, bq=bq, up=up, hu=hu, left=left, wl=wl, wt=wt, E=E, fin=fin, mom=mom, B=B,
                Lc=Lc, h=h, w=w, keep_h=6, keep_w=7, HL=10, WL=12, y0=2, x0=3)
    bad = [dict(src=None), dict(mom=None), dict(wt=None), dict(wq=None), dict(bq=None), dict(Lc=0), dict(E=-1), dict(hu=3), dict(wl=3),
           dict(keep_h=9), dict(keep_w=9), dict(keep_h=0), dict(keep_w=0), dict(y0=5), dict(x0=6), dict(y0=-1), dict(x0=-1), dict(B=0),
           dict(h=0), dict(w=0), dict(strides=(-1, h * w, 1)), dict(strides=(C * h * w, -1, 1)), dict(strides=(C * h * w, h * w, -1)),
           dict(HL=7), dict(WL=9), dict(B=65536), dict(h=1 << 16, w=1 << 15)]
    for change in bad:
        assert launch(lib, **dict(good, **change)) == 1, change                  # DA_ERR_INVALID
    # channel counts that are not built: anything but L = 4 and L = 16, and a quant_conv at L = 16
    for change in (dict(Lc=8), dict(Lc=2), dict(Lc=16), dict(Lc=3, wq=None, bq=None)):
        assert launch(lib, **dict(good, **change)) == 3, change                  # DA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((fin == 5.0).all()) and bool((mom == 7.0).all())
    assert launch(lib, **good) == L.DA_OK                                        # ... and the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert not bool((fin == 5.0).all()) and bool((mom[:, :, :2] == 7.0).all()) and not bool((mom[:, :, 2:8, 3:10] == 7.0).any())
    kw = dict(batch=B, latent_channels=Lc, height=h, width=w, moments=mom, y0=0, x0=0, keep_h=6, keep_w=7)
    with pytest.raises(ValueError, match="up must be contiguous"):
        ops.vae_moments_tile_blend(src, (C * h * w, h * w, 1), extent=8, up=up, **kw)
    with pytest.raises(ValueError, match="strides"):
        ops.vae_moments_tile_blend(src, (C * h * w, h * w, 2), **kw)
    with pytest.raises(ValueError, match="come together"):
        ops.vae_moments_tile_blend(src, (C * h * w, h * w, 1), wq=wq, **kw)
    with pytest.raises(NotImplementedError, match="latent_channels = 16 with a quant_conv"):
        ops.vae_moments_tile_blend(torch.zeros(32 * h * w, dtype=bf16, device=DEV), (32 * h * w, h * w, 1),
                                   wq=torch.zeros(32, 32, dtype=bf16, device=DEV), bq=torch.zeros(32, dtype=bf16, device=DEV),
                                   **dict(kw, latent_channels=16, moments=torch.zeros(1, 32, 10, 12, dtype=bf16, device=DEV)))
    with pytest.raises(ValueError, match="rectangle"):
        ops.vae_moments_tile_blend(src, (C * h * w, h * w, 1), **dict(kw, y0=5))


def test_torch_library_op_equals_the_wrapper():
    import diffusers_amd.torch_ops  # noqa: F401
    B, Lc, C, h, w, E = 2, 4, 8, 7, 9, 2
    tile, up = _rnd((B, C, h, w), 1, 2.0).to(DEV), _rnd((B, C, 5, w), 2, 2.0).to(DEV)
    wq, bq = (t.to(DEV) for t in _quant(C, 3))
    mom = _rnd((B, C, 20, 30), 4).to(DEV)
    want_mom = mom.clone()
    want_fin = ops.vae_moments_tile_blend(tile, (C * h * w, h * w, 1), batch=B, latent_channels=Lc, height=h, width=w, moments=want_mom,
                                          y0=3, x0=4, keep_h=6, keep_w=6, wq=wq, bq=bq, extent=E, up=up)
    keep = mom.clone()
    fin, out = torch.ops.mi355x.vae_moments_tile_blend(tile, C * h * w, h * w, 1, wq, bq, up, None, mom, Lc, h, w, E, 3, 4, 6, 6)
    torch.cuda.synchronize()
    assert same_bits(fin, want_fin) and same_bits(out, want_mom) and same_bits(mom, keep) and not same_bits(out, mom)


# ---- the engine's tiled encode ---------------------------------------------------------------------------------------------------
def untiled(vae, src, nchw, normalize):
    """The engine's encode of ``src`` as it is without tiling and slicing, whatever the flags say."""
    saved = vae.use_tiling, vae.use_slicing
    vae.use_tiling = vae.use_slicing = False
    try:
        return type(vae).encode_image(vae, src.contiguous(), nchw=nchw, normalize=normalize)
    finally:
        vae.use_tiling, vae.use_slicing = saved


def engine_reference(vae, src, nchw, normalize, slicing=False):
    """The reference's encode with tiling on, transcribed, over the engine's own UNTILED encodes of each tile; blends on the CPU."""
    return TE.reference_encode(src, lambda t: untiled(vae, t, nchw, normalize).parameters.cpu(), use_tiling=True, use_slicing=slicing,
                               tile_sample_min_size=vae.tile_sample_min_size, tile_latent_min_size=vae.tile_latent_min_size,
                               tile_overlap_factor=vae.tile_overlap_factor, nchw=nchw)


VAES = {"tiny_quant": dinit.TINY_VAE, "tiny_plain": dict(dinit.TINY_VAE, use_quant_conv=False), "tiny_flux": dinit.TINY_FLUX_VAE}


@pytest.fixture(scope="module", params=list(VAES))
def vae_case(request):
    from diffusers_amd import factory
    vae, _ = factory.build_vae(VAES[request.param], seed=1, device=DEV, with_encoder=True)
    assert (vae.encoder.quant_w is not None) == (request.param == "tiny_quant")
    return request.param, vae


def _image(B, H, W, seed):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("H,W", [(32, 32), (40, 28), (26, 40), (64, 64)])
def test_tiled_encode_equals_the_transcribed_reference(vae_case, H, W):
    """Tiles of 16 px (8 latent, overlap_size 12, E = 2): 3 x 3, 4 x 3, 3 x 4 (its last row ONE latent line) and 6 x 6 tiles, from
    every image source, B = 2, sliced and not.  The tiled moments are another tensor than the untiled encode of the whole image
    (tile-wise GroupNorm), which is what the reference gives and what an engine that ignores the flag does not."""
    name, vae = vae_case
    vae.tile_sample_min_size, vae.tile_latent_min_size = 16, 8
    Lc = vae.config.latent_channels
    img = _image(2, H, W, seed=H * 100 + W)
    try:
        for source, slicing in [(s, False) for s in TE.SOURCES] + [("f32_nchw", True)]:
            nchw, normalize = source == "f32_nchw", source != "f32_nhwc"
            src = TE.image_source(img, source).to(DEV)
            want = engine_reference(vae, src, nchw, normalize, slicing)
            vae.enable_tiling()
            if slicing:
                vae.enable_slicing()
            dist = vae.encode_image(src, nchw=nchw, normalize=normalize)
            got = dist.parameters
            vae.disable_tiling(), vae.disable_slicing()
            assert tuple(want.shape) == (2, 2 * Lc, H // 2, W // 2) and bool(torch.isfinite(want.float()).all())
            assert same_bits(got, want), (name, source, slicing, explain(got, want))
            whole = untiled(vae, src, nchw, normalize).parameters
            assert whole.shape == got.shape and not same_bits(whole, want), (name, source)
    finally:
        vae.disable_tiling(), vae.disable_slicing()
        vae.tile_sample_min_size, vae.tile_latent_min_size = 32, 16


def test_tiles_large_enough_for_the_implicit_gemm_conv_out(vae_case, monkeypatch):
    """Tiles of 128 px = 64 x 64 latent pixels: the thin conv_out of the first tile takes the implicit-GEMM route and leaves the
    16-padded channels-last result (the 16-channel VAE: NHWC of 32), the smaller edge tiles the NCHW one -- the strides handed to the
    kernel show it."""
    name, vae = vae_case
    routes, real = set(), ops.conv_thin_out_moments

    def spy(x, w, b):
        y, strides = real(x, w, b)
        routes.add(tuple(strides[1:]))                                           # (sC, sP)
        return y, strides

    vae.tile_sample_min_size, vae.tile_latent_min_size = 128, 64
    src = _image(1, 160, 144, seed=6).to(DEV)
    try:
        want = engine_reference(vae, src, True, True)
        monkeypatch.setattr(ops, "conv_thin_out_moments", spy)
        vae.enable_tiling()
        got = vae.encode_image(src, nchw=True, normalize=True).parameters
    finally:
        vae.disable_tiling()
        vae.tile_sample_min_size, vae.tile_latent_min_size = 32, 16
    assert tuple(got.shape) == (1, 2 * vae.config.latent_channels, 80, 72) and same_bits(got, want), (name, explain(got, want))
    # tiles of 64 x 64, 64 x 24, 32 x 64 and 32 x 24 latent pixels
    assert routes == ({(1, 32)} if name == "tiny_flux" else {(1, ops.THIN_OUT_PAD), (64 * 24, 1), (32 * 64, 1), (32 * 24, 1)}), routes


def test_an_image_no_larger_than_a_tile_is_encoded_as_today(vae_case):
    """32 x 32 px with the tiny VAEs' own 32 px tile: tiling on changes nothing; sliced, the samples go one by one through the
    quant_conv-and-place launch and give the same moments."""
    name, vae = vae_case
    src = (_image(2, 32, 32, seed=5) * 2 - 1).to(DEV)
    off = untiled(vae, src, True, False)
    vae.enable_tiling()
    try:
        on = vae.encode_image(src, nchw=True, normalize=False)
        assert on._strides == off._strides and on._params is None and same_bits(on.parameters, off.parameters)
        assert same_bits(vae.encode(src).latent_dist.parameters, off.parameters)
        vae.enable_slicing()
        sliced = vae.encode_image(src, nchw=True, normalize=False)
        assert sliced._params is not None and same_bits(sliced.parameters, off.parameters)
    finally:
        vae.disable_tiling(), vae.disable_slicing()


def test_posterior_calls_on_the_tiled_distribution(vae_case):
    """sample (with a generator), mode, latents(scale, shift, noise, a, b) and flux_latents on the tiled distribution equal the same
    calls on a distribution built from the transcription's moments."""
    name, vae = vae_case
    vae.tile_sample_min_size, vae.tile_latent_min_size = 16, 8
    Lc = vae.config.latent_channels
    src = (_image(2, 40, 28, seed=9) * 2 - 1).to(DEV)
    try:
        want = engine_reference(vae, src, True, False).to(DEV).contiguous()
        vae.enable_tiling()
        dist = vae.encode_image(src, nchw=True, normalize=False)
    finally:
        vae.disable_tiling()
        vae.tile_sample_min_size, vae.tile_latent_min_size = 32, 16
    ref = DiagonalGaussianDistribution(vae.encoder, want, None, (2, 20, 14), dist._noise_dtype, assembled=True)
    assert dist.latent_shape == ref.latent_shape == (2, Lc, 20, 14)
    assert same_bits(dist.mode(), ref.mode()) and same_bits(dist.mode(), want[:, :Lc])
    assert same_bits(dist.sample(torch.Generator().manual_seed(3)), ref.sample(torch.Generator().manual_seed(3)))
    assert same_bits(dist.mean, want[:, :Lc]) and same_bits(dist.logvar, torch.clamp(want[:, Lc:], -30.0, 20.0))
    assert same_bits(dist.std, torch.exp(0.5 * ref.logvar)) and same_bits(dist.var, torch.exp(ref.logvar))
    eps1, noise = (_rnd((2, Lc, 20, 14), s).to(DEV) for s in (1, 2))
    kw = dict(scale=0.3611, shift=0.1159, noise=noise, a=0.6914, b=0.7227)
    assert same_bits(dist.latents(eps1, **kw), ref.latents(eps1, **kw)) and same_bits(dist.latents(None, **kw), ref.latents(None, **kw))
    # ... and they are the posterior kernel's results on the NCHW moments, not a copy of the inputs
    plain = ops.vae_posterior_latents(want, (2 * Lc * 280, 280, 1), batch=2, hw=280, latent_channels=Lc, mode=L.POSTERIOR_SAMPLE, eps1=eps1,
                                      eps2=noise, **{k: kw[k] for k in ("scale", "shift", "a", "b")})
    assert same_bits(dist.latents(eps1, **kw), plain.view(2, Lc, 20, 14))
    if name == "tiny_quant":
        with pytest.raises(NotImplementedError, match="quant_conv"):
            dist.flux_latents(eps1, noise)
    else:
        fkw = dict(scale=0.3611, shift=0.1159, a=0.4, b=0.6, want_image_latents=True, want_noise=True)
        for e in (eps1, None):
            got, exp = dist.flux_latents(e, noise, **fkw), ref.flux_latents(e, noise, **fkw)
            assert all(same_bits(g, x) for g, x in zip(got, exp)) and tuple(got[0].shape) == (2, 70, 4 * Lc)


# ---- pipelines -------------------------------------------------------------------------------------------------------------------
def _sd_embeds(sdxl, seed=3):
    g = torch.Generator().manual_seed(seed)
    pe, npe = (torch.randn(1, 7, 64, generator=g).to(bf16).to(DEV) for _ in range(2))
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=npe)
    if sdxl:
        te, nte = (torch.randn(1, 64, generator=g).to(bf16).to(DEV) for _ in range(2))
        kw.update(pooled_prompt_embeds=te, negative_pooled_prompt_embeds=nte)
    return kw


def _flux_embeds(seed=3):
    g = torch.Generator().manual_seed(seed)
    return dict(prompt_embeds=torch.randn(1, 16, 64, generator=g).to(bf16).to(DEV),
                pooled_prompt_embeds=torch.randn(1, 64, generator=g).to(bf16).to(DEV), max_sequence_length=16)


def _pipeline(name):
    from diffusers_amd import factory
    m = torch.zeros(48, 64)
    m[12:36, 16:40] = 1.0
    if name == "sdxl_img2img":
        return factory.build_sdxl_pipeline(device=DEV, tiny=True, seed=0, img2img=True), dict(strength=0.6, guidance_scale=5.0, **_sd_embeds(True))
    if name == "sdxl_inpaint":
        return (factory.build_sdxl_pipeline(device=DEV, tiny=True, seed=0, inpaint=True, unet_in_channels=9),
                dict(strength=0.6, guidance_scale=5.0, mask_image=m, **_sd_embeds(True)))
    if name == "sd15_pix2pix":
        return factory.build_sd15_pipeline(device=DEV, tiny=True, seed=0, pix2pix=True), dict(guidance_scale=7.5, image_guidance_scale=1.5, **_sd_embeds(False))
    return factory.build_flux_pipeline(device=DEV, tiny=True, seed=5, img2img=True), dict(strength=0.6, **_flux_embeds())


@pytest.mark.parametrize("name", ["sdxl_img2img", "sdxl_inpaint", "sd15_pix2pix", "flux_img2img"])
def test_pipeline_with_vae_tiling_on_the_encode_side(name, monkeypatch):
    """A 48 x 64 image with the tiny VAEs' 32 px tiles: 2 x 3 tiles.  With tiling on, the pipeline equals the same pipeline fed the
    transcription's moments; eager equals HIP graph; switching the flag recaptures nothing and leaves no trace."""
    pipe, kw = _pipeline(name)
    vae = pipe.vae
    assert [len(r) for r in vae._encode_tile_plan(48, 64)[1]] == [3, 3]
    img = _image(1, 48, 64, seed=4)

    def run(use_graph=True):
        out = pipe(image=img, num_inference_steps=3, output_type="latent", generator=torch.Generator().manual_seed(21), use_graph=use_graph,
                   **kw).images
        torch.cuda.synchronize()
        return out.clone()

    plain = run()
    graph = pipe._graph
    pipe.enable_vae_tiling()
    assert vae.use_tiling is True
    tiled = run()
    assert pipe._graph is graph, "enabling VAE tiling recaptured the step"
    assert tiled.shape == plain.shape and bool(torch.isfinite(tiled.float()).all()) and not torch.equal(tiled, plain)
    assert torch.equal(run(False), tiled), "eager != HIP graph"
    real = type(vae).encode_image
    fed = []

    def transcribed(img_, *, nchw, normalize):
        want = engine_reference(vae, img_, nchw, normalize).to(DEV).contiguous()
        fed.append(tuple(want.shape))
        return DiagonalGaussianDistribution(vae.encoder, want, None, (want.shape[0], want.shape[2], want.shape[3]),
                                            torch.float32 if vae.config.force_upcast else bf16, assembled=True)

    monkeypatch.setattr(vae, "encode_image", transcribed, raising=False)
    assert torch.equal(run(), tiled), "the pipeline's start is not the transcription's moments"
    assert fed == [(1, 2 * vae.config.latent_channels, 24, 32)] * (2 if name == "sdxl_inpaint" else 1)
    monkeypatch.setattr(vae, "encode_image", lambda *a, **k: real(vae, *a, **k), raising=False)
    pipe.disable_vae_tiling()
    assert torch.equal(run(), plain) and pipe._graph is graph, "disabling VAE tiling recaptured the step or left a trace"
