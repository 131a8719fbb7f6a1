"""Image resizing on the GPU: da_resample_u8 against PIL.Image.resize to the bit on both routes and every tile, its footprint,
da_gather_resize against F.interpolate, and the pipelines' switch against the same pipeline fed Pillow's own resize."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import call_sequences as CS
import footprint as FP
import image_resize_emulation as RE
from diffusers_amd import _lib as L, factory, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
PIL_FILTER = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
ONE, TWO = L.RESAMPLE_ONE_LAUNCH, L.RESAMPLE_TWO_LAUNCH
# (shape, the route and tile of the automatic choice for lanczos RGB).  After the issue's list: 20 x 30 -> 33 x 65 is one more than the
# largest tile both ways; 120 x 160 -> 24 x 32 and 200 x 200 -> 40 x 40 outgrow the 32 x 64 and the 16 x 32 tile's 64 KiB of LDS;
# 400 x 400 -> 4 x 4 fits no tile for any filter or channel count.
CASES = [(s, ONE, (32, 64)) for s in RE.SHAPES] + [
    (((20, 30), (33, 65)), ONE, (32, 64)), (((120, 160), (24, 32)), ONE, (16, 32)), (((200, 200), (40, 40)), ONE, (8, 16)),
    (((400, 400), (4, 4)), TWO, (0, 0))]


def _images(hi, wi, C):
    """A batch of four different images: seeded random bytes, all 0, all 255, a 0 / 255 checkerboard."""
    rnd = torch.randint(0, 256, (hi, wi, C), generator=torch.Generator().manual_seed(hi * wi + C), dtype=torch.uint8)
    board = ((torch.arange(hi).view(hi, 1, 1) + torch.arange(wi).view(1, wi, 1)) % 2 * 255).to(torch.uint8).expand(hi, wi, C)
    return torch.stack([rnd, torch.zeros_like(rnd), torch.full_like(rnd, 255), board]).contiguous()


def _pillow(batch, size, filter):
    out = [np.asarray(Image.fromarray(a.numpy().squeeze(-1) if a.shape[-1] == 1 else a.numpy()).resize(size[::-1], PIL_FILTER[filter]))
           for a in batch]
    return torch.from_numpy(np.stack(out)).reshape(len(batch), *size, -1)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("filter", list(PIL_FILTER))
@pytest.mark.parametrize("shape,route,tile", CASES, ids=str)
def test_resample_equals_pillow(shape, route, tile, filter, C):
    (hi, wi), size = shape
    got_route, got_tile, ws = ops.resample_route(4, (hi, wi), size, C, filter)
    assert got_route == route and (ws > 0) == (route == TWO) and (got_tile == tile or (filter, C) != ("lanczos", 3))
    src = _images(hi, wi, C)
    want = _pillow(src, size, filter)
    assert torch.equal(ops.resample_u8(src.to(DEV), size, filter).cpu(), want)                    # the automatic route
    assert torch.equal(ops.resample_u8(src.to(DEV), size, filter, route=TWO).cpu(), want)         # integer sums: any split, same bytes
    assert shape[0] != shape[1] or torch.equal(want, src)


@pytest.mark.parametrize("route", [ONE, TWO])
def test_footprint(route):
    """dst and the workspace are written inside their footprint only; the bytes around src (the whole 16-byte lines the one-launch route
    stages reach into them) do not reach the result."""
    (hi, wi), (ho, wo), C, B = (37, 53), (16, 24), 3, 2
    src = _images(hi, wi, C)[:B].contiguous()
    nbytes = ops.resample_route(B, (hi, wi), (ho, wo), C, "lanczos", route)[2]
    assert (route == TWO) == (nbytes == B * hi * wo * C)
    tabs = [t.to(DEV) for n in ((wi, wo), (hi, ho)) for t in ops.resample_tables(*n, "lanczos")[:2]]
    ks = [ops.resample_tables(*n, "lanczos")[2] for n in ((wi, wo), (hi, ho))]
    outs = []
    for gs in (FP.poisoned(src), FP.poisoned(src).clean()):
        gd, gw = FP.guarded((B, ho, wo, C), dtype=torch.uint8), FP.guarded(max(nbytes, 16), dtype=torch.uint8)
        rc = L.load().da_resample_u8(gs.ptr(), gd.ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), ks[0], tabs[2].data_ptr(),
                                     tabs[3].data_ptr(), ks[1], gw.ptr(), nbytes, B, hi, wi, ho, wo, C, route, ops._stream())
        torch.cuda.synchronize()
        assert rc == L.DA_OK
        gd.check("dst"), gw.check("workspace"), gs.check("src")
        outs.append(gd.view.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], _pillow(src, (ho, wo), "lanczos"))
    # refusals launch nothing
    args = lambda **o: [o.get(k, v) for k, v in dict(  # noqa: E731
        src=gs.ptr(), dst=gd.ptr(), hc=tabs[0].data_ptr(), hb=tabs[1].data_ptr(), ksh=ks[0], vc=tabs[2].data_ptr(), vb=tabs[3].data_ptr(),
        ksv=ks[1], ws=gw.ptr(), nbytes=nbytes, B=B, hi=hi, wi=wi, ho=ho, wo=wo, C=C, route=route).items()] + [ops._stream()]
    before = gd.snapshot()
    for over in (dict(C=2), dict(C=4), dict(B=0), dict(ho=0), dict(hc=None), dict(vb=None)) + ((dict(nbytes=nbytes - 1), dict(ws=None))
                                                                                                  if route == TWO else ()):
        assert L.load().da_resample_u8(*args(**over)) == 3, over                                  # DA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(gd.snapshot(), before)


@pytest.mark.parametrize("dtype,nchw", [(torch.float32, True), (torch.uint8, False), (torch.float32, False)])
@pytest.mark.parametrize("size", [(16, 24), (40, 7), (37, 53)])
def test_gather_resize_equals_interpolate(size, dtype, nchw):
    x = torch.randn(2, 3, 37, 53, generator=torch.Generator().manual_seed(1))
    x = (x * 64 + 128).clamp(0, 255).to(dtype) if dtype == torch.uint8 else x
    want = F.interpolate(x.float(), size=size).to(dtype)
    to = (lambda t: t) if nchw else (lambda t: t.permute(0, 2, 3, 1).contiguous())
    assert FP.bits_equal(ops.gather_resize(to(x).to(DEV), size, nchw=nchw).cpu(), to(want))


def _photo(h, w, seed, mode="RGB"):
    a = np.random.default_rng(seed).integers(0, 256, size=(h, w, 3) if mode == "RGB" else (h, w), dtype=np.uint8)
    return Image.fromarray(a)


PIPES = {
    "sd15_img2img": (lambda: factory.build_sd15_pipeline(device=DEV, tiny=True, seed=0, img2img=True), CS._sd_kwargs(False, strength=0.5)),
    "sd15_inpaint": (lambda: factory.build_sd15_pipeline(device=DEV, tiny=True, seed=0, inpaint=True), CS._sd_kwargs(False, strength=0.5)),
    "sd15_controlnet": (lambda: factory.build_sd15_pipeline(device=DEV, tiny=True, seed=0, controlnet=True), CS._sd_kwargs(False)),
    "flux_img2img": (lambda: factory.build_flux_pipeline(device=DEV, tiny=True, seed=5, img2img=True), CS._flux_kwargs(strength=0.6)),
}


@pytest.mark.parametrize("name", list(PIPES))
def test_pipelines_resize_as_pillow_does(name):
    """Switch on + a PIL image of an odd size == switch off + Pillow's LANCZOS resize of it, to the bit; eager == captured graph; an
    image of another size that resizes to the same target replays the captured step."""
    build, kw = PIPES[name]
    pipe = build()
    h, w = 32, 48                                               # 33 x 49 and 32 x 49 both round down to it for any scale factor <= 16
    inputs = lambda hh, ww, seed: dict(image=_photo(hh, ww, seed), **(  # noqa: E731
        dict(mask_image=_photo(hh, ww, seed + 1, "L")) if name == "sd15_inpaint" else {}))
    first, other = inputs(h + 1, w + 1, 7), inputs(h, w + 1, 9)
    pipe.enable_image_resize()
    eager = CS.run(pipe, dict(kw, **first), False)
    graph = CS.run(pipe, dict(kw, **first), True)
    assert torch.equal(eager, graph) and bool(torch.isfinite(graph.float()).all())
    captured = pipe._graph
    again = CS.run(pipe, dict(kw, **other), True)
    assert pipe._graph is captured and torch.equal(again, CS.run(pipe, dict(kw, **other), False))
    pipe.disable_image_resize()
    with pytest.raises(ValueError):
        CS.run(pipe, dict(kw, **first), True)
    by_pillow = {k: v.convert("L").resize((w, h), Image.LANCZOS) if k == "mask_image" else v.resize((w, h), Image.LANCZOS)
                 for k, v in first.items()}
    assert torch.equal(CS.run(pipe, dict(kw, **by_pillow), True), graph)
