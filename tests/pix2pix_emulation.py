"""TEST INFRASTRUCTURE ONLY: torch-CPU stand-ins for the two ops entry points the InstructPix2Pix pipelines call on top of those of
tests/inpaint_emulation.py -- ops.conv_in_pix2pix (da_conv_in_inpaint with a NULL mask) and ops.cfg_combine3 (da_cfg_rescale with
DA_CFG_IMAGE_GUIDANCE) -- each with the C ABI's contract and the kernels' rounding points, plus a host-side model of the launch
geometry of the 8-channel conv_in.  The kernels themselves are tested on the GPU (tests/test_pix2pix_gpu.py)."""
from __future__ import annotations

import torch

import inpaint_emulation as I
import ops_emulation as E

bf16 = torch.bfloat16


def pix2pix_concat(xs, image_latents, rep):
    """What the reference hands to conv_in: cat([cat([s(x)] * rep), cat([img, img, zeros_like(img)][:rep])], dim=1); ``xs`` is the
    (scaled) latents repeated ``rep`` times already, ``image_latents`` [Bm][4][H][W] with Bm in {1, B}."""
    B = xs.shape[0] // rep
    img = image_latents.expand(B, -1, -1, -1)
    blocks = [img, img, torch.zeros_like(img)][:rep]
    return torch.cat([xs, torch.cat(blocks, 0)], dim=1).contiguous()


def conv_in_pix2pix(x, image_latents, w, bias, *, table=None, step_idx=None, rep=1):
    B = x.shape[0]
    assert x.shape[1] == 4 and image_latents.shape[0] in (1, B) and image_latents.shape[1] == 4 and w.shape[1] == 72 and rep in (1, 3)
    xs = E.euler_scale_model_input(x, table, step_idx) if table is not None else x
    return E.conv_thin_in(pix2pix_concat(torch.cat([xs] * rep, 0), image_latents, rep), w, bias, ksize=3, in_nchw=True)


def cfg_combine3(eps3b, guidance, image_guidance, out=None):
    """rnd(rnd(u + rnd(g rnd(t - i))) + rnd(ig rnd(i - u))): fp32 arithmetic with the rounding to the tensor dtype written out (torch's
    CPU bf16 kernels round a Python scalar to bf16 first in some positions; the device kernel, like torch on the GPU, does not)."""
    assert eps3b.shape[0] % 3 == 0 and eps3b.dtype in (bf16, torch.float32)
    dt = eps3b.dtype
    g, ig = (float(torch.tensor(v, dtype=torch.float32)) for v in (guidance, image_guidance))

    def r(v):
        return v.to(dt).float()
    t, i, u = (c.float() for c in eps3b.chunk(3))
    y = r(r(u + r(g * r(t - i))) + r(ig * r(i - u))).to(dt)
    if out is not None:
        out.copy_(y)
        return out
    return y


def conv_in_launch_model(B, H, W, Cout, kk=72, block=256, lds_bytes=64 * 1024, grid_cap=768):
    """The chunk / grid arithmetic of da_conv_in_inpaint for a [Cout][kk] weight, and the index decomposition of its kernel:
    returns ``(coc, nchunk, blocks, cover)`` with ``cover`` an int32 [B][H][W][Cout] count of how often each output element of ONE
    copy is stored."""
    coc = (lds_bytes // (kk * 4)) & ~7
    coc = min(coc, Cout)
    nchunk = (Cout + coc - 1) // coc
    cap = max(grid_cap // nchunk, 1)
    wq = (W + 3) // 4
    blocks = min((B * H * wq * (coc // 8) + block - 1) // block, cap)
    cover = torch.zeros(B, H, W, Cout, dtype=torch.int32)
    for by in range(nchunk):
        co0 = by * coc
        ncoc = min(coc, Cout - co0)
        cgroups = ncoc >> 3
        total = B * H * wq * cgroups
        for idx in range(total):                 # the grid-stride loop visits every idx < total exactly once, whatever `blocks` is
            cg, quad = idx % cgroups, idx // cgroups
            x0, yh, b = (quad % wq) * 4, (quad // wq) % H, quad // (wq * H)
            for px in range(4):
                if x0 + px >= W:
                    break
                cover[b, yh, x0 + px, co0 + cg * 8:co0 + cg * 8 + 8] += 1
    return coc, nchunk, blocks, cover


def install(monkeypatch, ops_module):
    """tests/inpaint_emulation.py's stand-ins plus the two above."""
    I.install(monkeypatch, ops_module)
    for name in ("conv_in_pix2pix", "cfg_combine3"):
        monkeypatch.setattr(ops_module, name, globals()[name])
