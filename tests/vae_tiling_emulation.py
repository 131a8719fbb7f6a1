"""TEST INFRASTRUCTURE ONLY: the tiled AutoencoderKL.decode restated with torch ops.

Three things live here, each independent of the code under test:

* ``blend`` / ``weights``: the arithmetic contract of ``da_vae_tile_blend`` (include/diffusers_amd.h) -- fp32 products and sum, a bf16
  rounding after each, the two weights evaluated in float64 and stored as fp32.  tests/test_vae_tiling_cpu.py holds it against
  torch's own bf16 ``a * (1 - y / E) + b * (y / E)``.
* ``vae_tile_blend``: a stand-in for ``ops.vae_tile_blend`` with the same signature, on any device (the CPU tests run the host
  tiling logic of AutoencoderKL on it; the GPU tests compare the kernel with it to the bit).
* ``reference_tiled_decode``: a literal transcription of the reference's ``tiled_decode`` / ``blend_v`` / ``blend_h`` -- in-place
  blends with bf16 torch ops, crops, concatenations -- over any per-tile decoder, and ``postprocess``: the image processor's
  arithmetic as ``da_nhwc_take_postprocess`` states it (``postprocess_image``).
"""
from __future__ import annotations

import torch

bf16 = torch.bfloat16
MODES = (None, "pt", "np", "uint8")


def weights(E: int) -> torch.Tensor:
    """fp32 [E][2] = (float32(1 - k / E), float32(k / E)), evaluated in float64 first."""
    return torch.tensor([[1 - k / E, k / E] for k in range(E)], dtype=torch.float64).reshape(E, 2).float()


def _rb(x: torch.Tensor) -> torch.Tensor:
    return x.to(bf16).float()


def blend(a: torch.Tensor, b: torch.Tensor, w0: torch.Tensor, w1: torch.Tensor) -> torch.Tensor:
    """bf16(bf16(float(a) * w0) + bf16(float(b) * w1)); ``w0`` / ``w1`` fp32, broadcast against the bf16 operands.  A NaN result
    (inf * 0, inf - inf) is the pattern 0x7FC0, as the kernel's contract says: torch has no single answer there (its scalar fp32 ->
    bf16 conversion stores 0x7FC0, the vectorised CPU one 0xFFFF), every other result is what torch's bf16 ops give."""
    r = (_rb(a.float() * w0) + _rb(b.float() * w1)).to(bf16).contiguous()
    r.view(torch.int16)[r != r] = 0x7FC0
    return r


def postprocess_image(img: torch.Tensor, mode):
    """NCHW bf16 decoder output -> what ``decode(postprocess=mode)`` returns: clamp(x * 0.5 + 0.5, 0, 1) with fmaxf / fminf's
    treatment of a NaN (it becomes 0), then "pt": NCHW fp32, "np": NHWC fp32, "uint8": NHWC round-half-even(255 x)."""
    if mode is None:
        return img
    x = img.float() * 0.5 + 0.5
    x = torch.where(x != x, torch.zeros_like(x), x).clamp(0.0, 1.0)
    if mode == "pt":
        return x
    x = x.permute(0, 2, 3, 1).contiguous()
    return x if mode == "np" else (x * 255.0).round().to(torch.uint8)


def read_strided(src: torch.Tensor, strides, B: int, C: int, h: int, w: int) -> torch.Tensor:
    """Element (b, c, y, x) of the tile at flat offset b sB + c sC + (y w + x) sP of ``src``: NCHW bf16 [B][C][h][w]."""
    sB, sC, sP = (int(s) for s in strides)
    flat = src.reshape(-1)
    return flat.as_strided((B, C, h, w), (sB, sC, w * sP, sP), flat.storage_offset()).clone()


def vae_tile_blend(src, strides, *, batch, channels, height, width, image, y0, x0, keep_h, keep_w, postprocess=None, extent=0,
                   up=None, left=None, want_fin=True):
    """Stand-in for ``ops.vae_tile_blend``: the same arguments, result and effect on ``image``, with torch ops."""
    B, C, h, w, E = int(batch), int(channels), int(height), int(width), int(extent)
    v = read_strided(src, strides, B, C, h, w)
    dev = v.device
    if up is not None and E > 0:
        hu = up.shape[2]
        assert tuple(up.shape) == (B, C, hu, w) and hu >= E
        n = min(hu, h, E)
        wt = weights(E).to(dev)
        v[:, :, :n] = blend(up[:, :, hu - E:hu - E + n], v[:, :, :n], wt[:n, 0].view(1, 1, n, 1), wt[:n, 1].view(1, 1, n, 1))
    if left is not None and E > 0:
        wl = left.shape[3]
        assert tuple(left.shape) == (B, C, h, wl) and wl >= E
        n = min(wl, w, E)
        wt = weights(E).to(dev)
        v[:, :, :, :n] = blend(left[:, :, :, wl - E:wl - E + n], v[:, :, :, :n], wt[:n, 0].view(1, 1, 1, n), wt[:n, 1].view(1, 1, 1, n))
    piece = postprocess_image(v[:, :, :keep_h, :keep_w], postprocess)
    if postprocess in ("np", "uint8"):
        image[:, y0:y0 + keep_h, x0:x0 + keep_w, :] = piece
    else:
        image[:, :, y0:y0 + keep_h, x0:x0 + keep_w] = piece
    return v if want_fin else None


# ---- the reference, transcribed -------------------------------------------------------------------------------------------------
def blend_v(a: torch.Tensor, b: torch.Tensor, E: int) -> torch.Tensor:
    for y in range(min(a.shape[2], b.shape[2], E)):
        b[:, :, y, :] = a[:, :, -E + y, :] * (1 - y / E) + b[:, :, y, :] * (y / E)
    return b


def blend_h(a: torch.Tensor, b: torch.Tensor, E: int) -> torch.Tensor:
    for x in range(min(a.shape[3], b.shape[3], E)):
        b[:, :, :, x] = a[:, :, :, -E + x] * (1 - x / E) + b[:, :, :, x] * (x / E)
    return b


def reference_tiled_decode(z: torch.Tensor, decode_tile, *, tile_latent_min_size: int, tile_sample_min_size: int,
                           tile_overlap_factor: float = 0.25) -> torch.Tensor:
    """``AutoencoderKL.tiled_decode`` of the reference with ``decode_tile(z_slice) -> NCHW bf16`` in place of
    ``decoder(post_quant_conv(.))``; bf16 torch ops on the tiles' device."""
    overlap_size = int(tile_latent_min_size * (1 - tile_overlap_factor))
    blend_extent = int(tile_sample_min_size * tile_overlap_factor)
    row_limit = tile_sample_min_size - blend_extent
    rows = []
    for i in range(0, z.shape[2], overlap_size):
        row = []
        for j in range(0, z.shape[3], overlap_size):
            tile = z[:, :, i:i + tile_latent_min_size, j:j + tile_latent_min_size]
            row.append(decode_tile(tile).clone())
        rows.append(row)
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = blend_v(rows[i - 1][j], tile, blend_extent)
            if j > 0:
                tile = blend_h(row[j - 1], tile, blend_extent)
            result_row.append(tile[:, :, :row_limit, :row_limit])
        result_rows.append(torch.cat(result_row, dim=3))
    return torch.cat(result_rows, dim=2)


def standin_decoder(scale: int = 2, out_channels: int = 3):
    """A deterministic per-tile "decoder" for the host-logic tests: NCHW bf16 latents -> NCHW bf16 [B][out_channels][scale h][scale w]
    whose values depend on the tile's content AND on its size (as tile-wise GroupNorm makes the real one), nothing more."""
    def decode(zt: torch.Tensor) -> torch.Tensor:
        B, L, h, w = zt.shape
        up = zt.float().repeat_interleave(scale, 2).repeat_interleave(scale, 3)
        yy = torch.arange(scale * h, dtype=torch.float32).view(1, 1, -1, 1)
        xx = torch.arange(scale * w, dtype=torch.float32).view(1, 1, 1, -1)
        chans = [up[:, c % L:c % L + 1] * (1.0 + 0.25 * c) + 0.03125 * yy - 0.015625 * xx + 0.001 * (h * 31 + w) for c in range(out_channels)]
        return torch.cat(chans, 1).to(bf16)
    return decode
