"""TEST INFRASTRUCTURE ONLY: the tiled / sliced AutoencoderKL.encode restated with torch ops.

Four things live here, each independent of the code under test:

* ``quant_conv``: the arithmetic contract of the first line of ``da_vae_moments_tile_blend`` (include/diffusers_amd.h) -- an fp32
  accumulator that starts at the bias, the channels added in ascending order (a product of two bf16 values is exact in fp32, so the
  kernel's fma chain is this multiply-add chain), one rounding to bf16.  The blends are ``vae_tiling_emulation.blend`` / ``weights``.
* ``vae_moments_tile_blend``: a stand-in for ``ops.vae_moments_tile_blend`` with the same signature, on any device (the CPU tests
  run the host tiling logic of AutoencoderKL on it; the GPU tests compare the kernel with it to the bit).
* ``reference_tiled_encode`` / ``reference_encode``: a literal transcription of the reference's ``_tiled_encode`` / ``blend_v`` /
  ``blend_h`` / ``encode`` (models/autoencoders/autoencoder_kl.py) -- in-place blends with bf16 torch ops, crops, concatenations --
  over any per-tile ``encode_tile(image slice) -> NCHW bf16 moments`` (the encoder AND the quant_conv).
* ``StandinEncoder``: a deterministic per-tile "encoder" for the host-logic tests.
"""
from __future__ import annotations

import torch

import vae_tiling_emulation as VE

bf16 = torch.bfloat16
LAYOUTS = ("nchw", "nhwc16", "nhwc")                        # what ops.conv_thin_out_moments can return
SOURCES = ("f32_nchw", "f32_nhwc", "u8_nhwc")               # what ops.vae_conv_in_image accepts


def quant_conv(x: torch.Tensor, wq, bq) -> torch.Tensor:
    """x: NCHW bf16 [B][2L][h][w] -> bf16(bq[o] + sum_k wq[o][k] x[k]), k ascending in fp32; ``wq`` None: x itself."""
    if wq is None:
        return x.clone()
    xf = x.float()
    acc = bq.float().view(1, -1, 1, 1).expand(x.shape[0], -1, x.shape[2], x.shape[3]).clone()
    for k in range(x.shape[1]):
        acc = acc + wq[:, k].float().view(1, -1, 1, 1) * xf[:, k:k + 1]
    return acc.to(bf16)


def layout_source(tile: torch.Tensor, layout: str, pad: torch.Tensor = None):
    """The tile [B][C][h][w] as the conv would have left it: ``(flat buffer, (sB, sC, sP))``.  "nchw": planes; "nhwc16": pixels of 16
    channels whose channels >= C hold ``pad``'s values (zeros without); "nhwc": pixels of exactly C channels."""
    B, C, h, w = tile.shape
    if layout == "nchw":
        return tile.reshape(-1).clone(), (C * h * w, h * w, 1)
    px = tile.permute(0, 2, 3, 1).reshape(B, h * w, C)
    if layout == "nhwc":
        return px.reshape(-1).clone(), (h * w * C, 1, C)
    assert layout == "nhwc16" and C <= 16
    buf = torch.zeros((B, h * w, 16), dtype=tile.dtype, device=tile.device) if pad is None else pad.clone()
    buf[:, :, :C] = px
    return buf.reshape(-1), (h * w * 16, 1, 16)


def vae_moments_tile_blend(src, strides, *, batch, latent_channels, height, width, moments, y0, x0, keep_h, keep_w, wq=None, bq=None,
                           extent=0, up=None, left=None, want_fin=True):
    """Stand-in for ``ops.vae_moments_tile_blend``: the same arguments, result and effect on ``moments``, with torch ops."""
    B, C, h, w, E = int(batch), 2 * int(latent_channels), int(height), int(width), int(extent)
    v = quant_conv(VE.read_strided(src, strides, B, C, h, w), wq, bq)
    if up is not None and E > 0:
        hu = up.shape[2]
        assert tuple(up.shape) == (B, C, hu, w) and hu >= E
        n = min(hu, h, E)
        wt = VE.weights(E).to(v.device)
        v[:, :, :n] = VE.blend(up[:, :, hu - E:hu - E + n], v[:, :, :n], wt[:n, 0].view(1, 1, n, 1), wt[:n, 1].view(1, 1, n, 1))
    if left is not None and E > 0:
        wl = left.shape[3]
        assert tuple(left.shape) == (B, C, h, wl) and wl >= E
        n = min(wl, w, E)
        wt = VE.weights(E).to(v.device)
        v[:, :, :, :n] = VE.blend(left[:, :, :, wl - E:wl - E + n], v[:, :, :, :n], wt[:n, 0].view(1, 1, 1, n), wt[:n, 1].view(1, 1, 1, n))
    assert tuple(moments.shape[:2]) == (B, C)
    moments[:, :, y0:y0 + keep_h, x0:x0 + keep_w] = v[:, :, :keep_h, :keep_w]
    return v if want_fin else None


# ---- the reference, transcribed -------------------------------------------------------------------------------------------------
def reference_tiled_encode(x: torch.Tensor, encode_tile, *, tile_sample_min_size: int, tile_latent_min_size: int,
                           tile_overlap_factor: float = 0.25, nchw: bool = True) -> torch.Tensor:
    """``AutoencoderKL._tiled_encode`` of the reference with ``encode_tile(image slice) -> NCHW bf16 moments`` in place of
    ``quant_conv(encoder(.))``; the blends are bf16 torch ops on the moments' device.  ``nchw`` False: ``x`` is an NHWC source of the
    engine (the reference's tensor is NCHW; only the slicing differs)."""
    overlap_size = int(tile_sample_min_size * (1 - tile_overlap_factor))
    blend_extent = int(tile_latent_min_size * tile_overlap_factor)
    row_limit = tile_latent_min_size - blend_extent
    H, W = (x.shape[2], x.shape[3]) if nchw else (x.shape[1], x.shape[2])
    S = tile_sample_min_size
    rows = []
    for i in range(0, H, overlap_size):
        row = []
        for j in range(0, W, overlap_size):
            tile = x[:, :, i:i + S, j:j + S] if nchw else x[:, i:i + S, j:j + S, :]
            row.append(encode_tile(tile.contiguous()).clone())
        rows.append(row)
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = VE.blend_v(rows[i - 1][j], tile, blend_extent)
            if j > 0:
                tile = VE.blend_h(row[j - 1], tile, blend_extent)
            result_row.append(tile[:, :, :row_limit, :row_limit])
        result_rows.append(torch.cat(result_row, dim=3))
    return torch.cat(result_rows, dim=2)


def reference_encode(x: torch.Tensor, encode_tile, *, use_tiling: bool, use_slicing: bool, tile_sample_min_size: int,
                     tile_latent_min_size: int, tile_overlap_factor: float = 0.25, nchw: bool = True) -> torch.Tensor:
    """``AutoencoderKL.encode`` / ``_encode`` of the reference up to the moments: tiled when ``use_tiling`` and the image is larger
    than a tile either way, sample by sample when ``use_slicing`` and B > 1."""
    H, W = (x.shape[2], x.shape[3]) if nchw else (x.shape[1], x.shape[2])

    def _encode(xs):
        if use_tiling and (W > tile_sample_min_size or H > tile_sample_min_size):
            return reference_tiled_encode(xs, encode_tile, tile_sample_min_size=tile_sample_min_size,
                                          tile_latent_min_size=tile_latent_min_size, tile_overlap_factor=tile_overlap_factor, nchw=nchw)
        return encode_tile(xs)

    if use_slicing and x.shape[0] > 1:
        return torch.cat([_encode(x[b:b + 1]) for b in range(x.shape[0])], 0)
    return _encode(x)


# ---- stand-ins for the host-logic tests --------------------------------------------------------------------------------------------
def image_source(img01: torch.Tensor, source: str) -> torch.Tensor:
    """An NCHW fp32 image in [0, 1] as one of the engine's sources ("u8_nhwc" quantises it to bytes)."""
    if source == "f32_nchw":
        return img01.contiguous()
    nhwc = img01.permute(0, 2, 3, 1).contiguous()
    return nhwc if source == "f32_nhwc" else (nhwc * 255.0).round().to(torch.uint8)


class StandinEncoder:
    """Takes the place of ``autoencoder_kl._Encoder``: ``(image slice, nchw=, normalize=) -> (raw, strides)`` with 2 L channels at
    1 / ``down`` of the size, whose values depend on the slice's content AND on its size (as tile-wise GroupNorm makes the real one's),
    nothing more; ``layout`` is how the result is left in memory.  ``moments(slice)`` is the same followed by the quant_conv: what
    the transcription's ``encode_tile`` needs.  Every call is recorded in ``calls`` as the slice's shape."""

    def __init__(self, latent_channels: int = 4, down: int = 2, quant: bool = True, layout: str = "nchw", seed: int = 0):
        self.latent_channels, self.down, self.layout = latent_channels, down, layout
        self.quant_w = self.quant_b = None
        if quant:
            g = torch.Generator().manual_seed(seed)
            C = 2 * latent_channels
            self.quant_w = (torch.randn(C, C, generator=g) * 0.5).to(bf16)
            self.quant_b = (torch.randn(C, generator=g) * 0.1).to(bf16)
        self.calls = []

    def features(self, img: torch.Tensor, nchw: bool, normalize: bool) -> torch.Tensor:
        x = img.float() / 255.0 if img.dtype == torch.uint8 else img.float()
        x = x if nchw else x.permute(0, 3, 1, 2)
        x = 2.0 * x - 1.0 if normalize else x
        B, _, H, W = x.shape
        d = self.down
        assert H % d == 0 and W % d == 0
        h, w = H // d, W // d
        pooled = x.reshape(B, 3, h, d, w, d).mean((3, 5))
        yy = torch.arange(h, dtype=torch.float32).view(1, 1, -1, 1)
        xx = torch.arange(w, dtype=torch.float32).view(1, 1, 1, -1)
        chans = [pooled[:, c % 3:c % 3 + 1] * (1.0 + 0.25 * c) + 0.03125 * yy - 0.015625 * xx + 0.001 * (h * 31 + w) - 0.1 * (c % 5)
                 for c in range(2 * self.latent_channels)]
        return torch.cat(chans, 1).to(bf16)

    def __call__(self, img, *, nchw, normalize):
        self.calls.append(tuple(img.shape))
        return layout_source(self.features(img, nchw, normalize), self.layout)

    def moments(self, img, nchw, normalize) -> torch.Tensor:
        return quant_conv(self.features(img, nchw, normalize), self.quant_w, self.quant_b)
