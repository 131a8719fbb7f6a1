"""AutoencoderTiny restated, and CPU stand-ins for the two ops it adds.

The reference package (``models/autoencoders/autoencoder_tiny.py``, ``vae.py`` EncoderTiny / DecoderTiny / AutoencoderTinyBlock) is
not importable by the suite, so its modules are written down once here from their constructors and forwards:

  ``ref_layers``      the ``layers`` Sequential of EncoderTiny / DecoderTiny as a list of callables over a reference state_dict
  ``ref_decode``      ``layers(tanh(x / 3) * 3) * 2 - 1`` after the pipeline's ``latents / scaling_factor (+ shift_factor)``
  ``ref_encode``      ``layers((x + 1) / 2)``
Both run in the dtype asked for: ``torch.float32`` is the reference the engine is held to, ``torch.bfloat16`` is the same graph
with every torch op rounding its result (the "floor": what the reference itself loses in bf16).

Stand-ins (the C ABI's contract, same rounding points as the kernels):
  ``conv2d_nhwc``            ``act == ACT_RELU``: max(bf16(conv + bias + residual), 0), one rounding; any other ``act`` is
                              tests/ops_emulation.py's
  ``tiny_vae_latents_in``    bf16(bf16(tanh(bf16(bf16(bf16(x / d) + a) / m))) * m), NCHW -> NHWC padded to 64 channels

``halo_offsets`` / ``output_offsets`` are the host-side model of the conv kernel's address arithmetic (csrc/conv_c64.hip) in
unbounded Python integers, for the large-offset check."""
import torch
import torch.nn.functional as F

import ops_emulation
import inpaint_emulation

bf16 = torch.bfloat16
ACT_RELU = 7
TH, TW = 8, 32            # the kernel's output tile (rows x pixels)


# ----------------------------------------------------------------------------------------------------------------------
# stand-ins
# ----------------------------------------------------------------------------------------------------------------------
def relu_conv_ref(x, w, bias=None, residual=None):
    """fp32 result BEFORE the rounding: conv3x3(x) + bias + residual on NHWC bf16 operands (w packed [64][9 * 64])."""
    wt = w.float().view(64, 3, 3, 64).permute(0, 3, 1, 2)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), wt, None if bias is None else bias.float(), padding=1).permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual.float()
    return y.contiguous()


def conv2d_nhwc(x, w, bias=None, *, act=0, residual=None, k_valid=0, out=None, **kw):
    if act != ACT_RELU:
        return ops_emulation.conv2d_nhwc(x, w, bias, act=act, residual=residual, k_valid=k_valid, out=out, **kw)
    # what da_gemm_bf16 admits with DA_ACT_RELU
    assert kw.get("ksize", 3) == 3 and kw.get("stride", 1) == 1 and not kw.get("up", False) and kw.get("pad") in (None, 1)
    assert all(kw.get(k) is None for k in ("x2", "rowvec", "gate", "tile", "staging", "split_k")) and kw.get("out_scale", 1.0) == 1.0
    assert x.is_contiguous() and x.shape[-1] == 64 and tuple(w.shape) == (64, 576) and 0 <= k_valid <= 64
    assert residual is None or (tuple(residual.shape) == tuple(x.shape) and residual.is_contiguous())
    assert out is None or residual is None or out.data_ptr() != residual.data_ptr()
    if k_valid:
        assert not x[..., k_valid:].any() and not w.view(64, 9, 64)[..., k_valid:].any()
    y = F.relu(relu_conv_ref(x, w, bias, residual).to(bf16))
    if out is not None:
        out.copy_(y)
        return out
    return y


def _r(t):
    return t.to(bf16).float()


def tiny_vae_latents_in(z, *, in_div=1.0, in_add=0.0, magnitude=3.0):
    assert z.dtype == bf16 and z.dim() == 4 and 1 <= z.shape[1] <= 16
    # The chain is spelled in fp32 with each rounding explicit and the scalars at fp32, as the device evaluates a bf16 tensor op with a
    # Python scalar: torch's CPU kernels round such a scalar to bf16 first in some positions (tests/lcm_emulation.py has the same note).
    x = z.float()
    if in_div != 1.0:
        x = _r(x / in_div)
    if in_add != 0.0:
        x = _r(x + in_add)
    x = _r(_r(torch.tanh(_r(x / magnitude))) * magnitude)
    B, Lc, H, W_ = z.shape
    y = torch.zeros((B, H, W_, 64), dtype=bf16)
    y[..., :Lc] = x.permute(0, 2, 3, 1).to(bf16)
    return y


def install(monkeypatch, ops_module):
    """tests/inpaint_emulation.py's stand-ins (tests/ops_emulation.py's plus the image loader) and the two above."""
    inpaint_emulation.install(monkeypatch, ops_module)
    monkeypatch.setattr(ops_module, "conv2d_nhwc", conv2d_nhwc)
    monkeypatch.setattr(ops_module, "tiny_vae_latents_in", tiny_vae_latents_in)


# ----------------------------------------------------------------------------------------------------------------------
# the reference modules restated
# ----------------------------------------------------------------------------------------------------------------------
def _conv(sd, p, dtype, stride=1):
    w = sd[p + ".weight"].to(dtype)
    b = sd[p + ".bias"].to(dtype) if (p + ".bias") in sd else None
    return lambda x: F.conv2d(x, w, b, stride=stride, padding=1)


def _block(sd, p, dtype):
    c0, c2, c4 = (_conv(sd, f"{p}.conv.{i}", dtype) for i in (0, 2, 4))
    return lambda x: F.relu(c4(F.relu(c2(F.relu(c0(x))))) + x)           # fuse(conv(x) + skip(x)), skip = Identity


def ref_layers(sd, cfg, half, dtype):
    """EncoderTiny.__init__ / DecoderTiny.__init__ (vae.py): the Sequential, index by index."""
    layers = []
    p = lambda: f"{half}.layers.{len(layers)}"                            # noqa: E731
    if half == "encoder":
        for i, nb in enumerate(cfg["num_encoder_blocks"]):
            layers.append(_conv(sd, p(), dtype) if i == 0 else _conv(sd, p(), dtype, stride=2))
            for _ in range(nb):
                layers.append(_block(sd, p(), dtype))
        layers.append(_conv(sd, p(), dtype))
    else:
        layers.append(_conv(sd, p(), dtype))
        layers.append(F.relu)
        n = len(cfg["num_decoder_blocks"])
        for i, nb in enumerate(cfg["num_decoder_blocks"]):
            for _ in range(nb):
                layers.append(_block(sd, p(), dtype))
            if i != n - 1:
                layers.append(lambda x: F.interpolate(x, scale_factor=cfg["upsampling_scaling_factor"], mode=cfg["upsample_fn"]))
            layers.append(_conv(sd, p(), dtype))
    return layers


def ref_decode(sd, cfg, z, dtype=torch.float32, latents_div=1.0, latents_add=0.0):
    """The pipeline's ``latents / scaling_factor (+ shift_factor)`` then DecoderTiny.forward; NCHW in ``dtype``."""
    x = z.to(dtype)
    if latents_div != 1.0:
        x = x / latents_div
    if latents_add != 0.0:
        x = x + latents_add
    x = torch.tanh(x / 3) * 3
    for f in ref_layers(sd, cfg, "decoder", dtype):
        x = f(x)
    return x.mul(2).sub(1)


def ref_encode(sd, cfg, x, dtype=torch.float32):
    """EncoderTiny.forward on an NCHW image in [-1, 1]."""
    x = x.to(dtype).add(1).div(2)
    for f in ref_layers(sd, cfg, "encoder", dtype):
        x = f(x)
    return x


def ref_postprocess(img, mode):
    """VaeImageProcessor.postprocess on the decoder output: denormalize, clamp; "np" -> NHWC; "uint8" -> (x * 255).round() bytes."""
    v = (img.float() / 2 + 0.5).clamp(0, 1)
    if mode == "pt":
        return v
    v = v.permute(0, 2, 3, 1).contiguous()
    return v if mode == "np" else (v * 255).round().to(torch.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# host-side model of csrc/conv_c64.hip's address arithmetic (element offsets, unbounded integers)
# ----------------------------------------------------------------------------------------------------------------------
def tiles(B, H, W):
    tx, ty = -(-W // TW), -(-H // TH)
    for t in range(B * tx * ty):
        b, r = divmod(t, tx * ty)
        yy, xx = divmod(r, tx)
        yield b, yy * TH, xx * TW


def halo_offsets(b, y0, x0, H, W, wrap=None):
    """First-element offsets of the 16-byte chunks one tile loads: ``(offset, inside)`` per chunk of the 10 x 34 pixel halo; pixels
    outside the image read the clamped pixel.  ``wrap``: evaluate the sum in that many bits (the bug class the check is for)."""
    out = []
    for c in range((TH + 2) * (TW + 2) * 8):
        p, q = divmod(c, 8)
        hy, hx = divmod(p, TW + 2)
        iy, ix = y0 + hy - 1, x0 + hx - 1
        cy, cx = min(max(iy, 0), H - 1), min(max(ix, 0), W - 1)
        off = ((b * H + cy) * W + cx) * 64 + q * 8
        if wrap:
            off &= (1 << wrap) - 1
        out.append((off, 0 <= iy < H and 0 <= ix < W))
    return out


def output_offsets(b, y0, x0, H, W, wrap=None):
    """First-element offsets of the 8-byte stores (and residual loads) of one tile: lane (row `wave`, pixel r, half h), group (mt, g)."""
    out = []
    for wave in range(TH):
        for r in range(TW):
            oy, ox = y0 + wave, x0 + r
            if oy >= H or ox >= W:
                continue
            for h in range(2):
                o = ((b * H + oy) * W + ox) * 64 + 4 * h
                for mt in range(2):
                    for g in range(4):
                        off = o + mt * 32 + 8 * g
                        out.append(off & ((1 << wrap) - 1) if wrap else off)
    return out
