"""AutoencoderKL.decode and AutoencoderKL.encode on the gfx950 kernels.

Mirrors models/autoencoders/autoencoder_kl.py:199-240 (decode/_decode) and models/autoencoders/vae.py:279-311
(Decoder.forward) with UNetMidBlock2D (unet_2d_blocks.py:736-748) and UpDecoderBlock2D (:2637-2645).  Input latents NCHW
bf16, output image NCHW bf16, as the reference.  The encoder half (autoencoder_kl.py:146-185, Encoder.forward vae.py:140-184
with DownEncoderBlock2D, unet_2d_blocks.py:1421-1502) is packed when the state_dict holds it: its two ends are fused kernels
(the caller's image -> conv_in: ops.vae_conv_in_image; conv_out's result -> quant_conv -> posterior -> latents:
ops.vae_posterior_latents), the trunk reuses the decoder's layers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import ops
from .config_utils import check_to
from .loading import PretrainedMixin
from . import _lib as L
from .layers import Downsample2D, GroupNorm, ResnetBlock2D, Upsample2D, Weights
from .unet_2d_condition import FrozenConfig

bf16 = torch.bfloat16


@dataclass
class DecoderOutput:
    sample: torch.Tensor


_DEFAULTS = dict(
    in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",), up_block_types=("UpDecoderBlock2D",),
    block_out_channels=(64,), layers_per_block=1, act_fn="silu", latent_channels=4, norm_num_groups=32, sample_size=32,
    scaling_factor=0.18215, shift_factor=None, latents_mean=None, latents_std=None, force_upcast=True,
    use_quant_conv=True, use_post_quant_conv=True, mid_block_add_attention=True,
)


class VaeAttention:
    """Legacy single-head Attention block of the VAE mid block (attention_processor.py:2696-2787 with a 4-D input:
    GroupNorm, to_q/k/v WITH bias, residual connection).  head_dim = channels (512 for SD/SDXL): handled as
    scores = Q K^T (fp32) -> row softmax -> P V with the MFMA GEMM; a flash-kernel head size uses the flash kernel.
    The V bias is folded into the output bias (softmax rows sum to 1):  W_o (P (V + 1 b_v^T)) + b_o = W_o P V + (W_o b_v + b_o)."""

    def __init__(self, w: Weights, prefix: str, groups: int, eps: float, heads: int = 1):
        self.group_norm = GroupNorm(w, prefix + ".group_norm", groups, eps)
        wq, wk, wv = (w.get(f"{prefix}.to_{n}.weight") for n in "qkv")
        bq, bk, bv = (w.opt(f"{prefix}.to_{n}.bias") for n in "qkv")
        self.inner = wq.shape[0]
        self.heads = heads
        self.head_dim = self.inner // heads
        self.wqk = torch.cat([wq, wk], 0).contiguous()
        self.bqk = torch.cat([bq, bk], 0).contiguous() if bq is not None else None
        self.wv = wv
        wo = w.get(prefix + ".to_out.0.weight")
        bo = w.opt(prefix + ".to_out.0.bias")
        self.wo = wo
        if bv is not None:
            eff = wo.float() @ bv.float()
            if bo is not None:
                eff = eff + bo.float()
            self.bo = eff.to(bf16).contiguous()
        else:
            self.bo = bo
        self.scale = self.head_dim ** -0.5
        self.force_gemm_path = False

    def __call__(self, x):
        B, H, W_, C = x.shape
        S = H * W_
        res = x.view(B * S, C)
        h = self.group_norm(x).view(B * S, C)
        if S % 8 and self.head_dim in (64, 96, 128, 160) and not self.force_gemm_path:
            # a token count that is no multiple of 8 (the one- and two-line edge tiles of a tiled encode): the flash kernel takes whole
            # groups of 8 ALLOCATED keys, so K and V^T go into zero-padded buffers and Skv masks the keys past S
            S8, n = (S + 7) // 8 * 8, self.inner
            qk = ops.linear(h, self.wqk, self.bqk)
            v = ops.linear(h, self.wv)
            k = torch.zeros((B, S8, n), device=x.device, dtype=bf16)
            k[:, :S] = qk.view(B, S, 2 * n)[:, :, n:]
            vt = torch.zeros((n, B, S8), device=x.device, dtype=bf16)
            vt[:, :, :S] = v.view(B, S, n).permute(2, 0, 1)
            o = ops.attention(qk, k, vt, B=B, H=self.heads, D=self.head_dim, Sq=S, Skv=S, Skv_alloc=S8, q_row_stride=2 * n,
                              k_row_stride=n, q_batch_stride=S * 2 * n, k_batch_stride=S8 * n, vt_ld=B * S8, vt_batch_stride=S8,
                              scale=self.scale)
            return ops.linear(o, self.wo, self.bo, residual=res).view(B, H, W_, C)
        # [B*S][2C] and [C][B*S] (V bias folded into self.bo): one paired launch (layers.Attention)
        qk, vt = ops.linear_pair({"x": h, "w": self.wqk, "bias": self.bqk}, {"x": self.wv, "w": h})
        if self.head_dim in (64, 96, 128, 160) and not self.force_gemm_path:
            o = ops.attention(qk, qk[:, self.inner:], vt, B=B, H=self.heads, D=self.head_dim, Sq=S, Skv=S, Skv_alloc=S,
                              q_row_stride=2 * self.inner, k_row_stride=2 * self.inner,
                              q_batch_stride=S * 2 * self.inner, k_batch_stride=S * 2 * self.inner,
                              vt_ld=B * S, vt_batch_stride=S, scale=self.scale)
        else:
            if self.heads != 1:
                raise ValueError("VaeAttention GEMM path supports a single head")
            # One head of D = 512: scores GEMM (fp32) -> row softmax -> P.V GEMM, in blocks of QBLK query rows so that the score
            # matrix held at any time is QBLK x S (268 MB at S = 16 384 instead of 1 GB + 0.5 GB of probabilities).  Measured
            # (profiles/README.md): the two GEMMs run at ~900 TFLOP/s here; a flash kernel at D = 512 would either recompute Q.K^T per
            # 128-wide output slice (2.5x the flops) or exchange partial scores between waves every tile -- slower than this path.
            o = torch.empty((B * S, C), device=x.device, dtype=bf16)
            QBLK = 4096
            nb = min(QBLK, S)
            scores = torch.empty((nb, S), device=x.device, dtype=torch.float32)
            probs = torch.empty((nb, S), device=x.device, dtype=bf16)
            for b in range(B):
                k = qk[b * S:(b + 1) * S, self.inner:]
                for q0 in range(0, S, nb):
                    n = min(nb, S - q0)
                    q = qk[b * S + q0:b * S + q0 + n, :self.inner]
                    ops.linear(q, k, alpha=self.scale, out_f32=True, out=scores[:n])       # [n][S] fp32
                    ops.softmax_rows(scores[:n], out=probs[:n])                             # [n][S] bf16
                    ops.linear(probs[:n], vt[:, b * S:(b + 1) * S], out=o[b * S + q0:b * S + q0 + n])
        y = ops.linear(o, self.wo, self.bo, residual=res)
        return y.view(B, H, W_, C)


@dataclass
class AutoencoderKLOutput:
    latent_dist: "DiagonalGaussianDistribution"


class _Encoder:
    """Encoder.forward (vae.py:140-184) on NHWC bf16: conv_in, DownEncoderBlock2D x n (resnets, Downsample2D(padding=0) but on the
    last block), mid block (resnet, attention, resnet), conv_norm_out + SiLU, conv_out -> 2 L channels; + quant_conv's weights."""

    def __init__(self, w: Weights, c, groups: int, eps: float):
        boc = tuple(c.block_out_channels)
        self.latent_channels = c.latent_channels
        self.conv_in_w = ops.pack_conv_weight(w.get("encoder.conv_in.weight"))
        self.conv_in_b = w.get("encoder.conv_in.bias")
        self.down = []
        for i in range(len(boc)):
            pre = f"encoder.down_blocks.{i}"
            self.down.append({"resnets": [ResnetBlock2D(w, f"{pre}.resnets.{j}", groups, eps) for j in range(c.layers_per_block)],
                              "down": Downsample2D(w, f"{pre}.downsamplers.0", padding=0) if i != len(boc) - 1 else None})
        self.mid_res0 = ResnetBlock2D(w, "encoder.mid_block.resnets.0", groups, eps)
        self.mid_attn = VaeAttention(w, "encoder.mid_block.attentions.0", groups, eps) if c.mid_block_add_attention else None
        self.mid_res1 = ResnetBlock2D(w, "encoder.mid_block.resnets.1", groups, eps)
        self.conv_norm_out = GroupNorm(w, "encoder.conv_norm_out", groups, eps)
        self.conv_out_w = ops.pack_conv_weight(w.get("encoder.conv_out.weight"))
        self.conv_out_b = w.get("encoder.conv_out.bias")
        self.quant_w = self.quant_b = None
        if c.use_quant_conv:
            qw = w.get("quant_conv.weight")
            self.quant_w = qw.reshape(qw.shape[0], qw.shape[1]).contiguous()
            self.quant_b = w.get("quant_conv.bias")

    def __call__(self, img: torch.Tensor, *, nchw: bool, normalize: bool):
        """Image (fp32 NCHW / NHWC or uint8 NHWC) -> the conv_out result and its strides (ops.conv_thin_out_moments)."""
        x = ops.vae_conv_in_image(img, self.conv_in_w, self.conv_in_b, nchw=nchw, normalize=normalize)
        for st in self.down:
            for rn in st["resnets"]:
                x = rn(x)
            if st["down"] is not None:
                x = st["down"](x)
        x = self.mid_res0(x)
        if self.mid_attn is not None:
            x = self.mid_attn(x)
        x = self.mid_res1(x)
        x = self.conv_norm_out(x, silu=True)
        return ops.conv_thin_out_moments(x, self.conv_out_w, self.conv_out_b)


class DiagonalGaussianDistribution:
    """vae.py:685-718 over the encoder's conv_out result.  ``sample`` / ``mode`` run quant_conv, the posterior and the sampling in one
    kernel (csrc/vae_encode.hip); ``parameters`` / ``mean`` / ``logvar`` / ``std`` / ``var`` are the reference's attributes (the
    quant_conv output from the same kernel, the rest as the reference's bf16 torch ops on it)."""

    def __init__(self, encoder: _Encoder, raw: torch.Tensor, strides, shape, noise_dtype, assembled: bool = False):
        self._enc, self._raw, self._strides = encoder, raw, strides
        self._B, self._H, self._W = shape
        self._noise_dtype = noise_dtype
        self._params = None
        self._wq, self._bq = encoder.quant_w, encoder.quant_b
        if assembled:
            # a tiled / sliced encode: ``raw`` IS the moments [B][2L][H][W] (NCHW, quant_conv applied tile by tile)
            hw = self._H * self._W
            self._strides = (2 * encoder.latent_channels * hw, hw, 1)
            self._params = raw
            self._wq = self._bq = None
        self.deterministic = False

    @property
    def latent_shape(self):
        return (self._B, self._enc.latent_channels, self._H, self._W)

    def _run(self, mode, **kw) -> torch.Tensor:
        e = self._enc
        y = ops.vae_posterior_latents(self._raw, self._strides, batch=self._B, hw=self._H * self._W,
                                      latent_channels=e.latent_channels, mode=mode, wq=self._wq, bq=self._bq, **kw)
        return y.view(self._B, -1, self._H, self._W)

    @property
    def parameters(self) -> torch.Tensor:
        if self._params is None:
            self._params = self._run(L.POSTERIOR_MOMENTS)
        return self._params

    @property
    def mean(self):
        return self.parameters[:, :self._enc.latent_channels]

    @property
    def logvar(self):
        return torch.clamp(self.parameters[:, self._enc.latent_channels:], -30.0, 20.0)

    @property
    def std(self):
        return torch.exp(0.5 * self.logvar)

    @property
    def var(self):
        return torch.exp(self.logvar)

    def draw_noise(self, generator=None, dtype=None) -> torch.Tensor:
        """ε of ``sample``: randn_tensor (utils/torch_utils.py) of the latent shape -- on the generator's device, one draw per
        generator when a list is given -- in the VAE's compute dtype (fp32 for a ``force_upcast`` VAE, as the reference's upcast
        path draws), then bf16 for the kernel."""
        shape, dev = self.latent_shape, self._raw.device
        dtype = dtype or self._noise_dtype
        if isinstance(generator, (list, tuple)):
            if len(generator) != shape[0]:
                raise ValueError(f"{len(generator)} generators for a batch of {shape[0]}")
            draws = [torch.randn((1,) + shape[1:], generator=g, device=g.device, dtype=dtype) for g in generator]
            eps = torch.cat([d.to(dev) for d in draws], 0)
        else:
            gdev = generator.device if generator is not None else dev
            eps = torch.randn(shape, generator=generator, device=gdev, dtype=dtype)
        return eps.to(device=dev, dtype=bf16).contiguous()

    def sample(self, generator=None) -> torch.Tensor:
        return self.latents(self.draw_noise(generator))

    def mode(self) -> torch.Tensor:
        return self.latents(None)

    def latents(self, eps1: Optional[torch.Tensor], *, scale: Optional[float] = None, shift: Optional[float] = None,
                noise: Optional[torch.Tensor] = None, a: float = 1.0, b: float = 0.0) -> torch.Tensor:
        """Engine extension: ``mean + std * eps1`` (``eps1`` None: the mode), then ``(z - shift) * scale`` and
        ``a z + b noise`` (scheduler.add_noise), each as the reference's bf16 op, in one pass."""
        mode = L.POSTERIOR_MEAN if eps1 is None else L.POSTERIOR_SAMPLE
        return self._run(mode, eps1=eps1, eps2=noise, scale=scale, shift=shift, a=a, b=b)

    def flux_latents(self, eps1: Optional[torch.Tensor], noise: torch.Tensor, *, batch: Optional[int] = None,
                     scale: Optional[float] = None, shift: Optional[float] = None, a: float = 0.0, b: float = 1.0,
                     want_image_latents: bool = False, want_noise: bool = False):
        """Engine extension (FLUX img2img / inpainting, ops.flux_prepare_latents): ``latents`` as above, then
        ``scheduler.scale_noise`` = ``a z + b noise`` and FluxPipeline._pack_latents, in one pass; returns the packed
        ``(latents, image_latents or None, noise or None)``, each (B, (h/2)(w/2), 4 L).  A VAE with a quant_conv is refused.  ``batch``
        > this distribution's: the posterior (and ``eps1``) is repeated over it, as the reference repeats the image latents."""
        e = self._enc
        if e.quant_w is not None:
            raise NotImplementedError("flux_latents: VAEs with a quant_conv are not packed by the FLUX prepare kernel")
        B = self._B if batch is None else int(batch)
        raw, (sB, sC, sP) = self._raw, self._strides
        if B != self._B:
            if B % self._B:
                raise ValueError(f"Cannot duplicate `image` of batch size {self._B} to {B} text prompts.")
            rep = B // self._B
            raw = torch.cat([raw] * rep, 0)              # (both layouts are contiguous per image: sB is unchanged)
            if eps1 is not None:
                eps1 = torch.cat([eps1] * rep, 0)
        return ops.flux_prepare_latents(raw, (sB, sC, sP), batch=B, height=self._H, width=self._W, latent_channels=e.latent_channels,
                                        mode=L.POSTERIOR_MEAN if eps1 is None else L.POSTERIOR_SAMPLE, eps1=eps1, noise=noise,
                                        scale=scale, shift=shift, a=a, b=b, want_image_latents=want_image_latents,
                                        want_noise=want_noise)


class AutoencoderKL(PretrainedMixin):
    """Drop-in for the reference ``AutoencoderKL`` decode path (inference, bf16, HIP device only)."""

    def __init__(self, **kwargs):
        unknown = set(kwargs) - set(_DEFAULTS)
        if unknown:
            raise TypeError(f"AutoencoderKL: unexpected config keys {sorted(unknown)}")
        cfg = dict(_DEFAULTS)
        cfg.update(kwargs)
        self.config = FrozenConfig(cfg)
        if self.config.act_fn != "silu":
            raise ValueError("AutoencoderKL: only act_fn='silu' is supported")
        for t in self.config.up_block_types:
            if t != "UpDecoderBlock2D":
                raise ValueError(f"{t} does not exist.")
        self.dtype = bf16
        self.device = None
        self._built = False
        self.post_quant_conv = None
        self.encoder = None
        # the reference's tiling / slicing attributes (autoencoder_kl.py __init__): plain and settable
        self.use_tiling = False
        self.use_slicing = False
        ss = self.config.sample_size
        self.tile_sample_min_size = ss[0] if isinstance(ss, (list, tuple)) else ss
        self.tile_latent_min_size = int(self.tile_sample_min_size / (2 ** (len(self.config.block_out_channels) - 1)))
        self.tile_overlap_factor = 0.25

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], device="cuda", strict: bool = False):
        """Packs the decoder half (``decoder.*``, ``post_quant_conv.*``) of a reference AutoencoderKL state_dict, and the encoder
        half (``encoder.*``, ``quant_conv.*``) when the state_dict holds it."""
        c = self.config
        w = Weights(state_dict, device)
        self.device = torch.device(device)
        groups, eps = c.norm_num_groups, 1e-6
        boc = tuple(c.block_out_channels)
        lat = c.latent_channels

        def pad_rows(t, rows):
            if t.shape[0] == rows:
                return t
            out = torch.zeros((rows,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
            out[: t.shape[0]] = t
            return out

        self.latent_pad = lat
        if c.use_post_quant_conv:
            # 1x1 conv lat -> lat; output channels padded to a multiple of 8 for the thin-input kernel
            lat_p = ((lat + 7) // 8) * 8
            pw = w.get("post_quant_conv.weight").reshape(lat, lat)
            self.pqc_w = pad_rows(pw, lat_p).contiguous()
            self.pqc_b = pad_rows(w.get("post_quant_conv.bias"), lat_p).contiguous()
            self.post_quant_conv = True
            self.latent_pad = lat_p
        ci = w.get("decoder.conv_in.weight")  # [C][lat][3][3]
        if self.latent_pad != lat:
            cip = torch.zeros((ci.shape[0], self.latent_pad, 3, 3), device=ci.device, dtype=ci.dtype)
            cip[:, :lat] = ci
            ci = cip
        self.conv_in_w = ops.pack_conv_weight(ci)
        self.conv_in_b = w.get("decoder.conv_in.bias")

        self.mid_res0 = ResnetBlock2D(w, "decoder.mid_block.resnets.0", groups, eps)
        self.mid_attn = VaeAttention(w, "decoder.mid_block.attentions.0", groups, eps) \
            if c.mid_block_add_attention else None
        self.mid_res1 = ResnetBlock2D(w, "decoder.mid_block.resnets.1", groups, eps)

        self.up = []
        n = len(boc)
        for i in range(n):
            pre = f"decoder.up_blocks.{i}"
            stage = {"resnets": [ResnetBlock2D(w, f"{pre}.resnets.{j}", groups, eps)
                                 for j in range(c.layers_per_block + 1)], "up": None}
            if i != n - 1:
                stage["up"] = Upsample2D(w, f"{pre}.upsamplers.0")
            self.up.append(stage)
        self.conv_norm_out = GroupNorm(w, "decoder.conv_norm_out", groups, eps)
        self.conv_out_w = ops.pack_conv_weight(w.get("decoder.conv_out.weight"))
        self.conv_out_b = w.get("decoder.conv_out.bias")
        self.encoder = _Encoder(w, c, groups, eps) if w.has("encoder.conv_in.weight") else None
        if strict:
            extra = [k for k in w.unused() if k.startswith(("decoder.", "post_quant_conv.", "encoder.", "quant_conv."))]
            if extra:
                raise RuntimeError(f"unexpected VAE keys: {extra[:8]}")
        self._built = True
        return self

    def to(self, *args, **kwargs):
        return check_to(self, args, kwargs)

    def eval(self):
        return self

    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """autoencoder_kl.py:146-185: ``x`` NCHW in [-1, 1] (the reference's preprocessed image; fp32 or bf16, taken at bf16 as the
        bf16 reference VAE does) -> ``AutoencoderKLOutput(latent_dist=DiagonalGaussianDistribution)``."""
        self._require_encoder()
        ops.require_hip(x, "x", dtypes=(bf16, torch.float32))
        if x.dim() != 4 or x.shape[1] != self.config.in_channels:
            raise ValueError(f"AutoencoderKL.encode: NCHW input with {self.config.in_channels} channels expected, got {tuple(x.shape)}")
        dist = self.encode_image(x.float().contiguous(), nchw=True, normalize=False)
        if not return_dict:
            return (dist,)
        return AutoencoderKLOutput(latent_dist=dist)

    def _require_encoder(self):
        if self.encoder is None:
            raise NotImplementedError("AutoencoderKL.encode: the encoder half of this VAE was not loaded (its state_dict held no "
                                      "encoder.* weights; build it with factory.build_vae(..., with_encoder=True) or load a "
                                      "checkpoint that has them)")

    def encode_image(self, img: torch.Tensor, *, nchw: bool, normalize: bool) -> DiagonalGaussianDistribution:
        """Engine extension: the caller's image -- fp32 NCHW / NHWC or uint8 NHWC (read as x / 255), ``normalize``: 2 x - 1
        (VaeImageProcessor.preprocess) -- straight into the encoder.  Sizes must be multiples of 2 ** (len(block_out_channels) - 1).
        ``use_tiling`` (``enable_tiling()``): an image larger than ``tile_sample_min_size`` either way is encoded as the reference's
        ``_tiled_encode`` does -- overlapping tiles, each normalised on its own, the moments blended at the seams; ``use_slicing``
        (``enable_slicing()``): a batch is encoded sample by sample.  Either way the distribution is over the assembled moments."""
        self._require_encoder()
        ops.require_hip(img, "image", dtypes=(torch.float32, torch.uint8))
        B = img.shape[0]
        H, W_ = (img.shape[2], img.shape[3]) if nchw else (img.shape[1], img.shape[2])
        f = 2 ** (len(self.config.block_out_channels) - 1)
        if H % f or W_ % f:
            raise ValueError(f"AutoencoderKL.encode: image size {H} x {W_} is not a multiple of {f} (the engine does not resize)")
        noise_dtype = torch.float32 if self.config.force_upcast else bf16
        S = self.tile_sample_min_size
        tiled = self.use_tiling and (W_ > S or H > S)
        sliced = self.use_slicing and B > 1
        if tiled or sliced:
            moments = self._assembled_encode(img, nchw, normalize, tiled, sliced)
            return DiagonalGaussianDistribution(self.encoder, moments, None, (B, moments.shape[2], moments.shape[3]), noise_dtype,
                                                assembled=True)
        raw, strides = self.encoder(img, nchw=nchw, normalize=normalize)
        return DiagonalGaussianDistribution(self.encoder, raw, strides, (B, H // f, W_ // f), noise_dtype)

    def _encode_tile_plan(self, H: int, W: int):
        """The reference's _tiled_encode bookkeeping for an H x W pixel image, host only: ``(E, rows, Hl, Wl)`` with ``E`` the blend
        extent in latent pixels and ``rows`` the tiles in encode order, each a dict -- pixel slice (``i``, ``j``, ``ph``, ``pw``; edge
        tiles are smaller), latent size (``h``, ``w``), the piece kept (``keep_h``, ``keep_w`` = the tile cropped to ``row_limit``) and
        where the concatenations put it (``y0``, ``x0``); ``(Hl, Wl)``, the assembled size, is the sum of the pieces."""
        tl, S, factor = self.tile_latent_min_size, self.tile_sample_min_size, self.tile_overlap_factor
        f = 2 ** (len(self.config.block_out_channels) - 1)
        overlap = int(S * (1 - factor))
        E = int(tl * factor)
        row_limit = tl - E
        if overlap < 1:
            raise ValueError(f"tile_sample_min_size = {S} with tile_overlap_factor = {factor} gives overlap_size = {overlap} < 1: the "
                             "tiles would not advance")
        if E < 0 or row_limit < 1:
            raise ValueError(f"tile_latent_min_size = {tl} with tile_overlap_factor = {factor} gives blend_extent = {E} and row_limit = "
                             f"{row_limit}: nothing of a tile would be kept")
        if overlap % f or S % f:
            raise ValueError(f"tile_sample_min_size = {S} with tile_overlap_factor = {factor} gives overlap_size = {overlap}: both must "
                             f"be multiples of {f}, the VAE's downscale factor (the engine does not floor odd tiles)")
        starts = [list(range(0, n, overlap)) for n in (H, W)]
        for name, n, st in zip(("rows", "columns"), (H, W), starts):
            for a in st[:-1]:                                    # every tile but the last is some tile's upper / left neighbour
                if min(S, n - a) // f < E:
                    raise ValueError(f"tile_latent_min_size = {tl} with tile_overlap_factor = {factor} gives blend_extent = {E}, more "
                                     f"than the {min(S, n - a) // f} latent {name} of a tile that is blended into its neighbour "
                                     f"(tile_sample_min_size = {S}, image {H} x {W})")
        rows, y0 = [], 0
        for i in starts[0]:
            ph = min(S, H - i)
            row, x0 = [], 0
            for j in starts[1]:
                pw = min(S, W - j)
                t = dict(i=i, j=j, ph=ph, pw=pw, h=ph // f, w=pw // f, keep_h=min(ph // f, row_limit), keep_w=min(pw // f, row_limit),
                         y0=y0, x0=x0)
                row.append(t)
                x0 += t["keep_w"]
            rows.append(row)
            y0 += row[0]["keep_h"]
        return E, rows, y0, x0

    def _assembled_encode(self, img: torch.Tensor, nchw: bool, normalize: bool, tiled: bool, sliced: bool) -> torch.Tensor:
        """autoencoder_kl.py _tiled_encode (``tiled``) and encode's per-sample loop (``sliced``): the moments [B][2L][Hl][Wl], NCHW
        bf16, quant_conv applied.  Tiles are encoded and blended in the reference's order, one ops.vae_moments_tile_blend launch per
        tile in place of its quant_conv, blend loops, crops and concatenations; of the blended tiles only the previous row and the
        current one stay alive.  Untiled slices are one tile with no neighbour: quant_conv and place."""
        B = img.shape[0]
        H, W_ = (img.shape[2], img.shape[3]) if nchw else (img.shape[1], img.shape[2])
        f = 2 ** (len(self.config.block_out_channels) - 1)
        if tiled:
            E, rows, Hl, Wl = self._encode_tile_plan(H, W_)
        else:
            E, Hl, Wl = 0, H // f, W_ // f
            rows = [[dict(i=0, j=0, ph=H, pw=W_, h=Hl, w=Wl, keep_h=Hl, keep_w=Wl, y0=0, x0=0)]]
        enc = self.encoder
        moments = torch.empty((B, 2 * enc.latent_channels, Hl, Wl), device=img.device, dtype=bf16)
        for b0, b1 in ([(b, b + 1) for b in range(B)] if sliced else [(0, B)]):
            above = None
            for r, row in enumerate(rows):
                done = []
                for c, t in enumerate(row):
                    ys, xs = slice(t["i"], t["i"] + t["ph"]), slice(t["j"], t["j"] + t["pw"])
                    tile = (img[b0:b1, :, ys, xs] if nchw else img[b0:b1, ys, xs, :]).contiguous()
                    raw, strides = enc(tile, nchw=nchw, normalize=normalize)
                    fin = ops.vae_moments_tile_blend(raw, strides, batch=b1 - b0, latent_channels=enc.latent_channels, height=t["h"],
                                                     width=t["w"], moments=moments[b0:b1], y0=t["y0"], x0=t["x0"],
                                                     keep_h=t["keep_h"], keep_w=t["keep_w"], wq=enc.quant_w, bq=enc.quant_b, extent=E,
                                                     up=above[c] if above is not None else None, left=done[-1] if done else None,
                                                     want_fin=r + 1 < len(rows) or c + 1 < len(row))
                    done.append(fin)
                above = done
        return moments

    # ---- tiling / slicing (autoencoder_kl.py enable_tiling / enable_slicing / tiled_decode) ----
    def enable_tiling(self, use_tiling: bool = True):
        self.use_tiling = use_tiling

    def disable_tiling(self):
        self.enable_tiling(False)

    def enable_slicing(self):
        self.use_slicing = True

    def disable_slicing(self):
        self.use_slicing = False

    def _tile_plan(self, H: int, W: int):
        """The reference's tiled_decode bookkeeping for an H x W latent grid, host only: ``(E, rows, image_h, image_w)`` with ``E`` the
        blend extent and ``rows`` the tiles in decode order, each a dict -- latent slice (``i``, ``j``, ``lh``, ``lw``; edge tiles are
        smaller), decoded size (``h``, ``w``), the piece kept (``keep_h``, ``keep_w`` = the tile cropped to ``row_limit``) and where the
        concatenations put it (``y0``, ``x0``: the running sums of the pieces before it; the image size is the sum of the pieces)."""
        tl, S, factor = self.tile_latent_min_size, self.tile_sample_min_size, self.tile_overlap_factor
        up = 2 ** (len(self.config.block_out_channels) - 1)
        overlap = int(tl * (1 - factor))
        E = int(S * factor)
        row_limit = S - E
        if overlap < 1:
            raise ValueError(f"tile_latent_min_size = {tl} with tile_overlap_factor = {factor} gives overlap_size = {overlap} < 1: the "
                             "tiles would not advance")
        if E < 0 or row_limit < 1:
            raise ValueError(f"tile_sample_min_size = {S} with tile_overlap_factor = {factor} gives blend_extent = {E} and row_limit = "
                             f"{row_limit}: nothing of a tile would be kept")
        starts = [list(range(0, n, overlap)) for n in (H, W)]
        for name, n, st in zip(("rows", "columns"), (H, W), starts):
            for a in st[:-1]:                                    # every tile but the last is some tile's upper / left neighbour
                if min(tl, n - a) * up < E:
                    raise ValueError(f"tile_sample_min_size = {S} with tile_overlap_factor = {factor} gives blend_extent = {E}, more "
                                     f"than the {min(tl, n - a) * up} {name} of a tile that is blended into its neighbour "
                                     f"(tile_latent_min_size = {tl}, latent grid {H} x {W})")
        rows, y0 = [], 0
        for i in starts[0]:
            lh = min(tl, H - i)
            row, x0 = [], 0
            for j in starts[1]:
                lw = min(tl, W - j)
                t = dict(i=i, j=j, lh=lh, lw=lw, h=lh * up, w=lw * up, keep_h=min(lh * up, row_limit), keep_w=min(lw * up, row_limit),
                         y0=y0, x0=x0)
                row.append(t)
                x0 += t["keep_w"]
            rows.append(row)
            y0 += row[0]["keep_h"]
        return E, rows, y0, x0

    def _trunk(self, z: torch.Tensor, latents_div: float, latents_add: float) -> torch.Tensor:
        """post_quant_conv ... conv_norm_out + SiLU on contiguous NCHW latents: the NHWC input of conv_out."""
        if self.post_quant_conv:
            x = ops.conv_thin_in(z, self.pqc_w, self.pqc_b, ksize=1, in_nchw=True, in_div=latents_div, in_add=latents_add)
            x = ops.conv_thin_in(x, self.conv_in_w, self.conv_in_b, ksize=3, in_nchw=False)
        else:
            x = ops.conv_thin_in(z, self.conv_in_w, self.conv_in_b, ksize=3, in_nchw=True, in_div=latents_div,
                                 in_add=latents_add)
        x = self.mid_res0(x)
        if self.mid_attn is not None:
            x = self.mid_attn(x)
        x = self.mid_res1(x)
        for st in self.up:
            for rn in st["resnets"]:
                x = rn(x)
            if st["up"] is not None:
                x = st["up"](x)
        return self.conv_norm_out(x, silu=True)

    def _decode(self, z: torch.Tensor, latents_div: float, latents_add: float, postprocess: Optional[str]) -> torch.Tensor:
        return ops.conv_thin_out(self._trunk(z, latents_div, latents_add), self.conv_out_w, self.conv_out_b, postprocess=postprocess)

    def _decode_tile(self, z: torch.Tensor, latents_div: float, latents_add: float):
        """One tile up to conv_out, its result left where the conv wrote it: ``(raw, (sB, sC, sP))``."""
        return ops.conv_thin_out_tile(self._trunk(z, latents_div, latents_add), self.conv_out_w, self.conv_out_b)

    def _image_like(self, B: int, H: int, W: int, postprocess: Optional[str], device) -> torch.Tensor:
        """The empty result of a decode: what ops.conv_thin_out returns for ``postprocess``."""
        C = self.config.out_channels
        if postprocess in ("np", "uint8"):
            return torch.empty((B, H, W, C), device=device, dtype=torch.uint8 if postprocess == "uint8" else torch.float32)
        if postprocess not in (None, "pt"):
            raise ValueError(f"AutoencoderKL.decode: postprocess={postprocess!r} (use 'pt', 'np' or 'uint8')")
        return torch.empty((B, C, H, W), device=device, dtype=bf16 if postprocess is None else torch.float32)

    def _tiled_decode(self, z: torch.Tensor, latents_div: float, latents_add: float, postprocess: Optional[str],
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """autoencoder_kl.py tiled_decode: tiles decoded and blended in the reference's order, one ops.vae_tile_blend launch per tile
        in place of its blend loops, crops, concatenations and the image processor.  Of the blended tiles only the previous row and
        the current one stay alive."""
        B, C = z.shape[0], self.config.out_channels
        if C > 4:
            raise NotImplementedError(f"AutoencoderKL: tiled decode of {C} image channels (the tile-blend kernel takes at most 4)")
        E, rows, IH, IW = self._tile_plan(z.shape[2], z.shape[3])
        if out is None:
            out = self._image_like(B, IH, IW, postprocess, z.device)
        above = None
        for r, row in enumerate(rows):
            done = []
            for c, t in enumerate(row):
                tile = z[:, :, t["i"]:t["i"] + t["lh"], t["j"]:t["j"] + t["lw"]].contiguous()
                raw, strides = self._decode_tile(tile, latents_div, latents_add)
                fin = ops.vae_tile_blend(raw, strides, batch=B, channels=C, height=t["h"], width=t["w"], image=out, y0=t["y0"],
                                         x0=t["x0"], keep_h=t["keep_h"], keep_w=t["keep_w"], postprocess=postprocess, extent=E,
                                         up=above[c] if above is not None else None, left=done[-1] if done else None,
                                         want_fin=r + 1 < len(rows) or c + 1 < len(row))
                done.append(fin)
            above = done
        return out

    def decode(self, z: torch.Tensor, return_dict: bool = True, generator=None, *, latents_div: float = 1.0,
               latents_add: float = 0.0, postprocess: Optional[str] = None):
        """autoencoder_kl.py:214-240.  ``latents_div`` / ``latents_add`` fuse the pipeline's
        ``latents / scaling_factor (+ shift_factor)`` (pipeline_stable_diffusion_xl.py:1283, pipeline_flux.py:960) into
        the first conv's input read.  ``postprocess`` ("pt" / "np" / "uint8") fuses the pipeline's
        ``image_processor.postprocess`` (image_processor.py:738-786) into the last pass of ``conv_out``: the sample is then the
        finished image ([0, 1] fp32 NCHW / NHWC, or NHWC bytes) instead of the bf16 decoder output in [-1, 1].
        ``use_tiling`` (``enable_tiling()``): a latent grid larger than ``tile_latent_min_size`` either way is decoded as the
        reference's ``tiled_decode`` does -- overlapping tiles, each normalised on its own, seams blended -- and ``postprocess`` is
        applied as each tile is placed.  ``use_slicing`` (``enable_slicing()``): a batch is decoded sample by sample."""
        if not self._built:
            raise RuntimeError("AutoencoderKL: call load_state_dict() first")
        ops.require_hip(z, "z")
        z = z.contiguous()
        tl = self.tile_latent_min_size
        tiled = self.use_tiling and (z.shape[-1] > tl or z.shape[-2] > tl)
        if self.use_slicing and z.shape[0] > 1:
            img = None
            for b in range(z.shape[0]):
                if tiled:
                    if img is None:
                        _, _, IH, IW = self._tile_plan(z.shape[2], z.shape[3])
                        img = self._image_like(z.shape[0], IH, IW, postprocess, z.device)
                    self._tiled_decode(z[b:b + 1], latents_div, latents_add, postprocess, out=img[b:b + 1])
                else:
                    # (conv_out's layout pass allocates its own result, so an untiled slice costs one extra copy of the image; the
                    # tiled path above writes the output in place)
                    one = self._decode(z[b:b + 1], latents_div, latents_add, postprocess)
                    if img is None:
                        img = torch.empty((z.shape[0],) + tuple(one.shape[1:]), device=one.device, dtype=one.dtype)
                    img[b:b + 1].copy_(one)
        elif tiled:
            img = self._tiled_decode(z, latents_div, latents_add, postprocess)
        else:
            img = self._decode(z, latents_div, latents_add, postprocess)
        if not return_dict:
            return (img,)
        return DecoderOutput(sample=img)
