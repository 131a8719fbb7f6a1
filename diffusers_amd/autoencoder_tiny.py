"""AutoencoderTiny (TAESD / TAESDXL / TAEF1) on the gfx950 kernels.

Mirrors models/autoencoders/autoencoder_tiny.py (AutoencoderTiny) with vae.py's EncoderTiny, DecoderTiny and AutoencoderTinyBlock:
a 64-channel, ReLU-only codec whose trunk is one conv shape -- 3x3, 64 -> 64, stride 1, bias (+ residual) + ReLU -- which runs on
its own kernel (csrc/conv_c64.hip, ``ops.conv2d_nhwc(act=ACT_RELU)``).  The stride-2 and nearest-2x convs, the image -> first conv
of the encoder and the 64 -> 3 / 64 -> latent convs at the two ends are the kernels AutoencoderKL already uses.

Layout of a decode (latents NCHW bf16 in, image NCHW bf16 or the postprocessed image out):
  1. ops.tiny_vae_latents_in      latents / scaling_factor (+ shift_factor), tanh(x / 3) * 3, NCHW -> NHWC padded to 64 channels
  2. conv_in + ReLU               one ReLU-conv launch, k_valid = latent_channels (weights zero-padded to 64 input channels)
  3. every AutoencoderTinyBlock   three ReLU-conv launches, the third with residual = the block's input: relu(conv(x) + x)
  4. Upsample + its conv          one conv2d_nhwc(up=True) launch
  5. the last conv and `* 2 - 1`  ops.conv_thin_out with the affine map folded into the packed weights: w' = 2 w (exact in bf16),
                                  b' = bf16(2 b - 1); `postprocess` rides on it as in AutoencoderKL.decode
Rounding differences from the reference's op-by-op bf16: the residual joins the fp32 accumulator (one rounding where
the reference rounds conv and add separately), and step 5 rounds once where the reference rounds conv, * 2 and - 1.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib as L
from . import init as dinit
from . import ops
from .autoencoder_kl import DecoderOutput
from .config_utils import check_to, from_reference_config
from .layers import Weights
from .loading import PretrainedMixin
from .unet_2d_condition import FrozenConfig

bf16 = torch.bfloat16
WIDTH = 64          # the one channel count csrc/conv_c64.hip is built for

_DEFAULTS = dict(
    in_channels=3, out_channels=3, encoder_block_out_channels=(64, 64, 64, 64), decoder_block_out_channels=(64, 64, 64, 64),
    act_fn="relu", upsample_fn="nearest", latent_channels=4, upsampling_scaling_factor=2, num_encoder_blocks=(1, 3, 3, 3),
    num_decoder_blocks=(3, 3, 3, 1), latent_magnitude=3, latent_shift=0.5, force_upcast=False, scaling_factor=1.0, shift_factor=0.0,
)


@dataclass
class AutoencoderTinyOutput:
    latents: torch.Tensor


class _ReluConv:
    """Conv3x3(64 -> 64) + ReLU on the 64-channel kernel; ``k_valid``: real input channels of a zero-padded first conv."""

    def __init__(self, w: Weights, prefix: str, cin: int = WIDTH):
        wt = w.get(prefix + ".weight")                      # [64][cin][3][3]
        if cin != WIDTH:
            wp = torch.zeros((wt.shape[0], WIDTH, 3, 3), device=wt.device, dtype=wt.dtype)
            wp[:, :cin] = wt
            wt = wp
        self.weight = ops.pack_conv_weight(wt)
        self.bias = w.opt(prefix + ".bias")
        self.k_valid = cin if cin != WIDTH else 0

    def __call__(self, x, residual=None):
        return ops.conv2d_nhwc(x, self.weight, self.bias, ksize=3, residual=residual, act=L.ACT_RELU, k_valid=self.k_valid)


class _Block:
    """AutoencoderTinyBlock (in == out channels: the skip is the identity): relu(conv(x) + x)."""

    def __init__(self, w: Weights, prefix: str):
        self.convs = [_ReluConv(w, f"{prefix}.conv.{i}") for i in (0, 2, 4)]

    def __call__(self, x):
        h = self.convs[0](x)
        h = self.convs[1](h)
        return self.convs[2](h, residual=x)


class _PlainConv:
    """A conv with no activation on the existing implicit-GEMM kernel: ``up`` (nearest 2x fused into the gather) or stride 2."""

    def __init__(self, w: Weights, prefix: str, *, up: bool = False, stride: int = 1):
        self.weight = ops.pack_conv_weight(w.get(prefix + ".weight"))
        self.bias = w.opt(prefix + ".bias")
        self.up, self.stride = bool(up), int(stride)

    def __call__(self, x):
        return ops.conv2d_nhwc(x, self.weight, self.bias, ksize=3, up=self.up, stride=self.stride)


class _Decoder:
    def __init__(self, w: Weights, c):
        plan = dinit.tiny_vae_layer_plan(c, "decoder")
        self.magnitude = float(c.latent_magnitude)
        self.steps = []
        i = 0
        while i < len(plan):
            idx, kind = plan[i][0], plan[i][1]
            p = f"decoder.layers.{idx}"
            if kind == "conv" and i + 1 < len(plan) and plan[i + 1][1] == "relu":
                self.steps.append(_ReluConv(w, p, cin=plan[i][2]))
                i += 2
            elif kind == "block":
                self.steps.append(_Block(w, p))
                i += 1
            elif kind == "up":
                self.steps.append(_PlainConv(w, f"decoder.layers.{plan[i + 1][0]}", up=True))
                i += 2
            else:                                                # the last conv: 64 -> out_channels with bias, then * 2 - 1
                if i != len(plan) - 1:
                    raise ValueError("AutoencoderTiny: unexpected decoder layout")
                wt, b = w.get(p + ".weight"), w.get(p + ".bias")
                self.out_w = ops.pack_conv_weight(wt * 2)        # exact: a power of two
                self.out_b = (b.float() * 2 - 1).to(bf16).contiguous()
                i += 1

    def __call__(self, z, latents_div, latents_add, postprocess):
        x = ops.tiny_vae_latents_in(z, in_div=latents_div, in_add=latents_add, magnitude=self.magnitude)
        for st in self.steps:
            x = st(x)
        return ops.conv_thin_out(x, self.out_w, self.out_b, postprocess=postprocess)


class _Encoder:
    def __init__(self, w: Weights, c):
        plan = dinit.tiny_vae_layer_plan(c, "encoder")
        p0 = f"encoder.layers.{plan[0][0]}"
        self.conv_in_w = ops.pack_conv_weight(w.get(p0 + ".weight"))      # [64][27]
        self.conv_in_b = w.get(p0 + ".bias")
        self.steps = []
        for e in plan[1:-1]:
            p = f"encoder.layers.{e[0]}"
            self.steps.append(_Block(w, p) if e[1] == "block" else _PlainConv(w, p, stride=2))
        pl = f"encoder.layers.{plan[-1][0]}"
        self.out_w = ops.pack_conv_weight(w.get(pl + ".weight"))
        self.out_b = w.get(pl + ".bias")

    def __call__(self, img01, nchw: bool):
        # EncoderTiny.forward feeds (x + 1) / 2 of the normalised image, i.e. the image in [0, 1]: normalize = 0
        x = ops.vae_conv_in_image(img01, self.conv_in_w, self.conv_in_b, nchw=nchw, normalize=False)
        for st in self.steps:
            x = st(x)
        return ops.conv_thin_out(x, self.out_w, self.out_b)


class AutoencoderTiny(PretrainedMixin):
    """Drop-in for the reference ``AutoencoderTiny`` (inference, bf16, HIP device only): ``decode`` / ``encode`` /
    ``scale_latents`` / ``unscale_latents``.  Goes in a pipeline's ``vae`` slot for text-to-image (the image-conditioned pipelines
    read a posterior, which this codec does not have, and refuse it)."""

    def __init__(self, **kwargs):
        boc = kwargs.pop("block_out_channels", None)      # the reference registers it (= decoder_block_out_channels); config.json has it
        unknown = set(kwargs) - set(_DEFAULTS)
        if unknown:
            raise TypeError(f"AutoencoderTiny: unexpected config keys {sorted(unknown)}")
        cfg = dict(_DEFAULTS)
        cfg.update(kwargs)
        for key in ("encoder_block_out_channels", "decoder_block_out_channels", "num_encoder_blocks", "num_decoder_blocks"):
            cfg[key] = tuple(cfg[key])
        if boc is not None and tuple(boc) != cfg["decoder_block_out_channels"]:
            raise ValueError("AutoencoderTiny: block_out_channels must equal decoder_block_out_channels")
        for key in ("encoder_block_out_channels", "decoder_block_out_channels"):
            if any(int(v) != WIDTH for v in cfg[key]):
                raise ValueError(f"AutoencoderTiny: {key}={cfg[key]} -- only {WIDTH}-channel stages are built (the conv kernel has one width)")
        if cfg["act_fn"] != "relu":
            raise ValueError(f"AutoencoderTiny: act_fn={cfg['act_fn']!r} -- only 'relu' is supported")
        if cfg["upsample_fn"] != "nearest":
            raise ValueError(f"AutoencoderTiny: upsample_fn={cfg['upsample_fn']!r} -- only 'nearest' is supported")
        if cfg["upsampling_scaling_factor"] != 2:
            raise ValueError(f"AutoencoderTiny: upsampling_scaling_factor={cfg['upsampling_scaling_factor']} -- only 2 is supported")
        if not 1 <= int(cfg["latent_channels"]) <= 16:
            raise ValueError(f"AutoencoderTiny: latent_channels={cfg['latent_channels']} -- 1 .. 16 (the latent input kernel's limit)")
        if len(cfg["encoder_block_out_channels"]) != len(cfg["num_encoder_blocks"]):
            raise ValueError("AutoencoderTiny: `encoder_block_out_channels` should have the same length as `num_encoder_blocks`.")
        if len(cfg["decoder_block_out_channels"]) != len(cfg["num_decoder_blocks"]):
            raise ValueError("AutoencoderTiny: `decoder_block_out_channels` should have the same length as `num_decoder_blocks`.")
        cfg["block_out_channels"] = cfg["decoder_block_out_channels"]      # the pipelines derive vae_scale_factor from it
        self.config = FrozenConfig(cfg)
        self.latent_magnitude, self.latent_shift = cfg["latent_magnitude"], cfg["latent_shift"]
        self.spatial_scale_factor = 2 ** (len(cfg["decoder_block_out_channels"]) - 1)
        self.dtype = bf16
        self.device = None
        self._built = False
        self.decoder = None
        self.encoder = None

    @classmethod
    def from_config(cls, config, **overrides):
        """``ConfigMixin.from_config``: the reference's config mapping (private keys dropped, lists -> tuples)."""
        return from_reference_config(cls, config, **overrides)

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], device="cuda", strict: bool = False):
        """Packs a reference AutoencoderTiny state_dict: ``decoder.layers.*``, and ``encoder.layers.*`` when it is there."""
        c = self.config
        w = Weights(state_dict, device)
        self.device = torch.device(device)
        self.decoder = _Decoder(w, c)
        self.encoder = _Encoder(w, c) if w.has("encoder.layers.0.weight") else None
        if strict:
            extra = [k for k in w.unused() if k.startswith(("decoder.", "encoder."))]
            if extra:
                raise RuntimeError(f"unexpected AutoencoderTiny keys: {extra[:8]}")
        self._built = True
        self._new_weights_generation()
        return self

    def to(self, *args, **kwargs):
        return check_to(self, args, kwargs)

    def eval(self):
        return self

    def scale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """raw latents -> [0, 1] (autoencoder_tiny.py scale_latents)."""
        return x.div(2 * self.latent_magnitude).add(self.latent_shift).clamp(0, 1)

    def unscale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """[0, 1] -> raw latents (autoencoder_tiny.py unscale_latents)."""
        return x.sub(self.latent_shift).mul(2 * self.latent_magnitude)

    def _require(self, half: str):
        if not self._built:
            raise RuntimeError("AutoencoderTiny: call load_state_dict() first")
        if half == "encoder" and self.encoder is None:
            raise NotImplementedError("AutoencoderTiny.encode: the encoder half was not loaded (the state_dict held no "
                                      "encoder.layers.* weights)")

    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """autoencoder_tiny.py encode: ``x`` NCHW in [-1, 1] (fp32 or bf16) -> ``AutoencoderTinyOutput(latents=...)``, NCHW bf16; there
        is no posterior.  EncoderTiny starts with (x + 1) / 2: that map is applied HERE, as two torch operators on a fp32 copy of the
        caller's tensor (the image loader of the first conv takes pixels in [0, 1]); ``encode_image`` takes such pixels directly."""
        self._require("encoder")
        ops.require_hip(x, "x", dtypes=(bf16, torch.float32))
        if x.dim() != 4 or x.shape[1] != self.config.in_channels:
            raise ValueError(f"AutoencoderTiny.encode: NCHW input with {self.config.in_channels} channels expected, got {tuple(x.shape)}")
        out = self.encode_image(((x.float() + 1.0) / 2.0).contiguous(), nchw=True, normalize=True)
        return out if return_dict else (out.latents,)

    def encode_image(self, img: torch.Tensor, *, nchw: bool, normalize: bool = True) -> AutoencoderTinyOutput:
        """Engine extension, as ``AutoencoderKL.encode_image``: pixels in [0, 1] -- fp32 NCHW / NHWC, or uint8 NHWC read as x / 255 --
        straight into the encoder.  ``normalize=True`` (2 x - 1, VaeImageProcessor.preprocess) cancels against EncoderTiny's
        (x + 1) / 2, so the loader normalises nothing; ``normalize=False`` would mean an image already in [-1, 1]: use ``encode``."""
        self._require("encoder")
        ops.require_hip(img, "image", dtypes=(torch.float32, torch.uint8))
        if not normalize:
            raise ValueError("AutoencoderTiny.encode_image takes pixels in [0, 1] (normalize=True); for a [-1, 1] tensor call encode()")
        if self.config.in_channels != 3:
            raise NotImplementedError("AutoencoderTiny.encode: the image loader is built for 3-channel images")
        H, W_ = (img.shape[2], img.shape[3]) if nchw else (img.shape[1], img.shape[2])
        f = 2 ** (len(self.config.encoder_block_out_channels) - 1)
        if H % f or W_ % f:
            raise ValueError(f"AutoencoderTiny.encode: image size {H} x {W_} is not a multiple of {f} (the engine does not resize)")
        return AutoencoderTinyOutput(latents=self.encoder(img, nchw))

    def decode(self, z: torch.Tensor, return_dict: bool = True, generator=None, *, latents_div: float = 1.0,
               latents_add: float = 0.0, postprocess: Optional[str] = None):
        """autoencoder_tiny.py decode (DecoderTiny.forward): the keywords of ``AutoencoderKL.decode`` -- ``latents_div`` /
        ``latents_add`` fuse the pipeline's ``latents / scaling_factor (+ shift_factor)``, ``postprocess`` ("pt" / "np" / "uint8") the
        pipeline's ``image_processor.postprocess`` into the last pass.  Every step is a kernel launch (module docstring)."""
        self._require("decoder")
        ops.require_hip(z, "z")
        if z.dim() != 4 or z.shape[1] != self.config.latent_channels:
            raise ValueError(f"AutoencoderTiny.decode: NCHW latents with {self.config.latent_channels} channels expected, got {tuple(z.shape)}")
        img = self.decoder(z.contiguous(), float(latents_div), float(latents_add), postprocess)
        if not return_dict:
            return (img,)
        return DecoderOutput(sample=img)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("AutoencoderTiny.forward (the byte-quantised encode -> decode round trip) is not built; call "
                                  "encode() and decode()")

    __call__ = forward
