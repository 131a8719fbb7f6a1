"""Build engine models / pipelines from canonical configs with seeded random weights (no checkpoints exist offline)."""
from __future__ import annotations

from typing import Optional

from . import init as dinit
from .autoencoder_kl import AutoencoderKL
from .autoencoder_kl_wan import AutoencoderKLWan
from .autoencoder_tiny import AutoencoderTiny
from .controlnet import ControlNetModel
from .pipelines import (DDPMPipeline, FluxImg2ImgPipeline, FluxInpaintPipeline, FluxPipeline, StableDiffusionControlNetPipeline,
                        StableDiffusionImg2ImgPipeline, StableDiffusionInpaintPipeline, StableDiffusionInstructPix2PixPipeline,
                        StableDiffusionPipeline, StableDiffusionXLInstructPix2PixPipeline,
                        StableDiffusionXLControlNetPipeline, StableDiffusionXLImg2ImgPipeline, StableDiffusionXLInpaintPipeline,
                        StableDiffusionXLPipeline, WanPipeline)
from .schedulers import DDPMScheduler
from .unet_2d import UNet2DModel
from .transformer_wan import WanTransformer3DModel
from .schedulers import (DDIMScheduler, EulerDiscreteScheduler, FlowMatchEulerDiscreteScheduler, HeunDiscreteScheduler,
                         KDPM2DiscreteScheduler, LCMScheduler)
from .transformer_flux import FluxTransformer2DModel
from .unet_2d_condition import UNet2DConditionModel

SDXL_SCHEDULER = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                      timestep_spacing="leading")
SD15_SCHEDULER = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                      set_alpha_to_one=False, steps_offset=1)
# DPM-Solver++ 2M with Karras sigmas ("DPM++ 2M Karras") on the same betas: DPMSolverMultistepScheduler(**SDXL_DPM_SCHEDULER)
SDXL_DPM_SCHEDULER = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                          timestep_spacing="leading", use_karras_sigmas=True)
SD15_DPM_SCHEDULER = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                          timestep_spacing="leading", use_karras_sigmas=True)
# Euler ancestral ("Euler a") on the same betas: EulerAncestralDiscreteScheduler(**SDXL_EULER_A_SCHEDULER); few-step
# Turbo-style checkpoints add timestep_spacing="trailing" and run 1-4 steps with guidance_scale=0
SDXL_EULER_A_SCHEDULER = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                              timestep_spacing="leading")
SD15_EULER_A_SCHEDULER = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                              timestep_spacing="leading")
# latent-consistency sampling (LCM-LoRA fused into the checkpoint, or a distilled LCM U-Net) on the same betas:
# LCMScheduler(**LCM_SCHEDULER), 2-8 steps
LCM_SCHEDULER = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", original_inference_steps=50,
                     timestep_scaling=10.0)


# the second-order single-step samplers ("Heun", "DPM2") on the same betas: HeunDiscreteScheduler(**SECOND_ORDER_SCHEDULER),
# KDPM2DiscreteScheduler(**SECOND_ORDER_SCHEDULER); n steps are 2n - 1 model calls
SECOND_ORDER_SCHEDULER = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                              timestep_spacing="leading")


def _scheduler_for(scheduler: Optional[str], default):
    """``scheduler=None``: the pipeline's usual one (``default()``); ``"lcm"``: LCMScheduler; ``"heun"`` / ``"kdpm2"``:
    HeunDiscreteScheduler / KDPM2DiscreteScheduler."""
    if scheduler is None:
        return default()
    if scheduler == "lcm":
        return LCMScheduler(**LCM_SCHEDULER)
    if scheduler == "heun":
        return HeunDiscreteScheduler(**SECOND_ORDER_SCHEDULER)
    if scheduler == "kdpm2":
        return KDPM2DiscreteScheduler(**SECOND_ORDER_SCHEDULER)
    raise ValueError("scheduler must be None (the pipeline's default), 'lcm', 'heun' or 'kdpm2'")


def build_unet(cfg: dict, seed: int = 0, device="cuda", init_device: Optional[str] = None, state_dict=None):
    unet = UNet2DConditionModel(**cfg)
    if state_dict is None:
        shapes = dinit.unet_param_shapes(unet.config)
        state_dict = dinit.random_state_dict(shapes, seed=seed, device=init_device or "cpu")
    unet.load_state_dict(state_dict, device=device)
    return unet, state_dict


def build_controlnet(unet_config: dict, seed: int = 3, device="cuda", init_device: Optional[str] = None, state_dict=None,
                     zero_convs: bool = False, **config_overrides):
    """The ControlNet that goes with ``unet_config`` (``ControlNetModel.from_unet``: the U-Net's encoder-side options; pass e.g.
    ``conditioning_embedding_out_channels=`` to change the rest) with seeded random weights.  A trained-from-scratch ControlNet
    starts with its zero convs (``controlnet_down_blocks.*``, ``controlnet_mid_block``, the embedding's ``conv_out``) at zero and
    changes nothing; here they are random like every other weight, so that the model has an effect, unless ``zero_convs``."""
    cn = ControlNetModel(**dinit.controlnet_config(dict(unet_config), **config_overrides))
    if state_dict is None:
        state_dict = dinit.random_state_dict(dinit.controlnet_param_shapes(cn.config), seed=seed, device=init_device or "cpu")
        if zero_convs:
            for k, v in state_dict.items():
                if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.", "controlnet_cond_embedding.conv_out.")):
                    v.zero_()
    cn.load_state_dict(state_dict, device=device)
    return cn, state_dict


def build_vae(cfg: dict, seed: int = 1, device="cuda", init_device: Optional[str] = None, state_dict=None,
              with_encoder: bool = False):
    """``with_encoder``: the encoder half (+ quant_conv) as well, for ``encode`` (random_state_dict seeds per key: the decoder
    weights are the same either way)."""
    vae = AutoencoderKL(**cfg)
    if state_dict is None:
        shapes = dinit.vae_decoder_param_shapes(vae.config)
        if with_encoder:
            shapes.update(dinit.vae_encoder_param_shapes(vae.config))
        state_dict = dinit.random_state_dict(shapes, seed=seed, device=init_device or "cpu")
    vae.load_state_dict(state_dict, device=device)
    return vae, state_dict


def build_tiny_vae(cfg: dict, seed: int = 1, device="cuda", init_device: Optional[str] = None, state_dict=None,
                   with_encoder: bool = True):
    """AutoencoderTiny (``init.TAESD`` / ``TAESDXL`` / ``TAEF1`` or a sibling) with seeded random weights; ``with_encoder=False``
    packs the decoder half only (random_state_dict seeds per key: the decoder weights are the same either way)."""
    vae = AutoencoderTiny(**cfg)
    if state_dict is None:
        shapes = dinit.tiny_vae_param_shapes(vae.config, halves=("encoder", "decoder") if with_encoder else ("decoder",))
        state_dict = dinit.random_state_dict(shapes, seed=seed, device=init_device or "cpu")
    vae.load_state_dict(state_dict, device=device)
    return vae, state_dict


def _vae_for(tiny_vae: bool, tiny: bool, full_cfg: dict, tiny_cfg: dict, kl_cfg: dict, seed: int, device, idev, with_encoder: bool):
    """The pipeline's ``vae``: AutoencoderKL, or -- ``tiny_vae`` -- AutoencoderTiny (text-to-image only)."""
    if not tiny_vae:
        return build_vae(kl_cfg, seed=seed, device=device, init_device=idev, with_encoder=with_encoder)[0]
    if with_encoder:
        raise ValueError("tiny_vae=True builds a text-to-image pipeline: AutoencoderTiny has no posterior for img2img / inpainting")
    return build_tiny_vae(tiny_cfg if tiny else full_cfg, seed=seed, device=device, init_device=idev, with_encoder=False)[0]


def build_wan_vae(cfg: dict, seed: int = 21, device="cuda", init_device: Optional[str] = None, state_dict=None):
    vae = AutoencoderKLWan(**cfg)
    if state_dict is None:
        shapes = dinit.wan_vae_decoder_param_shapes(vae.config)
        state_dict = dinit.random_state_dict(shapes, seed=seed, device=init_device or "cpu")
    vae.load_state_dict(state_dict, device=device)
    return vae, state_dict


def _inpaint_unet_config(ucfg: dict, unet_in_channels: int) -> dict:
    if unet_in_channels not in (4, 9):
        raise ValueError("unet_in_channels: 4 (any checkpoint, mask blend after every step) or 9 (an inpainting U-Net)")
    return ucfg if unet_in_channels == ucfg.get("in_channels", 4) else dict(ucfg, in_channels=unet_in_channels)


def _pix2pix_unet_config(ucfg: dict, img2img: bool, inpaint: bool, controlnet, tiny_vae: bool) -> dict:
    """``pix2pix=True``: the 8-channel U-Net of an InstructPix2Pix checkpoint (latents | image latents); a pipeline of its own."""
    if img2img or inpaint or controlnet or tiny_vae:
        raise ValueError("pix2pix=True builds the InstructPix2Pix pipeline: not together with img2img / inpaint / controlnet / tiny_vae")
    return dict(ucfg, in_channels=8)


def _controlnet_for(ucfg: dict, tiny: bool, seed: int, device, idev, controlnet):
    """``controlnet=True``: a seeded ControlNet for the U-Net config; a ControlNetModel is taken as it is."""
    if controlnet is not True:
        return controlnet
    over = {"conditioning_embedding_out_channels": dinit.TINY_SDXL_CONTROLNET["conditioning_embedding_out_channels"]} if tiny else {}
    return build_controlnet(ucfg, seed=seed + 3, device=device, init_device=idev, **over)[0]


def build_sdxl_pipeline(device="cuda", tiny: bool = False, seed: int = 0, init_device: Optional[str] = None,
                        with_encoder: bool = False, img2img: bool = False, inpaint: bool = False, unet_in_channels: int = 4,
                        controlnet=False, scheduler: Optional[str] = None, time_cond_proj_dim: Optional[int] = None,
                        tiny_vae: bool = False, pix2pix: bool = False):
    """SDXL-base (BASELINE config 3) or its tiny sibling.  Full size: weights are generated on ``init_device``
    (default: the HIP device, ~2.6 B parameters in seconds) and freed after packing.  ``with_encoder``: the VAE's encoder as
    well; ``img2img``: the same components in a StableDiffusionXLImg2ImgPipeline, ``inpaint``: in a
    StableDiffusionXLInpaintPipeline (both imply ``with_encoder``), whose U-Net takes ``unet_in_channels`` = 4 or 9 input channels.
    ``controlnet``: True (a seeded ControlNet, seed + 3) or a ControlNetModel -- a StableDiffusionXLControlNetPipeline (text-to-image).
    ``scheduler="lcm"``: LCMScheduler instead of Euler; ``time_cond_proj_dim``: a U-Net with the guidance-scale embedding input of the
    distilled LCM checkpoints (``time_embedding.cond_proj``).  ``tiny_vae``: AutoencoderTiny (TAESDXL, or its two-stage sibling with
    ``tiny``) in the ``vae`` slot instead of AutoencoderKL -- text-to-image and ControlNet only.  ``pix2pix``: an 8-channel U-Net and the
    VAE with its encoder in a StableDiffusionXLInstructPix2PixPipeline (exclusive with img2img / inpaint / controlnet / tiny_vae)."""
    ucfg = dinit.TINY_SDXL_UNET if tiny else dinit.SDXL_UNET
    if time_cond_proj_dim is not None:
        ucfg = dict(ucfg, time_cond_proj_dim=int(time_cond_proj_dim))
    if inpaint:
        ucfg = _inpaint_unet_config(ucfg, unet_in_channels)
    if pix2pix:
        ucfg = _pix2pix_unet_config(ucfg, img2img, inpaint, controlnet, tiny_vae)
    vcfg = dinit.TINY_VAE if tiny else dinit.SDXL_VAE
    idev = init_device or ("cpu" if tiny else str(device))
    unet, _ = build_unet(ucfg, seed=seed, device=device, init_device=idev)
    vae = _vae_for(tiny_vae, tiny, dinit.TAESDXL, dinit.TINY_TAESD, vcfg, seed + 1, device, idev, with_encoder or img2img or inpaint or pix2pix)
    sch = _scheduler_for(scheduler, lambda: EulerDiscreteScheduler(**SDXL_SCHEDULER))
    if controlnet:
        if img2img or inpaint:
            raise ValueError("controlnet= builds the text-to-image ControlNet pipeline (no ControlNet img2img / inpainting pipeline)")
        return StableDiffusionXLControlNetPipeline(vae=vae, unet=unet, scheduler=sch,
                                                   controlnet=_controlnet_for(ucfg, tiny, seed, device, idev, controlnet))
    if pix2pix:
        return StableDiffusionXLInstructPix2PixPipeline(vae=vae, unet=unet, scheduler=sch)
    cls = StableDiffusionXLInpaintPipeline if inpaint else StableDiffusionXLImg2ImgPipeline if img2img else StableDiffusionXLPipeline
    return cls(vae=vae, unet=unet, scheduler=sch)


def build_sd15_pipeline(device="cuda", tiny: bool = False, seed: int = 0, init_device: Optional[str] = None,
                        with_encoder: bool = False, img2img: bool = False, inpaint: bool = False, unet_in_channels: int = 4,
                        controlnet=False, scheduler: Optional[str] = None, time_cond_proj_dim: Optional[int] = None,
                        tiny_vae: bool = False, pix2pix: bool = False):
    """SD1.5 or its tiny sibling, as ``build_sdxl_pipeline`` (DDIM by default; ``tiny_vae``: TAESD; ``pix2pix``: a
    StableDiffusionInstructPix2PixPipeline)."""
    ucfg = dinit.TINY_SD15_UNET if tiny else dinit.SD15_UNET
    if time_cond_proj_dim is not None:
        ucfg = dict(ucfg, time_cond_proj_dim=int(time_cond_proj_dim))
    if inpaint:
        ucfg = _inpaint_unet_config(ucfg, unet_in_channels)
    if pix2pix:
        ucfg = _pix2pix_unet_config(ucfg, img2img, inpaint, controlnet, tiny_vae)
    vcfg = dinit.TINY_VAE if tiny else dinit.SD_VAE
    idev = init_device or ("cpu" if tiny else str(device))
    unet, _ = build_unet(ucfg, seed=seed, device=device, init_device=idev)
    vae = _vae_for(tiny_vae, tiny, dinit.TAESD, dinit.TINY_TAESD, vcfg, seed + 1, device, idev, with_encoder or img2img or inpaint or pix2pix)
    sch = _scheduler_for(scheduler, lambda: DDIMScheduler(**SD15_SCHEDULER))
    if controlnet:
        if img2img or inpaint:
            raise ValueError("controlnet= builds the text-to-image ControlNet pipeline (no ControlNet img2img / inpainting pipeline)")
        return StableDiffusionControlNetPipeline(vae=vae, unet=unet, scheduler=sch,
                                                 controlnet=_controlnet_for(ucfg, tiny, seed, device, idev, controlnet))
    if pix2pix:
        return StableDiffusionInstructPix2PixPipeline(vae=vae, unet=unet, scheduler=sch)
    cls = StableDiffusionInpaintPipeline if inpaint else StableDiffusionImg2ImgPipeline if img2img else StableDiffusionPipeline
    return cls(vae=vae, unet=unet, scheduler=sch)


def build_flux_transformer(cfg: dict, seed: int = 5, device="cuda", init_device: Optional[str] = None, state_dict=None):
    tr = FluxTransformer2DModel(**cfg)
    if state_dict is None:
        state_dict = dinit.random_state_dict(dinit.flux_param_shapes(tr.config), seed=seed, device=init_device or "cpu")
    tr.load_state_dict(state_dict, device=device)
    return tr, state_dict


def build_flux_pipeline(device="cuda", tiny: bool = False, seed: int = 5, init_device: Optional[str] = None,
                        with_encoder: bool = False, img2img: bool = False, inpaint: bool = False, tiny_vae: bool = False):
    """FLUX.1-schnell (BASELINE config 4) or its tiny sibling: transformer + 16-channel VAE + FlowMatch-Euler (shift 1).
    ``with_encoder``: the VAE's encoder as well; ``img2img``: the same components in a FluxImg2ImgPipeline, ``inpaint``: in a
    FluxInpaintPipeline (both imply ``with_encoder``).  ``tiny_vae``: AutoencoderTiny (TAEF1) as the ``vae`` (text-to-image only)."""
    tcfg = dinit.TINY_FLUX if tiny else dinit.FLUX_SCHNELL
    vcfg = dinit.TINY_FLUX_VAE if tiny else dinit.FLUX_VAE
    idev = init_device or ("cpu" if tiny else str(device))
    tr, _ = build_flux_transformer(tcfg, seed=seed, device=device, init_device=idev)
    vae = _vae_for(tiny_vae, tiny, dinit.TAEF1, dinit.TINY_TAEF1, vcfg, seed + 1, device, idev, with_encoder or img2img or inpaint)
    sch = FlowMatchEulerDiscreteScheduler(shift=1.0, use_dynamic_shifting=False)
    cls = FluxInpaintPipeline if inpaint else FluxImg2ImgPipeline if img2img else FluxPipeline
    return cls(scheduler=sch, vae=vae, transformer=tr)


def build_wan_transformer(cfg: dict, seed: int = 9, device="cuda", init_device: Optional[str] = None, state_dict=None):
    tr = WanTransformer3DModel(**cfg)
    if state_dict is None:
        state_dict = dinit.random_state_dict(dinit.wan_param_shapes(tr.config), seed=seed, device=init_device or "cpu")
    tr.load_state_dict(state_dict, device=device)
    return tr, state_dict


def build_wan_pipeline(device="cuda", tiny: bool = False, seed: int = 9, init_device: Optional[str] = None,
                       flow_shift: float = 3.0, with_vae: bool = False, scheduler: str = "flowmatch"):
    """Wan2.1-T2V-1.3B (BASELINE config 5) or its tiny sibling.  ``scheduler="unipc"``: the sampler the checkpoint ships
    (pipeline_wan.py:52-59: UniPCMultistepScheduler, flow_prediction, use_flow_sigmas, flow_shift 3.0 for 480p), else the
    FlowMatch-Euler scheduler of SURVEY.md 8d; ``with_vae`` adds AutoencoderKLWan (seed + 12) so that
    ``output_type="raw" / "pt"`` decodes the video."""
    cfg = dinit.TINY_WAN if tiny else dinit.WAN_1_3B
    idev = init_device or ("cpu" if tiny else str(device))
    tr, _ = build_wan_transformer(cfg, seed=seed, device=device, init_device=idev)
    if scheduler == "unipc":
        from .schedulers import UniPCMultistepScheduler
        sch = UniPCMultistepScheduler(prediction_type="flow_prediction", use_flow_sigmas=True, flow_shift=flow_shift)
    elif scheduler == "flowmatch":
        sch = FlowMatchEulerDiscreteScheduler(shift=flow_shift, use_dynamic_shifting=False)
    else:
        raise ValueError("scheduler must be 'unipc' or 'flowmatch'")
    vae = None
    if with_vae:
        vae, _ = build_wan_vae(dinit.TINY_WAN_VAE if tiny else dinit.WAN_VAE, seed=seed + 12, device=device, init_device=idev)
    return WanPipeline(scheduler=sch, transformer=tr, vae=vae)


def build_unet2d(cfg: dict, seed: int = 0, device="cuda", init_device: Optional[str] = None, state_dict=None):
    unet = UNet2DModel(**cfg)
    if state_dict is None:
        full = dict(unet.config)
        state_dict = dinit.random_state_dict(dinit.unet2d_param_shapes(full), seed=seed, device=init_device or "cpu")
    unet.load_state_dict(state_dict, device=device)
    return unet, state_dict


def build_ddpm_pipeline(device="cuda", tiny: bool = False, seed: int = 0, init_device: Optional[str] = None):
    """google/ddpm-cat-256 (BASELINE config 1) or its tiny sibling."""
    cfg = dinit.TINY_DDPM if tiny else dinit.DDPM_CAT
    unet, _ = build_unet2d(cfg, seed=seed, device=device, init_device=init_device or ("cpu" if tiny else str(device)))
    return DDPMPipeline(unet=unet, scheduler=DDPMScheduler(**dinit.DDPM_SCHEDULER))
