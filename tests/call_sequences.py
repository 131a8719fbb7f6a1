"""The call-sequence table of tests/test_call_sequences_gpu.py and tests/test_call_sequences_cpu.py.

Every pipeline captures its denoising step once (HIP graph, or launch plan with ``use_graph="plan"``) and replays it on later calls;
whether a later call replays or captures again is decided by the pipeline's ``_make_graph_key``.  A captured step bakes in what it
was handed by value -- the sampler kernel the scheduler's class picks, ``pred_type``, guidance, the CFG / rescale / dtype branches,
raw pointers into packed weights and scheduler state -- so a key that misses one of them lets a changed second call run the first
call's step.  This module lists, per pipeline family, one first call and the ways a second call may differ from it:

  FAMILIES[name]   how the tiny pipeline is built (diffusers_amd.factory, fixed seeds: a second build is the oracle), its base call
                   and its mutations.
  a mutation       a named function ``(pipe, kwargs) -> kwargs`` that changes exactly one thing of the pipeline or of the call and
                   declares ``expect``: "recapture" (the captured step cannot serve the new call) or "replay" (only the contents
                   of static buffers change: a capture would be wasted).  ``setup`` puts the pipeline into the state the mutation
                   starts from when that is not the factory's (the later hops of a scheduler chain), ``base`` does the same for the
                   first call's arguments, ``undo`` takes the mutation back -- for a scheduler by building a NEW one of the old
                   kind, as the mutation itself does: ``pipe.scheduler = ...`` in one statement drops the last reference to the
                   scheduler before it, its device buffers go back to the caching allocator, and the next ``set_timesteps``
                   allocates a table and a counter of exactly those sizes.

Tensors of the calls are drawn on the CPU from fixed seeds and moved to the pipeline's device, so the same table drives the GPU
tests (outputs, bit for bit against an eager oracle) and the CPU tests (keys only).
"""
from collections import namedtuple

import numpy as np
import torch

from diffusers_amd import factory, init as dinit, packed_cache
from diffusers_amd.schedulers import (DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,
                                      EulerDiscreteScheduler, FlowMatchEulerDiscreteScheduler, UniPCMultistepScheduler)

bf16 = torch.bfloat16
OTHER_SEED = 7          # the weights a model is swapped for / reloaded with


def _rand(shape, seed, dtype=bf16):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)).to(dtype)


def _gen(seed=3):
    return lambda: torch.Generator("cpu").manual_seed(seed)


def materialise(kwargs, device):
    """The arguments of one call: tensors copied (the pipelines update latents in place) onto ``device``, callables (generators:
    a fresh one per call) called.  Images and masks stay on the CPU as callers hand them in."""
    out = {}
    for k, v in kwargs.items():
        if callable(v):
            v = v()
        elif torch.is_tensor(v):
            v = v.clone() if k in ("image", "mask_image") else v.clone().to(device)
        out[k] = v
    return out


def run(pipe, kwargs, use_graph):
    """One call; the result as a tensor of its own (with ``output_type="latent"`` / "raw" the pipelines return the buffer the
    captured step writes, which the next call overwrites)."""
    out = pipe(use_graph=use_graph, **materialise(kwargs, pipe.device)).images
    return torch.from_numpy(out) if isinstance(out, np.ndarray) else out.clone()


class _KeyTaken(Exception):
    pass


def graph_key_of(pipe, kwargs):
    """The key ``pipe(**kwargs)`` would compare with its captured step's: the call runs up to ``_make_graph_key`` -- schedule,
    conditioning, noise tables, everything the key reads -- and ends there, before anything touches a stream.  Works on
    ``device="cpu"`` pipelines over the kernel stand-ins."""
    taken = []
    make = pipe._make_graph_key

    def spy(*a, **k):
        taken.append(make(*a, **k))
        raise _KeyTaken

    pipe._make_graph_key = spy
    try:
        pipe(use_graph=True, **materialise(kwargs, pipe.device))
    except _KeyTaken:
        pass
    finally:
        del pipe._make_graph_key
    return taken[0]


# ----------------------------------------------------------------------------------------------------------------------
# mutations
# ----------------------------------------------------------------------------------------------------------------------
def _nothing(pipe):
    pass


def mutation(expect, name=None, setup=_nothing, undo=_nothing, base=None):
    assert expect in ("recapture", "replay")

    def deco(fn):
        fn.expect, fn.setup, fn.undo, fn.base = expect, setup, undo, base or (lambda kw: kw)
        fn.name = name or fn.__name__
        return fn
    return deco


def _set(expect, name, **changes):
    """A mutation of the call's arguments alone."""
    @mutation(expect, name=name)
    def fn(pipe, kw):
        return dict(kw, **changes)
    return fn


# -- schedulers: every kind is built anew each time, from the factory's constants ------------------------------------------------
def _sd_schedulers(prefix):
    base = getattr(factory, f"{prefix}_SCHEDULER")
    euler_a, dpm = getattr(factory, f"{prefix}_EULER_A_SCHEDULER"), getattr(factory, f"{prefix}_DPM_SCHEDULER")
    ddim = dict(clip_sample=False, set_alpha_to_one=False)
    return {
        "euler": lambda **o: EulerDiscreteScheduler.from_config(base, **o),
        "ddim": lambda **o: DDIMScheduler.from_config(base, **dict(ddim, **o)),
        "euler_a": lambda **o: EulerAncestralDiscreteScheduler.from_config(euler_a, **o),
        "dpm": lambda **o: DPMSolverMultistepScheduler.from_config(dpm, **o),
    }


SCHEDULERS = {
    "sd15": dict(_sd_schedulers("SD15"), base="ddim"),
    "sdxl": dict(_sd_schedulers("SDXL"), base="euler"),
    "flux": {"flowmatch": lambda **o: FlowMatchEulerDiscreteScheduler(**dict(dict(shift=1.0, use_dynamic_shifting=False), **o)),
             "base": "flowmatch"},
    "wan": {"flowmatch": lambda **o: FlowMatchEulerDiscreteScheduler(**dict(dict(shift=3.0, use_dynamic_shifting=False), **o)),
            # the configuration of test_tiny_wan_pipeline_unipc_vs_oracle
            "unipc": lambda **o: UniPCMultistepScheduler(prediction_type="flow_prediction", use_flow_sigmas=True, flow_shift=3.0, **o),
            "base": "flowmatch"},
    "ddpm": {"ddpm": lambda **o: DDPMScheduler(**dict(dinit.DDPM_SCHEDULER, **o)), "base": "ddpm"},
}
CHAIN = ("euler", "ddim", "euler_a", "dpm", "euler")        # SD / SDXL, at an equal step count


def scheduler_swap(table, src, dst, src_cfg=None, dst_cfg=None, name=None):
    """``pipe.scheduler`` of kind ``src`` (a new object before the first call) replaced by a new one of kind ``dst``; undone by a
    new one of kind ``src``.  Each assignment is one statement that drops the last reference to the scheduler before it."""
    make = SCHEDULERS[table]
    src_cfg, dst_cfg = src_cfg or {}, dst_cfg or {}

    def to_src(pipe):
        pipe.scheduler = make[src](**src_cfg)

    @mutation("recapture", name=name or f"scheduler_{src}_to_{dst}", setup=to_src, undo=to_src)
    def fn(pipe, kw):
        pipe.scheduler = make[dst](**dst_cfg)
        return kw
    fn.src, fn.dst = (src, src_cfg), (dst, dst_cfg)
    return fn


def alias_scheduler_buffers(new, old):
    """Force what the caching allocator may do after ``pipe.scheduler = new`` dropped ``old``: every device buffer of ``new`` sits
    where the buffer of ``old`` of the same size sat.  ``new`` keeps its own contents.  Returns the names aliased."""
    done = []
    for name in ("_table", "_step_dev", "_begin_dev", "_coef", "_hist", "_noise_coef"):
        a, b = getattr(old, name, None), getattr(new, name, None)
        if a is None or (name not in vars(new) and name != "_noise_coef"):     # (not a buffer of `new`'s class)
            continue
        if torch.is_tensor(a) and (b is None or (torch.is_tensor(b) and b.shape == a.shape and b.dtype == a.dtype)):
            if b is not None:
                a.copy_(b)
            setattr(new, name, a)
            done.append(name)
        elif isinstance(a, tuple) and b is None:
            setattr(new, name, a)
            done.append(name)
    return done


# -- models ------------------------------------------------------------------------------------------------------------------
def model_slot(pipe):
    return "transformer" if hasattr(pipe, "transformer") else "unet"


def model_of(pipe):
    return getattr(pipe, model_slot(pipe))


def _state_dict(model, seed):
    shapes = {"UNet2DConditionModel": dinit.unet_param_shapes, "UNet2DModel": lambda c: dinit.unet2d_param_shapes(dict(c)),
              "FluxTransformer2DModel": dinit.flux_param_shapes, "WanTransformer3DModel": dinit.wan_param_shapes}[type(model).__name__]
    return dinit.random_state_dict(shapes(model.config), seed=seed)


def model_swap():
    """``pipe.unet = other`` / ``pipe.transformer = other``: another object with other weights."""
    def put_back(pipe):
        setattr(pipe, model_slot(pipe), pipe._swapped_out)

    @mutation("recapture", name="model_swap", undo=put_back)
    def fn(pipe, kw):
        old = pipe._swapped_out = model_of(pipe)
        other = type(old)(**dict(old.config))
        other.load_state_dict(_state_dict(old, OTHER_SEED), device=str(old.device))
        setattr(pipe, model_slot(pipe), other)
        return kw
    return fn


def model_reload(own_seed):
    """``load_state_dict`` of other weights on the SAME model object: new packed tensors under the same ``id()``.  (The test holds
    ``packed_cache.packed_tensors(model)`` of before the reload until its asserts are done, so that a wrongly replayed step would
    read live memory.)"""
    def load(pipe, seed):
        m = model_of(pipe)
        m.load_state_dict(_state_dict(m, seed), device=str(m.device))

    @mutation("recapture", name="model_reload", undo=lambda pipe: load(pipe, own_seed))
    def fn(pipe, kw):
        load(pipe, OTHER_SEED)
        return kw
    return fn


def lora_fuse(own_seed):
    """``fuse_lora`` of a small rank-2 adapter (the construction of tests/test_loading.py): the re-pack is in place, a captured step
    follows it; ``unfuse_lora`` takes it back."""
    targets = ["mid_block.attentions.0.transformer_blocks.0.attn1.to_q", "mid_block.attentions.0.transformer_blocks.0.attn2.to_v",
               "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj"]

    def unfuse(pipe):
        pipe.unet.unfuse_lora(base_state_dict=pipe._lora_base)

    @mutation("replay", name="lora_fuse", undo=unfuse)
    def fn(pipe, kw):
        from test_loading import _lora_for
        sd = pipe._lora_base = _state_dict(pipe.unet, own_seed)
        lora, _ = _lora_for(sd, targets, r=2, seed=5)
        # (an update large enough to move bf16 weights, as test_from_pretrained_and_lora_forward_on_gpu scales its adapter)
        lora = {k: (v * 6.0 if k.endswith("lora_B.weight") else v) for k, v in lora.items()}
        pipe.unet.fuse_lora(lora, lora_scale=0.7, base_state_dict=sd)
        return kw
    return fn


# ----------------------------------------------------------------------------------------------------------------------
# families
# ----------------------------------------------------------------------------------------------------------------------
Family = namedtuple("Family", "build kwargs mutations")


def _sd_kwargs(xl, **extra):
    kw = dict(prompt_embeds=_rand((1, 7, 64), 1), negative_prompt_embeds=_rand((1, 7, 64), 2), num_inference_steps=4,
              guidance_scale=5.0, output_type="latent", generator=_gen())
    if xl:
        kw.update(pooled_prompt_embeds=_rand((1, 64), 3), negative_pooled_prompt_embeds=_rand((1, 64), 4))
    kw.update(extra)
    return kw


def _rect_mask(H, W_):
    m = torch.zeros(H, W_)
    m[H // 4:3 * H // 4, W_ // 8:W_ // 2] = 1.0
    return m


def _image(hw):
    return torch.rand(1, 3, hw, hw, generator=torch.Generator("cpu").manual_seed(4))


def _guidance_and_prompt_length():
    """The three SD / SDXL mutations every variant of the family takes."""
    return [_set("recapture", "guidance_scale_5_to_7.5", guidance_scale=7.5),
            _set("recapture", "cfg_off", guidance_scale=1.0),
            _set("recapture", "prompt_7_to_9_tokens", prompt_embeds=_rand((1, 9, 64), 11), negative_prompt_embeds=_rand((1, 9, 64), 12))]


def _sd_txt2img_mutations(table, xl, seed=0):
    def two_images(pipe, kw):
        return dict(kw, num_images_per_prompt=2, latents=_rand((2, 4, 16, 16), 6))
    base = SCHEDULERS[table]["base"]
    muts = _guidance_and_prompt_length() + [
        _set("recapture", "latents_16x16_to_16x24", latents=_rand((1, 4, 16, 24), 6), height=32, width=48),
        _set("recapture", "steps_4_to_6", num_inference_steps=6),
        mutation("recapture", name="images_per_prompt_1_to_2")(two_images),
        _set("recapture", "guidance_rescale_0_to_0.7", guidance_rescale=0.7),
    ]
    if not xl:           # (DDIM's eta is an argument of the SD pipeline only)
        muts.append(_set("recapture", "ddim_eta_0_to_0.5", eta=0.5))
    muts += [scheduler_swap(table, a, b) for a, b in zip(CHAIN, CHAIN[1:])]
    muts += [
        scheduler_swap(table, base, base, dst_cfg=dict(prediction_type="v_prediction"), name="scheduler_epsilon_to_v_prediction"),
        scheduler_swap(table, base, base, dst_cfg=dict(timestep_spacing="trailing"), name="scheduler_leading_to_trailing"),
        scheduler_swap(table, "dpm", "dpm", dst_cfg=dict(use_karras_sigmas=False), name="scheduler_dpm_karras_off"),
        scheduler_swap(table, "dpm", "dpm", src_cfg=dict(use_karras_sigmas=False), name="scheduler_dpm_karras_on"),
        model_swap(), model_reload(seed),
        _set("replay", "other_prompt_same_length", prompt_embeds=_rand((1, 7, 64), 21)),
        lora_fuse(seed),
    ]
    if xl:
        muts.append(_set("replay", "sdxl_size_conditioning", original_size=(64, 64), target_size=(48, 48), crops_coords_top_left=(4, 8)))
    return muts


def _flux_kwargs(**extra):
    kw = dict(prompt_embeds=_rand((1, 16, 64), 1), pooled_prompt_embeds=_rand((1, 64), 2), num_inference_steps=4, guidance_scale=0.0,
              max_sequence_length=16, output_type="latent", generator=_gen())
    kw.update(extra)
    return kw


def _flux_mutations(txt2img):
    muts = [
        _set("recapture", "steps_4_to_6", num_inference_steps=6),
        scheduler_swap("flux", "flowmatch", "flowmatch", dst_cfg=dict(shift=3.0), name="scheduler_other_shift"),
        model_reload(5),
        _set("replay", "other_pooled_embeds", pooled_prompt_embeds=_rand((1, 64), 22)),
    ]
    if txt2img:
        @mutation("replay", name="64x32_after_32x64", base=lambda kw: dict(kw, height=32, width=64))
        def transposed(pipe, kw):
            return dict(kw, height=64, width=32)
        muts += [
            _set("recapture", "sequence_16_to_24", prompt_embeds=_rand((1, 24, 64), 11), max_sequence_length=24),
            model_swap(), transposed,
        ]
        # (TINY_FLUX has guidance_embeds=False: guidance_scale reaches no kernel, so there is no guidance mutation)
    return muts


def _wan_mutations():
    return [
        _set("recapture", "guidance_5_to_1", guidance_scale=1.0),
        scheduler_swap("wan", "flowmatch", "unipc"),
        scheduler_swap("wan", "unipc", "flowmatch"),
        _set("recapture", "frames_9_to_5", num_frames=5),
        _set("recapture", "steps_3_to_5", num_inference_steps=5),
        model_swap(), model_reload(9),
        _set("replay", "other_prompt_embeds", prompt_embeds=_rand((1, 16, 64), 21)),
    ]


def _ddpm_mutations():
    return [
        _set("recapture", "steps_5_to_7", num_inference_steps=7),
        _set("recapture", "batch_1_to_2", batch_size=2),
        model_reload(11), model_swap(),
        scheduler_swap("ddpm", "ddpm", "ddpm", dst_cfg=dict(variance_type="fixed_large"), name="scheduler_other_variance_type"),
    ]


FAMILIES = {
    "sd15": Family(lambda dev: factory.build_sd15_pipeline(device=dev, tiny=True, seed=0),
                   _sd_kwargs(False, latents=_rand((1, 4, 16, 16), 5), height=32, width=32), _sd_txt2img_mutations("sd15", False)),
    "sdxl": Family(lambda dev: factory.build_sdxl_pipeline(device=dev, tiny=True, seed=0),
                   _sd_kwargs(True, latents=_rand((1, 4, 16, 16), 5), height=32, width=32), _sd_txt2img_mutations("sdxl", True)),
    "sdxl_img2img": Family(lambda dev: factory.build_sdxl_pipeline(device=dev, tiny=True, seed=0, img2img=True),
                           _sd_kwargs(True, image=_image(32), strength=0.5), _guidance_and_prompt_length()),
    "sd15_inpaint": Family(lambda dev: factory.build_sd15_pipeline(device=dev, tiny=True, seed=0, inpaint=True),
                           _sd_kwargs(False, image=_image(32), mask_image=_rect_mask(32, 32), strength=0.5),
                           _guidance_and_prompt_length()),
    "flux": Family(lambda dev: factory.build_flux_pipeline(device=dev, tiny=True, seed=5),
                   _flux_kwargs(height=64, width=64), _flux_mutations(True)),
    "flux_img2img": Family(lambda dev: factory.build_flux_pipeline(device=dev, tiny=True, seed=5, img2img=True),
                           _flux_kwargs(image=_image(64), strength=0.6), _flux_mutations(False)),
    "wan": Family(lambda dev: factory.build_wan_pipeline(device=dev, tiny=True, seed=9),
                  dict(prompt_embeds=_rand((1, 16, 64), 1), negative_prompt_embeds=_rand((1, 16, 64), 2), num_inference_steps=3,
                       guidance_scale=5.0, height=64, width=64, num_frames=9, output_type="latent", generator=_gen()),
                  _wan_mutations()),
    "ddpm": Family(lambda dev: factory.build_ddpm_pipeline(device=dev, tiny=True, seed=11),
                   dict(batch_size=1, num_inference_steps=5, output_type="raw", generator=_gen(0)), _ddpm_mutations()),
}

CASES = [(name, m) for name, fam in FAMILIES.items() for m in fam.mutations]
CASE_IDS = [f"{name}-{m.name}" for name, m in CASES]


def hold_packed(pipe):
    """References to every packed tensor of the pipeline's denoiser as it is now."""
    return packed_cache.packed_tensors(model_of(pipe))
