"""The case table of tests/test_sd_call_paths_cpu.py and tools/record_sd_call_paths.py: what the six SD / SDXL ``__call__``
methods do between their arguments and the denoising loop.

Every case is one call of a ``device="cpu"`` tiny pipeline over the kernel stand-ins, with ``_denoise`` replaced by a stand-in that
records what it is handed and returns the latents.  Images are 4-channel latents and 9-channel U-Nets get ``masked_image_latents``,
so no VAE encoder runs: everything recorded comes from CPU generator draws, copies, concatenations and elementwise bf16 arithmetic
and is compared bit for bit with tests/golden/sd_call_paths.npz (valid calls) and sd_call_paths.json (refused calls), which
tools/record_sd_call_paths.py wrote from this table.

  CASES     valid calls; ``record(case)`` returns ``(arrays, meta)``: the tensors as numpy arrays (bf16 as its int16 bits) and
            everything else as JSON
  ERRORS    calls that are invalid in exactly one way; ``record_error(case)`` returns the exception's type name and message
"""
import functools
import hashlib
import json
from collections import namedtuple

import numpy as np
import torch

import call_sequences as CS
from diffusers_amd import factory, init as dinit, pipelines as P

bf16 = torch.bfloat16
F = 2                   # the tiny VAE's scale factor
LAT = (4, 6)            # latent height x width of every case: small (the golden file holds every tensor) and not square
KINDS = ("sd", "sd_i2i", "sd_inp", "xl", "xl_i2i", "xl_inp")
SD3, XL3 = KINDS[:3], KINDS[3:]
IMG4, XL2, INP2, TXT2 = ("sd_i2i", "sd_inp", "xl_i2i", "xl_inp"), ("xl_i2i", "xl_inp"), ("sd_inp", "xl_inp"), ("sd", "xl")
SCHEDULE5 = ("sd_i2i", "sd_inp") + XL3          # the pipelines that take `timesteps` / `sigmas`
DROP = object()         # a base argument the case leaves out

Case = namedtuple("Case", "name kind changes scheduler in_ch aesthetics refiner_unet stub_prompt global_seed")
_rand = CS._rand


def _case(name, kind, scheduler=None, in_ch=4, aesthetics=None, refiner_unet=None, stub_prompt=False, global_seed=None, **changes):
    """``aesthetics``: the pipeline's ``requires_aesthetics_score``, on a U-Net shaped for it unless ``refiner_unet`` says otherwise."""
    refiner_unet = bool(aesthetics) if refiner_unet is None else refiner_unet
    return Case(f"{kind}-{name}", kind, changes, scheduler, in_ch, aesthetics, refiner_unet, stub_prompt, global_seed)


def _over(kinds, name, **kw):
    return [_case(name, k, **kw) for k in kinds]


def _mask():
    return CS._rect_mask(LAT[0] * F, LAT[1] * F)


def base_kwargs(kind):
    kw = dict(prompt_embeds=_rand((1, 3, 64), 1), negative_prompt_embeds=_rand((1, 3, 64), 2), num_inference_steps=4,
              guidance_scale=5.0, output_type="latent", generator=CS._gen())
    if kind.startswith("xl"):
        kw.update(pooled_prompt_embeds=_rand((1, 64), 3), negative_pooled_prompt_embeds=_rand((1, 64), 4))
    if kind in TXT2:
        kw.update(height=LAT[0] * F, width=LAT[1] * F)
    else:
        kw.update(image=_rand((1, 4) + LAT, 5), strength=0.5)
    if kind in INP2:
        kw.update(mask_image=_mask())
    return kw


def _batch2(kind):
    kw = dict(prompt_embeds=_rand((2, 3, 64), 11), negative_prompt_embeds=_rand((2, 3, 64), 12))
    if kind.startswith("xl"):
        kw.update(pooled_prompt_embeds=_rand((2, 64), 13), negative_pooled_prompt_embeds=_rand((2, 64), 14))
    kw.update(latents=_rand((2, 4) + LAT, 6)) if kind in TXT2 else kw.update(image=_rand((2, 4) + LAT, 15))
    return kw


_NO_EMBEDS = dict(prompt_embeds=DROP, negative_prompt_embeds=DROP, pooled_prompt_embeds=DROP, negative_pooled_prompt_embeds=DROP)
_SIZES = dict(original_size=(64, 48), crops_coords_top_left=(4, 8), target_size=(40, 56))
_NEG_SIZES = dict(negative_original_size=(32, 24), negative_crops_coords_top_left=(2, 6), negative_target_size=(20, 28))
_TIMESTEPS, _SIGMAS = [900, 600, 300, 100], [10.0, 4.0, 1.5, 0.5, 0.0]


def _valid_cases():
    c = []
    c += _over(KINDS, "defaults")
    c += _over(KINDS, "cfg_off", guidance_scale=1.0, negative_prompt_embeds=DROP, negative_pooled_prompt_embeds=DROP)
    c += _over(KINDS, "two_per_prompt_tuple_out", num_images_per_prompt=2, return_dict=False)
    c += [_case("batch_of_2", k, **_batch2(k)) for k in KINDS]
    c += _over(KINDS, "prompt_strings", stub_prompt=True, prompt=["a cat", "a dog"], negative_prompt="blurry", clip_skip=1,
               **_NO_EMBEDS)
    c += _over(XL3, "prompt_2", stub_prompt=True, prompt="a cat", prompt_2="a dog", negative_prompt_2="dull", guidance_scale=1.0,
               **_NO_EMBEDS)
    c += _over(KINDS, "guidance_rescale", guidance_rescale=0.7)
    c += _over(TXT2 + ("xl_i2i",), "no_generator", generator=DROP, global_seed=17)
    # schedules
    c += _over(XL3, "custom_timesteps", timesteps=_TIMESTEPS)
    c += _over(XL3, "custom_sigmas", sigmas=_SIGMAS)
    c += _over(("sd_i2i", "sd_inp"), "custom_timesteps", scheduler="euler", timesteps=_TIMESTEPS)
    c += _over(("sd_i2i", "sd_inp"), "custom_sigmas", scheduler="euler", sigmas=_SIGMAS)
    c += _over(XL2, "custom_timesteps_strength_0.75", timesteps=_TIMESTEPS, strength=0.75)
    c += [_case("denoising_end", "xl", num_inference_steps=8, denoising_end=0.6)]
    c += _over(XL2, "denoising_end_over_the_tail", num_inference_steps=8, strength=0.75, denoising_end=0.6)
    c += _over(XL2, "denoising_start", num_inference_steps=8, denoising_start=0.4)
    c += _over(XL2, "denoising_start_and_end", num_inference_steps=8, denoising_start=0.4, denoising_end=0.8)
    c += _over(XL3, "denoising_end_not_a_fraction", denoising_end=1.0)
    c += _over(IMG4, "strength_1", strength=1.0)
    c += _over(IMG4, "strength_0.3_of_10", strength=0.3, num_inference_steps=10)
    # supplied latents
    c += [_case("latents_shortcut", "xl_i2i", image=DROP, latents=_rand((1, 4) + LAT, 6))]
    c += _over(INP2, "supplied_latents", latents=_rand((1, 4) + LAT, 6))
    c += _over(TXT2, "supplied_latents", latents=_rand((1, 4) + LAT, 6))
    # SDXL size conditioning
    c += _over(XL3, "sizes", **_SIZES)
    c += _over(XL2, "negative_sizes", **_SIZES, **_NEG_SIZES)
    c += _over(XL2, "aesthetics_score", aesthetics=True, aesthetic_score=6.1, negative_aesthetic_score=2.25, **_SIZES, **_NEG_SIZES)
    c += _over(XL2, "aesthetics_score_cfg_off", aesthetics=True, guidance_scale=1.0)
    c += _over(XL2, "no_aesthetics_score", aesthetics=False, aesthetic_score=6.1, **_NEG_SIZES)
    # samplers
    c += _over(SD3, "ddim_eta", eta=0.5)
    c += _over(SD3, "ddim_eta_1", eta=1.0, num_inference_steps=3)
    for s in ("euler", "euler_a", "dpm"):
        c += _over(KINDS, s, scheduler=s)
    c += _over(XL3, "ddim", scheduler="ddim")
    c += _over(IMG4, "euler_a_strength_1", scheduler="euler_a", strength=1.0)
    c += _over(XL2, "euler_a_denoising_start_and_end", scheduler="euler_a", num_inference_steps=8, denoising_start=0.4,
               denoising_end=0.8)
    c += _over(KINDS, "euler_a_two_per_prompt", scheduler="euler_a", num_images_per_prompt=2)
    # 9-channel inpainting U-Nets
    masked = _rand((1, 4) + LAT, 8)
    c += _over(INP2, "9_channels", in_ch=9, masked_image_latents=masked)
    c += _over(INP2, "9_channels_euler_strength_1", in_ch=9, scheduler="euler", strength=1.0, masked_image_latents=masked)
    c += _over(INP2, "9_channels_two_per_prompt", in_ch=9, num_images_per_prompt=2, masked_image_latents=masked)
    c += [_case("mask_per_sample", k, mask_image=torch.stack([_mask(), 1 - _mask()])[:, None], **_batch2(k)) for k in INP2]
    return c


def _error_cases():
    e = []
    e += _over(KINDS, "prompt_and_embeds", prompt="a cat")
    e += _over(KINDS, "no_prompt_no_embeds", **_NO_EMBEDS)
    e += _over(KINDS, "cfg_without_negatives", negative_prompt_embeds=DROP, negative_pooled_prompt_embeds=DROP)
    e += _over(XL3, "cfg_without_negative_pooled", negative_pooled_prompt_embeds=DROP)
    e += _over(XL3, "no_pooled", pooled_prompt_embeds=DROP)
    e += _over(IMG4, "strength_above_1", strength=1.5)
    e += _over(IMG4, "strength_below_0", strength=-0.1)
    e += _over(IMG4, "strength_leaves_no_steps", strength=0.1)
    e += _over(IMG4, "no_image", image=DROP)
    e += _over(INP2, "no_mask", mask_image=DROP)
    e += _over(SD3, "eta_above_1", eta=1.5)
    e += _over(SD3, "eta_below_0", eta=-0.5)
    e += _over(XL2, "eta_not_0", eta=0.5)
    for s in ("euler", "euler_a", "dpm"):
        e += _over(SD3, f"eta_with_{s}", scheduler=s, eta=0.5)
    e += _over(INP2, "ip_adapter_image", ip_adapter_image=torch.zeros(1, 3, 8, 8))
    e += _over(INP2, "ip_adapter_image_embeds", ip_adapter_image_embeds=[torch.zeros(1, 1, 8)])
    e += _over(INP2, "padding_mask_crop", padding_mask_crop=4)
    for s in ("euler", "ddim", "euler_a", "dpm"):
        e += _over(SCHEDULE5, f"timesteps_and_sigmas_{s}", scheduler=s, timesteps=_TIMESTEPS, sigmas=_SIGMAS)
        if s != "euler":       # (Euler takes them: CASES)
            e += _over(SCHEDULE5, f"custom_timesteps_{s}", scheduler=s, timesteps=_TIMESTEPS)
            e += _over(SCHEDULE5, f"custom_sigmas_{s}", scheduler=s, sigmas=_SIGMAS)
    e += _over(XL2, "denoising_start_not_below_end", denoising_start=0.6, denoising_end=0.6)
    e += _over(TXT2, "latents_batch", latents=_rand((2, 4) + LAT, 6))
    e += [_case("latents_batch", "xl_i2i", image=DROP, latents=_rand((2, 4) + LAT, 6))]
    e += _over(INP2, "latents_batch", latents=_rand((2, 4) + LAT, 6))
    e += _over(IMG4, "image_batch", image=_rand((3, 4) + LAT, 5), num_images_per_prompt=2)
    e += _over(KINDS, "callback_tensor_inputs", callback_on_step_end_tensor_inputs=["latents", "prompt_embeds"])
    e += _over(KINDS, "zero_per_prompt", num_images_per_prompt=0)
    e += _over(TXT2, "generator_list", num_images_per_prompt=2, generator=lambda: [CS._gen(3)(), CS._gen(4)()])
    e += _over(XL2, "aesthetics_score_on_a_base_unet", aesthetics=True, refiner_unet=False)
    e += _over(XL2, "no_aesthetics_score_on_a_refiner_unet", aesthetics=False, refiner_unet=True)
    return e


CASES, ERRORS = _valid_cases(), _error_cases()
assert len({c.name for c in CASES}) == len(CASES) and len({c.name for c in ERRORS}) == len(ERRORS)


# ----------------------------------------------------------------------------------------------------------------------
# pipelines
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _built(kind, in_ch):
    build = factory.build_sdxl_pipeline if kind.startswith("xl") else factory.build_sd15_pipeline
    return build(device="cpu", tiny=True, seed=0, img2img=kind.endswith("i2i"), inpaint=kind.endswith("inp"), unet_in_channels=in_ch)


@functools.lru_cache(maxsize=None)
def _refiner_unet():
    """A refiner-shaped U-Net (five added time ids: ``requires_aesthetics_score``), as test_img2img_cpu builds it."""
    cfg = dict(dinit.TINY_SDXL_UNET)
    cfg["projection_class_embeddings_input_dim"] -= cfg["addition_time_embed_dim"]
    return factory.build_unet(cfg, seed=0, device="cpu")[0]


def make_pipe(case):
    """A new pipeline object per call (no noise buffer, inpainting inputs or captured step left by another case) around the
    factory's components, with a new scheduler of the case's kind."""
    src = _built(case.kind, case.in_ch)
    table = "sdxl" if case.kind.startswith("xl") else "sd15"
    sch = CS.SCHEDULERS[table][case.scheduler or CS.SCHEDULERS[table]["base"]]()
    kw, unet = {}, src.unet
    if case.aesthetics is not None:
        kw["requires_aesthetics_score"] = case.aesthetics
    if case.refiner_unet:
        unet = _refiner_unet()
    return type(src)(vae=src.vae, unet=unet, scheduler=sch, **kw)


def call_kwargs(case):
    kw = dict(base_kwargs(case.kind), **case.changes)
    return {k: v for k, v in kw.items() if v is not DROP}


# ----------------------------------------------------------------------------------------------------------------------
# recording
# ----------------------------------------------------------------------------------------------------------------------
def _plain(v):
    """``v`` as JSON: what a call was handed, without addresses."""
    if torch.is_tensor(v):
        return {"tensor": v.detach().float().cpu().reshape(-1).tolist(), "shape": list(v.shape), "dtype": str(v.dtype)}
    if isinstance(v, np.ndarray):
        return {"array": v.reshape(-1).tolist(), "shape": list(v.shape), "dtype": str(v.dtype)}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (torch.device, torch.dtype)):
        return str(v)
    if isinstance(v, torch.Generator):
        return "generator"
    if isinstance(v, np.generic):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


def _arrays_of(prefix, t, arrays, meta):
    if t is None:
        meta["tensors"][prefix] = None
        return
    t = t.detach()
    meta["tensors"][prefix] = [str(t.dtype), list(t.shape), str(t.device)]
    t = t.cpu().contiguous()
    arrays[prefix] = (t.view(torch.int16) if t.dtype == bf16 else t).numpy().copy()


def masked_key(key):
    """A graph key with what differs from process to process taken out: addresses become "is there one", the generation of the
    packed weights and the scheduler's serial are dropped."""
    key = list(key)
    key[4] = bool(key[4])                                         # the noise table's address
    tail = key[7:12]                                              # _key_tail: table, step counter, weights, buffers, token
    key[7:12] = ["ptr", "ptr", "generation", len(tail[3]), [tail[4][0], tail[4][2]]]
    return _plain([(e[0], bool(e[1]), e[2]) if isinstance(e, tuple) and len(e) == 3 and isinstance(e[0], str) else e for e in key])


class _Spies:
    """``torch.randn`` and the pipelines' ``_randn`` logged in call order while a pipeline call runs."""

    def __init__(self, draws):
        self.draws = draws

    def __enter__(self):
        self.randn, self.p_randn = torch.randn, P._randn
        draws = self.draws

        def randn(*a, **k):
            shape = a[0] if len(a) == 1 and not isinstance(a[0], int) else a
            draws.append(["torch.randn", list(shape), str(k.get("dtype")), str(k.get("device")), k.get("generator") is not None])
            return self.randn(*a, **k)

        def p_randn(shape, generator, device, dtype):
            draws.append(["_randn", list(shape), str(dtype), str(device),
                          "list" if isinstance(generator, (list, tuple)) else generator is not None])
            return self.p_randn(shape, generator, device, dtype)

        torch.randn, P._randn = randn, p_randn
        return self

    def __exit__(self, *exc):
        torch.randn, P._randn = self.randn, self.p_randn
        return False


def _stub_encode_prompt(pipe, log):
    xl = hasattr(pipe, "text_encoder_2")

    def encode_prompt(*a, **k):
        log.append(_plain([a, k]))
        n = 2 * a[3 if xl else 2] if isinstance(a[0], list) else a[3 if xl else 2]
        out = (_rand((n, 3, 64), 31), _rand((n, 3, 64), 32))
        return out + (_rand((n, 64), 33), _rand((n, 64), 34)) if xl else out
    pipe.encode_prompt = encode_prompt


def _prepared(case, log=None):
    pipe = make_pipe(case)
    if case.stub_prompt:
        _stub_encode_prompt(pipe, [] if log is None else log)
    if case.global_seed is not None:
        torch.manual_seed(case.global_seed)
    return pipe, CS.materialise(call_kwargs(case), "cpu")


def _digest(t):
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def record(case):
    """One valid call: ``(arrays, meta)``."""
    arrays, meta = {}, {"tensors": {}, "draws": [], "scheduler_calls": [], "encode_prompt": [], "conditioning_calls": 0}
    pipe, kw = _prepared(case, meta["encode_prompt"])
    sch, unet = pipe.scheduler, pipe.unet
    for name in ("set_timesteps", "set_begin_index"):
        real = getattr(sch, name)
        # (a keyword handed over as None is the scheduler's default: `timesteps=ts, sigmas=None` is the call `timesteps=ts`)
        setattr(sch, name, lambda *a, _n=name, _r=real, **k: meta["scheduler_calls"].append(
            [_n, _plain(a), _plain({key: v for key, v in k.items() if v is not None})]) or _r(*a, **k))
    precompute = unet.precompute_conditioning

    def spy_conditioning(pe, added):
        i = meta["conditioning_calls"]
        meta["conditioning_calls"] = i + 1
        _arrays_of(f"cond{i}.prompt_embeds", pe, arrays, meta)
        meta[f"cond{i}.contiguous"] = pe.is_contiguous()
        for k in ("text_embeds", "time_ids"):
            _arrays_of(f"cond{i}.{k}", None if added is None else added[k], arrays, meta)
        return precompute(pe, added)

    def denoise(latents, step_args, num_steps, use_graph, begin=0):
        cond, guidance_scale, do_cfg = step_args
        meta["denoise"] = dict(n_steps=num_steps, begin=begin, use_graph=use_graph, guidance_scale=guidance_scale, do_cfg=do_cfg,
                               cond_keys=sorted(cond), eta=pipe._eta, guidance_rescale=pipe._guidance_rescale,
                               inpaint=None if getattr(pipe, "_inpaint", None) is None else sorted(pipe._inpaint),
                               callback_armed=pipe._step_callback is not None, interrupt=pipe._interrupt,
                               noise_table_is_buffer=pipe._noise_table is not None and pipe._noise_table is pipe._noise_buffer)
        _arrays_of("latents", latents, arrays, meta)
        meta["latents_contiguous"] = latents.is_contiguous()
        _arrays_of("noise_table", pipe._noise_table, arrays, meta)
        for k, v in (getattr(pipe, "_inpaint", None) or {}).items():
            _arrays_of(f"inpaint.{k}", v, arrays, meta)
        return latents

    pipe._denoise = denoise
    unet.precompute_conditioning = spy_conditioning
    try:
        with _Spies(meta["draws"]):
            out = pipe(**kw)
    finally:
        del unet.precompute_conditioning
    meta["return"] = [type(out).__name__, len(out) if isinstance(out, tuple) else None]
    images = out[0] if isinstance(out, tuple) else out.images
    meta["returns_the_loop_latents"] = bool(torch.equal(images, torch.from_numpy(arrays["latents"]).view(images.dtype)
                                                        if images.dtype == bf16 else torch.from_numpy(arrays["latents"])))
    meta["scheduler"] = [type(sch).__name__, sch.begin_index]
    _arrays_of("timesteps", torch.as_tensor(sch.timesteps), arrays, meta)
    g = kw.get("generator")
    state = g.get_state() if g is not None else torch.get_rng_state()
    meta["generator_after"] = _digest(state)
    # the same call up to the capture key, on a pipeline of its own
    pipe2 = make_pipe(case)
    if case.stub_prompt:
        _stub_encode_prompt(pipe2, [])
    meta["graph_key"] = masked_key(CS.graph_key_of(pipe2, {k: v for k, v in call_kwargs(case).items() if k != "use_graph"}))
    return arrays, json.loads(json.dumps(meta))


def record_error(case):
    """One refused call: the exception's type name and message ("no error" when the call goes through)."""
    pipe, kw = _prepared(case)
    pipe._denoise = lambda latents, *a, **k: latents
    try:
        pipe(**kw)
    except Exception as exc:        # noqa: BLE001  (whatever the call raises is what is recorded)
        return {"type": type(exc).__name__, "message": str(exc)}
    return {"type": None, "message": "no error"}
