"""EulerAncestralDiscreteScheduler ("Euler a"), host side -- no kernel runs here.

The reference implementation is not available to the suite, so this file restates its arithmetic: ``ref_schedule`` (timesteps and
sigmas for the three spacings, numpy floats) and ``ref_step`` (the op chain of ``scheduling_euler_ancestral_discrete.py`` ``step``,
written once with torch CPU ops on 0-d fp32 sigmas, every rounding point where the reference has it).  ``ref_step`` serves twice:
``euler_ancestral_step`` below wraps it as the CPU stand-in that is monkeypatched over ``ops.euler_ancestral_step``, and
``tests/test_euler_ancestral_gpu.py`` imports it as the expected value of the kernel, bit for bit (the chain is the same IEEE
operations).  It reads only slots 0 and 1 (sigma, sigma_to) of a table row: dt, c_out, sigma^2 + 1 and sigma_up are recomputed here,
so the slots the scheduler wrote are checked too."""
import json

import numpy as np
import pytest
import torch

from diffusers_amd import _lib as L
from diffusers_amd import factory, ops
from diffusers_amd.schedulers import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,
                                      EulerDiscreteScheduler)

import inpaint_emulation

bf16 = torch.bfloat16
SD_BETAS = dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)
SPACINGS = ("linspace", "leading", "trailing")


# ----------------------------------------------------------------------------------------------------------------------
# restatement
# ----------------------------------------------------------------------------------------------------------------------
def ref_base_sigmas(beta_schedule="linear", beta_start=1e-4, beta_end=0.02, N=1000):
    """((1 - abar) / abar) ** 0.5 of the training schedule with fp32 torch, as the reference's __init__ builds it."""
    if beta_schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, N, dtype=torch.float32)
    else:
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, N, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0)
    return (((1 - ac) / ac) ** 0.5).numpy()


def ref_schedule(n, spacing, steps_offset=0, N=1000, **betas):
    """(timesteps float32 [n], sigmas float32 [n + 1], init_noise_sigma)."""
    base = ref_base_sigmas(N=N, **betas)
    if spacing == "linspace":
        ts = np.linspace(0, N - 1, n, dtype=np.float32)[::-1].copy()
    elif spacing == "leading":
        ts = (np.arange(0, n) * (N // n)).round()[::-1].copy().astype(np.float32) + steps_offset
    else:
        ts = np.arange(N, 0, -N / n).round() - 1
    sig = np.interp(ts, np.arange(N), base)
    sig = np.concatenate([sig, [0.0]]).astype(np.float32)
    smax = sig.max()
    init = smax if spacing in ("linspace", "trailing") else (np.float32(smax) ** 2 + 1) ** 0.5
    return ts.astype(np.float32), sig, float(init)


def ref_combine(model_output, cfg, guidance):
    """noise_pred = uncond + g (text - uncond), every op in the model output's dtype ([2][...] = (uncond, cond))."""
    if not cfg:
        return model_output
    u, c = model_output[0], model_output[1]
    return u + guidance * (c - u)


def ref_step(model_output, sample, noise, sigma, sigma_to, prediction_type="epsilon"):
    """scheduling_euler_ancestral_discrete.py step: ``sigma`` / ``sigma_to`` are 0-d fp32 CPU tensors (they promote nothing)."""
    assert sigma.dim() == 0 and sigma.dtype == torch.float32 and sigma_to.dtype == torch.float32
    sample = sample.to(torch.float32)
    if prediction_type == "epsilon":
        # `sigma * model_output` as the reference runs on a device: the 0-d fp32 sigma stays fp32 and the product is rounded once, in
        # the model output's dtype.  torch's CPU kernels round a 0-d scalar written FIRST to bf16 before multiplying (they keep it in
        # fp32 when the tensor comes first, as in the other two products below), so the product is spelled out here.
        pred_original_sample = sample - (model_output.to(torch.float32) * sigma).to(model_output.dtype)
    elif prediction_type == "v_prediction":
        pred_original_sample = model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
    else:
        raise NotImplementedError("prediction_type not implemented yet: sample")
    sigma_up = (sigma_to ** 2 * (sigma ** 2 - sigma_to ** 2) / sigma ** 2) ** 0.5
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    derivative = (sample - pred_original_sample) / sigma
    dt = sigma_down - sigma
    prev_sample = sample + derivative * dt
    assert noise.dtype == model_output.dtype
    prev_sample = prev_sample + noise * sigma_up
    return prev_sample.to(model_output.dtype)


def ref_step_row(model_output, sample, noise, row, *, cfg=False, guidance=0.0, pred_type=0):
    """``ref_step`` from a table row (slots 0 and 1 only), with the CFG combine in front; flat or shaped operands."""
    row = torch.as_tensor(row, dtype=torch.float32)
    e = ref_combine(model_output.reshape((2, -1) if cfg else (-1,)), cfg, guidance)
    out = ref_step(e, sample.reshape(-1), noise.reshape(-1), row[0], row[1], ("epsilon", "v_prediction")[pred_type])
    return out.view(sample.shape)


# CPU stand-in of ops.euler_ancestral_step
def euler_ancestral_step(eps, x, noise, table, step_idx, *, cfg, guidance, out=None, pred_type=0, noise_step_stride=0):
    assert noise is not None and noise.dtype == eps.dtype == x.dtype and table.shape[1] == 8
    i, n = int(step_idx), x.numel()
    assert noise.numel() >= (table.shape[0] - 1) * noise_step_stride + n
    nz = noise.reshape(-1)[i * noise_step_stride:i * noise_step_stride + n]
    prev = ref_step_row(eps, x, nz, table[i].cpu(), cfg=cfg, guidance=guidance, pred_type=pred_type)
    if out is not None:
        out.copy_(prev)
        return out
    return prev


@pytest.fixture(autouse=True)
def _emulated_kernels(monkeypatch):
    inpaint_emulation.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "euler_ancestral_step", euler_ancestral_step)
    monkeypatch.setattr(ops, "TUNING", False)


def _sched(n=None, **kw):
    cfg = dict(SD_BETAS)
    cfg.update(kw)
    s = EulerAncestralDiscreteScheduler(**cfg)
    if n is not None:
        s.set_timesteps(n, device="cpu")
    return s


# ----------------------------------------------------------------------------------------------------------------------
# schedule
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("betas", [SD_BETAS, {}], ids=["sd", "default"])
def test_schedule_equals_the_restatement_and_shares_the_euler_row(spacing, betas):
    for n in (1, 4, 20):
        off = 1 if spacing == "leading" else 0
        kw = dict(betas, timestep_spacing=spacing, steps_offset=off)
        s = EulerAncestralDiscreteScheduler(**kw)
        s.set_timesteps(n, device="cpu")
        ts, sig, init = ref_schedule(n, spacing, steps_offset=off, **betas)
        assert s.timesteps.dtype == torch.float32 and s.sigmas.dtype == torch.float32 and s.sigmas.device.type == "cpu"
        assert np.array_equal(s.timesteps.numpy(), ts) and np.array_equal(s.sigmas.numpy(), sig), (n, spacing)
        assert float(s.init_noise_sigma) == pytest.approx(init, rel=1e-6)
        assert s.num_inference_steps == n and s.order == 1 and s.step_index is None and s.begin_index is None
        rows = s.device_table.numpy()
        assert rows.dtype == np.float32 and rows.shape == (n, 8) and np.isfinite(rows).all()
        e = EulerDiscreteScheduler(**kw)
        e.set_timesteps(n, device="cpu")
        assert np.array_equal(e.timesteps.numpy(), ts) and np.array_equal(e.sigmas.numpy(), sig)
        for slot in (0, 1, 3, 4, 5, 7):
            assert np.array_equal(rows[:, slot], e.device_table.numpy()[:, slot]), slot
        assert rows[-1, 6] == 0.0 and rows[-1, 2] == -rows[-1, 0] and rows[-1, 1] == 0.0
        assert (rows[:-1, 6] > 0).all() and (rows[:, 2] < 0).all()
        # slots 2 and 6 are the restatement's fp32 scalar chain
        for i in range(n):
            sg, st = torch.tensor(sig[i]), torch.tensor(sig[i + 1])
            up = (st ** 2 * (sg ** 2 - st ** 2) / sg ** 2) ** 0.5
            assert rows[i, 6] == float(up) and rows[i, 2] == float((st ** 2 - up ** 2) ** 0.5 - sg)


def test_variance_identity_of_every_row():
    """sigma_down^2 + sigma_up^2 = sigma_to^2.  The fp32 chain takes ~6 roundings for sigma_up and 3 more for sigma_down, each
    2^-24 relative to a value <= sigma_to^2 (sigma_down^2 is a difference whose operands are <= sigma_to^2): 2^-20 sigma_to^2."""
    for spacing in SPACINGS:
        s = _sched(20, timestep_spacing=spacing, steps_offset=int(spacing == "leading"))
        rows = s.device_table.double().numpy()
        for r in rows:
            down, up, to = r[2] + r[0], r[6], r[1]
            assert abs(down ** 2 + up ** 2 - to ** 2) <= 2.0 ** -20 * to ** 2 + 0.0, (spacing, r)
            assert 0.0 <= down <= to and 0.0 <= up <= to


# ----------------------------------------------------------------------------------------------------------------------
# closed forms
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_last_step_of_an_exact_model_with_zero_noise_returns_x0(pred):
    """A model that always returns the epsilon (or v) of a fixed x0: on the last row sigma_to = 0, so sigma_up = sigma_down = 0,
    dt = -sigma and prev = x - ((x - x0) / sigma) sigma = x0 up to the fp32 roundings of x at |x| ~ |x0| + sigma |z|."""
    n = 6
    s = _sched(n, prediction_type=pred)
    g = torch.Generator().manual_seed(0)
    x0, z = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    s.reset(n - 1)
    sigma = s.sigmas[n - 1]
    x = x0 + sigma * z
    if pred == "epsilon":
        out = z
    else:       # v = alpha eps - sigma_vp x0 with alpha = 1 / sqrt(sigma^2 + 1), sigma_vp = sigma alpha; the scheduler's sample is x / alpha
        al = 1 / (sigma ** 2 + 1) ** 0.5
        out = al * z - sigma * al * x0
    table = torch.zeros(n, *x.shape)
    got = s.step_cfg(out, x.clone(), 0.0, cfg=False, noise_table=table)
    assert s.step_index == n
    tol = 2.0 ** -20 * (x0.abs() + float(sigma) * z.abs() + 1.0)
    assert ((got - x0).abs() <= tol).all()
    with pytest.raises(IndexError):
        s.step_cfg(out, x.clone(), 0.0, cfg=False, noise_table=table)


def test_variance_after_every_step_is_the_next_sigma_squared():
    """x0 = 0 and an exact epsilon model (eps = x / sigma): x_{i+1} = x_i sigma_down / sigma + sigma_up n is N(0, sigma_{i+1}^2) per
    element when x_i is N(0, sigma_i^2).  N = 65536 fp32 elements: the sample variance of N normal values has relative standard
    deviation sqrt(2 / N) = 5.5e-3; the 5-sigma bound is 2.8e-2 (fp32 rounding, 1e-7, is far below it)."""
    n, N = 20, 65536
    bound = 5.0 * (2.0 / N) ** 0.5
    s = _sched(n)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 4, 128, 128, generator=g) * s.sigmas[0]
    assert x.numel() == N
    for i, t in enumerate(s.timesteps):
        x = s.step(x / s.sigmas[i], t, x, generator=g).prev_sample
        target = float(s.sigmas[i + 1]) ** 2
        var = float(x.double().pow(2).mean())
        if i < n - 1:
            assert abs(var / target - 1.0) <= bound, (i, var, target)
        else:
            assert var <= 1e-10        # the last step returns x0 = 0 up to rounding
    assert s.step_index == n


# ----------------------------------------------------------------------------------------------------------------------
# generator stream
# ----------------------------------------------------------------------------------------------------------------------
def _embeds(kind):
    g = torch.Generator().manual_seed(3)
    d = dict(prompt_embeds=torch.randn((1, 7, 64), generator=g).to(bf16), negative_prompt_embeds=torch.randn((1, 7, 64), generator=g).to(bf16),
             output_type="latent", use_graph=False)
    if kind == "sdxl":
        d.update(pooled_prompt_embeds=torch.randn((1, 64), generator=g).to(bf16),
                 negative_pooled_prompt_embeds=torch.randn((1, 64), generator=g).to(bf16))
    return d


def _pipe(kind, **kw):
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    pipe = build(device="cpu", tiny=True, seed=0, **kw)
    pipe.scheduler = EulerAncestralDiscreteScheduler(**(factory.SDXL_EULER_A_SCHEDULER if kind == "sdxl" else factory.SD15_EULER_A_SCHEDULER))
    return pipe


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_text_to_image_noise_rows_follow_the_initial_latents_in_the_generator_stream(kind):
    pipe, n, seed = _pipe(kind), 5, 1234
    out = pipe(num_inference_steps=n, guidance_scale=5.0, height=32, width=32, generator=torch.Generator().manual_seed(seed),
               **_embeds(kind)).images
    assert out.shape == (1, 4, 16, 16) and out.dtype == bf16 and torch.isfinite(out.float()).all()
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn((1, 4, 16, 16), generator=g, dtype=bf16)                    # the call's earlier draw: the initial latents
    table = pipe._noise_table
    assert table.shape == (n, 1, 4, 16, 16) and table.dtype == bf16
    rows = [torch.randn((1, 4, 16, 16), generator=g, dtype=bf16) for _ in range(n)]
    for i in range(n):
        assert torch.equal(table[i], rows[i]), i
    # scheduler.step(generator=...) called n times consumes the same stream: the loop written with step() gives the same latents
    sch = EulerAncestralDiscreteScheduler.from_config(pipe.scheduler.config)
    sch.set_timesteps(n, device="cpu")
    g = torch.Generator().manual_seed(seed)
    torch.randn((1, 4, 16, 16), generator=g, dtype=bf16)
    x = torch.zeros(1, 4, 16, 16, dtype=bf16)
    seen = []
    orig = ops.euler_ancestral_step
    try:
        ops.euler_ancestral_step = lambda eps, x_, noise, *a, **k: seen.append((noise.clone(), k["noise_step_stride"])) or orig(eps, x_, noise, *a, **k)
        for t in sch.timesteps:
            x = sch.step(torch.zeros_like(x), t, x, generator=g).prev_sample
    finally:
        ops.euler_ancestral_step = orig
    assert len(seen) == n and all(st == 0 for _, st in seen)
    for i in range(n):
        assert torch.equal(seen[i][0], rows[i]), i
    # a second call of the same shape refills the table in place (captured graphs keep its address) with the new seed's draws
    ptr = table.data_ptr()
    pipe(num_inference_steps=n, guidance_scale=5.0, height=32, width=32, generator=torch.Generator().manual_seed(seed + 1), **_embeds(kind))
    assert pipe._noise_table.data_ptr() == ptr and not torch.equal(pipe._noise_table[0], rows[0])
    assert torch.equal(pipe(num_inference_steps=n, guidance_scale=5.0, height=32, width=32,
                            generator=torch.Generator().manual_seed(seed), **_embeds(kind)).images, out)


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_img2img_noise_rows_follow_both_earlier_draws_and_sit_in_the_rows_that_run(kind):
    pipe, n, seed = _pipe(kind, img2img=True), 8, 77
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    out = pipe(image=img, strength=0.5, num_inference_steps=n, guidance_scale=5.0, generator=torch.Generator().manual_seed(seed),
               **_embeds(kind)).images
    assert torch.isfinite(out.float()).all() and pipe.scheduler.step_index == n
    g = torch.Generator().manual_seed(seed)
    ndt = torch.float32 if (kind == "sdxl" and pipe.vae.config.force_upcast) else bf16
    torch.randn((1, 4, 16, 16), generator=g, dtype=ndt)                            # (1) the VAE posterior sample
    torch.randn((1, 4, 16, 16), generator=g, dtype=bf16)                           # (2) the img2img noise
    table = pipe._noise_table
    assert table.shape == (n, 1, 4, 16, 16)
    assert float(table[:4].float().abs().max()) == 0.0                             # rows before `begin` are never read
    for i in range(4, n):
        assert torch.equal(table[i], torch.randn((1, 4, 16, 16), generator=g, dtype=bf16)), i


def test_inpaint_and_the_other_loop_options_run_on_the_stand_ins():
    pipe = _pipe("sd15", inpaint=True, unet_in_channels=4)
    g = torch.Generator().manual_seed(3)
    img = torch.rand(1, 3, 32, 32, generator=g)
    out = pipe(image=img, mask_image=torch.zeros(32, 32), strength=0.5, num_inference_steps=10, generator=torch.Generator().manual_seed(5),
               **_embeds("sd15")).images
    assert torch.equal(out, pipe._inpaint["image_latents"])                        # mask == 0: the last blend row un-noises
    pipe = _pipe("sdxl", inpaint=True, unet_in_channels=9)
    out = pipe(image=img, mask_image=torch.ones(32, 32), strength=0.6, num_inference_steps=5, generator=torch.Generator().manual_seed(5),
               **_embeds("sdxl")).images
    assert torch.isfinite(out.float()).all() and pipe._noise_table.shape[0] == 5
    pipe = _pipe("sdxl")
    base = pipe(num_inference_steps=4, guidance_scale=5.0, height=32, width=32, generator=torch.Generator().manual_seed(1), **_embeds("sdxl")).images
    for kw in (dict(guidance_scale=1.0), dict(guidance_scale=5.0, guidance_rescale=0.7)):
        o = pipe(num_inference_steps=4, height=32, width=32, generator=torch.Generator().manual_seed(1), **kw, **_embeds("sdxl")).images
        assert torch.isfinite(o.float()).all() and not torch.equal(o, base)
    seen = []
    pipe(num_inference_steps=10, guidance_scale=5.0, height=32, width=32, denoising_end=0.5, generator=torch.Generator().manual_seed(1),
         callback_on_step_end=lambda p, i, t, d: seen.append(i) or {}, **_embeds("sdxl"))
    assert 0 < len(seen) < 10 and pipe._noise_table.shape[0] == 10
    # Turbo style: trailing, one step, no guidance
    pipe.scheduler = EulerAncestralDiscreteScheduler.from_config(pipe.scheduler.config, timestep_spacing="trailing")
    o = pipe(num_inference_steps=1, guidance_scale=0.0, height=32, width=32, generator=torch.Generator().manual_seed(1), **_embeds("sdxl")).images
    assert torch.isfinite(o.float()).all() and pipe.scheduler.timesteps.tolist() == [999.0]
    # DDIM's eta keeps its own table, and a deterministic sampler has none
    pipe = _pipe("sd15")
    pipe.scheduler = DDIMScheduler(**factory.SD15_SCHEDULER)
    pipe(num_inference_steps=3, height=32, width=32, eta=0.5, generator=torch.Generator().manual_seed(1), **_embeds("sd15"))
    assert pipe._noise_table is not None and pipe._noise_table.shape[0] == 3
    pipe(num_inference_steps=3, height=32, width=32, generator=torch.Generator().manual_seed(1), **_embeds("sd15"))
    assert pipe._noise_table is None


# ----------------------------------------------------------------------------------------------------------------------
# from_config, loading
# ----------------------------------------------------------------------------------------------------------------------
def test_from_config_of_other_schedulers_and_of_a_reference_config_file(tmp_path):
    eul = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    a = EulerAncestralDiscreteScheduler.from_config(eul.config)
    assert (a.config.beta_schedule, a.config.beta_start, a.config.beta_end) == ("scaled_linear", 0.00085, 0.012)
    assert a.config.timestep_spacing == "leading" and a.config.steps_offset == 1 and "interpolation_type" not in a.config
    assert a.config == EulerAncestralDiscreteScheduler(**factory.SDXL_EULER_A_SCHEDULER).config
    d = DPMSolverMultistepScheduler(**factory.SD15_DPM_SCHEDULER)
    a = EulerAncestralDiscreteScheduler.from_config(d.config, timestep_spacing="trailing")
    assert "use_karras_sigmas" not in a.config and a.config.timestep_spacing == "trailing" and a.config.beta_end == 0.012
    assert EulerDiscreteScheduler.from_config(a.config).config.timestep_spacing == "trailing"
    ref_cfg = dict(_class_name="EulerAncestralDiscreteScheduler", _diffusers_version="0.40.0", num_train_timesteps=1000,
                   beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None, prediction_type="epsilon",
                   timestep_spacing="trailing", steps_offset=1, rescale_betas_zero_snr=False)
    f = tmp_path / "scheduler_config.json"
    f.write_text(json.dumps(ref_cfg))
    a = EulerAncestralDiscreteScheduler.from_config(json.loads(f.read_text()))
    assert set(ref_cfg) - {"_class_name", "_diffusers_version"} == set(a.config) == set(EulerAncestralDiscreteScheduler._defaults)
    assert a.needs_step_noise is True and not getattr(eul, "needs_step_noise", False)
    import diffusers_amd
    assert diffusers_amd.EulerAncestralDiscreteScheduler is EulerAncestralDiscreteScheduler
    assert factory.SD15_EULER_A_SCHEDULER["steps_offset"] == 1
    with pytest.raises(TypeError, match="unexpected config keys"):
        EulerAncestralDiscreteScheduler(use_karras_sigmas=True)


def _sdxl_dir(tmp_path):
    from diffusers_amd import init as dinit, loading
    from diffusers_amd.autoencoder_kl import AutoencoderKL
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    root = tmp_path / "pipe"
    usd = dinit.random_state_dict(dinit.unet_param_shapes(UNet2DConditionModel(**dinit.TINY_SDXL_UNET).config), seed=0)
    loading.save_reference_checkpoint(usd, dict(dinit.TINY_SDXL_UNET, _class_name="UNet2DConditionModel"), root / "unet")
    vsd = dinit.random_state_dict(dinit.vae_decoder_param_shapes(AutoencoderKL(**dinit.TINY_VAE).config), seed=1)
    loading.save_reference_checkpoint(vsd, dict(dinit.TINY_VAE, _class_name="AutoencoderKL"), root / "vae")
    (root / "scheduler").mkdir(parents=True)
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(
        factory.SDXL_EULER_A_SCHEDULER, _class_name="EulerAncestralDiscreteScheduler", _diffusers_version="0.40.0",
        timestep_spacing="trailing", prediction_type="epsilon")))
    index = {"_class_name": "StableDiffusionXLPipeline", "_diffusers_version": "0.40.0", "force_zeros_for_empty_prompt": True,
             "unet": ["diffusers", "UNet2DConditionModel"], "vae": ["diffusers", "AutoencoderKL"],
             "scheduler": ["diffusers", "EulerAncestralDiscreteScheduler"], "text_encoder": [None, None],
             "text_encoder_2": [None, None], "tokenizer": [None, None], "tokenizer_2": [None, None]}
    (root / "model_index.json").write_text(json.dumps(index))
    return root


def test_pipeline_directory_that_names_the_scheduler_loads_and_runs(tmp_path):
    from diffusers_amd.pipelines import StableDiffusionXLPipeline
    pipe = StableDiffusionXLPipeline.from_pretrained(_sdxl_dir(tmp_path), device="cpu")
    sch = pipe.scheduler
    assert type(sch) is EulerAncestralDiscreteScheduler and sch.config.timestep_spacing == "trailing" and sch.config.steps_offset == 1
    seen = []
    out = pipe(num_inference_steps=4, guidance_scale=0.0, height=32, width=32, generator=torch.Generator().manual_seed(2),
               callback_on_step_end=lambda p, i, t, d: seen.append((i, float(t))) or {}, **_embeds("sdxl")).images
    assert out.shape == (1, 4, 16, 16) and torch.isfinite(out.float()).all()
    assert [i for i, _ in seen] == [0, 1, 2, 3] and [t for _, t in seen] == [999.0, 749.0, 499.0, 249.0] and sch.step_index == 4
    with pytest.raises(NotImplementedError, match="EulerAncestralDiscrete"):
        StableDiffusionXLPipeline._load_component(tmp_path, "scheduler", "diffusers", "PNDMScheduler", "cpu", None, "none", False)


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    with pytest.raises(NotImplementedError, match="prediction_type not implemented yet: sample"):
        _sched(prediction_type="sample")
    with pytest.raises(ValueError, match="must be one of"):
        _sched(prediction_type="flow_prediction")
    with pytest.raises(NotImplementedError, match="zero-SNR"):
        _sched(rescale_betas_zero_snr=True)
    with pytest.raises(ValueError, match="is not supported"):
        _sched(5, timestep_spacing="middle")
    s = _sched()
    x = torch.zeros(1, 4, 2, 2)
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(x, s.timesteps[0], x)
    s = _sched(4)
    for t in (3, torch.tensor(3), torch.tensor(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="integer indices"):
            s.step(x, t, x)
    with pytest.raises(ValueError, match="noise_table"):
        s.step_cfg(torch.zeros(2, 4, 2, 2), x, 5.0, out=x)
    with pytest.raises(ValueError, match="rows"):
        s.step_cfg(torch.zeros(2, 4, 2, 2), x, 5.0, out=x, noise_table=torch.zeros(3, 1, 4, 2, 2))
    with pytest.raises(TypeError):
        s.set_timesteps(timesteps=[900, 500, 100], device="cpu")


@pytest.mark.parametrize("kind,flavour", [(k, f) for k in ("sdxl", "sd15") for f in ("t2i", "img2img", "inpaint") if (k, f) != ("sd15", "t2i")])
def test_custom_schedules_stay_refused_through_the_pipelines(kind, flavour):
    pipe = _pipe(kind, **({} if flavour == "t2i" else {flavour: True}))
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    kw = dict(_embeds(kind), num_inference_steps=4)
    if flavour == "t2i":
        kw.update(height=32, width=32)
    else:
        kw.update(image=img, strength=0.5)
    if flavour == "inpaint":
        kw.update(mask_image=torch.ones(32, 32))
    for sched in (dict(timesteps=[900, 500, 100]), dict(sigmas=[10.0, 1.0, 0.0])):
        with pytest.raises(ValueError, match="does not support custom timestep or sigma schedules"):
            pipe(**kw, **sched)


def test_add_noise_and_begin_index_follow_the_euler_rules():
    s = _sched(10, timestep_spacing="leading", steps_offset=1)
    e = EulerDiscreteScheduler(**SD_BETAS, timestep_spacing="leading", steps_offset=1)
    e.set_timesteps(10, device="cpu")
    for sch in (s, e):
        sch.set_begin_index(3)
    assert int(s.device_step) == 3 and s.step_index is None
    assert s._add_noise_coeffs(s.timesteps[7:8].repeat(2), bf16) == e._add_noise_coeffs(e.timesteps[7:8].repeat(2), bf16) \
        == ([1.0, 1.0], [float(s.sigmas.to(bf16)[3])] * 2)
    s.set_timesteps(10, device="cpu")
    assert s._add_noise_coeffs(s.timesteps[7:8], bf16) == ([1.0], [float(s.sigmas.to(bf16)[7])])
    t = s.add_noise_table(bf16)
    assert tuple(t.shape) == (11, 2) and t[10].tolist() == [1.0, 0.0] and float(t[4, 1]) == float(s.sigmas.to(bf16)[4])
    table, step = s.device_table, s.device_step
    s.reset(6)
    assert int(step) == 6 and s.step_index == 6
    s.set_timesteps(10, device="cpu")
    assert s.device_table.data_ptr() == table.data_ptr() and s.device_step.data_ptr() == step.data_ptr() and int(step) == 0


# ----------------------------------------------------------------------------------------------------------------------
# ABI
# ----------------------------------------------------------------------------------------------------------------------
def test_abi_tables_carry_the_new_entry_point():
    name = "da_euler_ancestral_step"
    assert L.FN_IDS[name] == L.FN_COUNT - 2 and L.FN_IDS["da_dpmpp_2m_step"] == L.FN_COUNT - 1
    assert L.SIGNATURES[name] == L.SIGNATURES["da_x0_linear_step"]            # same argument list (noise + stride)
    lib = L.load()
    assert lib.da_version() == L.ABI_VERSION == 9
    assert lib.da_plan_arg_kinds(L.FN_IDS[name]).decode() == "ppplpppiflii"
    assert lib.da_plan_arg_count(L.FN_IDS[name]) == len(L.SIGNATURES[name][1]) - 1
    # host-side argument checks (no launch happens for a refused call): null pointers, n <= 0, a pred_type outside {0, 1}
    assert lib.da_euler_ancestral_step(None, None, None, 0, None, None, None, 0, 0.0, 16, 0, 0, None) == 1
    one = 1 << 12       # any non-null value: a refused call dereferences nothing
    assert lib.da_euler_ancestral_step(one, one, None, 0, one, one, one, 0, 0.0, 16, 0, 0, None) == 1      # the noise is required
    assert lib.da_euler_ancestral_step(one, one, one, 0, one, one, one, 0, 0.0, 0, 0, 0, None) == 1
    assert lib.da_euler_ancestral_step(one, one, one, 0, one, one, one, 0, 0.0, 16, 0, 2, None) == 1
    assert lib.da_euler_ancestral_step(one, one, one, -1, one, one, one, 0, 0.0, 16, 0, 0, None) == 1
    import diffusers_amd.torch_ops as T
    assert "euler_ancestral_step" in T.OPS and not torch.ops.mi355x.euler_ancestral_step.default._schema.is_mutable
