"""LCMScheduler, the U-Net's ``timestep_cond`` and the pipelines' guidance-scale embedding, host side -- no kernel runs here.

The reference's arithmetic is restated in tests/lcm_emulation.py (schedule, table rows, the step's op chain); its ``x0_linear_step`` is
the CPU stand-in monkeypatched over ``ops.x0_linear_step`` and the expected value of the kernel in tests/test_lcm_gpu.py."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from diffusers_amd import _lib as L
from diffusers_amd import factory, ops
from diffusers_amd.schedulers import DDIMScheduler, EulerDiscreteScheduler, LCMScheduler, LCMSchedulerOutput

import inpaint_emulation
import lcm_emulation as E

bf16 = torch.bfloat16
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(autouse=True)
def _emulated_kernels(monkeypatch):
    inpaint_emulation.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "x0_linear_step", E.x0_linear_step)
    monkeypatch.setattr(ops, "TUNING", False)


def _sched(n=None, set_kw=None, **kw):
    s = LCMScheduler(**kw)
    if n is not None or set_kw:
        s.set_timesteps(n, device="cpu", **(set_kw or {}))
    return s


# ----------------------------------------------------------------------------------------------------------------------
# schedules
# ----------------------------------------------------------------------------------------------------------------------
KNOWN = [
    (4, {}, [999, 759, 499, 259]),
    (8, {}, [999, 879, 759, 639, 499, 379, 259, 139]),
    (1, {}, [999]),
    (6, {}, [999, 839, 679, 499, 339, 179]),
    (4, dict(strength=0.5), [499, 379, 259, 139]),
    (2, dict(strength=0.3), [299, 159]),
    (3, dict(original_inference_steps=20), [999, 699, 349]),
    (50, {}, list(range(999, 0, -20))),
]


@pytest.mark.parametrize("n,kw,want", KNOWN, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in kw.items()) or 'plain'}" for n, kw, _ in KNOWN])
def test_known_schedules(n, kw, want):
    s = _sched(n, set_kw=kw)
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == want
    assert E.ref_schedule(n, **kw).tolist() == want
    assert s.num_inference_steps == n and s.order == 1 and s.init_noise_sigma == 1.0 and s.needs_step_noise is True
    assert s.step_index is None and s.begin_index is None and int(s.device_step) == 0
    assert s.device_table.dtype == torch.float32 and s.device_table.shape[1] == 8 and s.device_table.shape[0] >= n


def test_defaults_are_the_references():
    assert LCMScheduler._defaults == dict(
        num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None,
        original_inference_steps=50, clip_sample=False, clip_sample_range=1.0, set_alpha_to_one=True, steps_offset=0,
        prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
        timestep_spacing="leading", timestep_scaling=10.0, rescale_betas_zero_snr=False)


def test_custom_timesteps_and_refusals():
    s = _sched(set_kw=dict(timesteps=[999, 600, 300, 20]))
    assert s.timesteps.tolist() == [999, 600, 300, 20] and s.num_inference_steps == 4 and s.custom_timesteps is True
    s = _sched()
    for bad, n in ((dict(timesteps=[999, 500]), 2),                      # both
                   (dict(timesteps=[500, 600, 100]), None),              # not descending
                   (dict(timesteps=[500, 500, 100]), None),              # not strictly
                   (dict(timesteps=[1000, 500]), None),                  # starts at num_train_timesteps
                   ({}, None),                                           # neither
                   ({}, 51),                                             # n > original steps
                   (dict(strength=0.1), 6),                              # len(origin) // n < 1: 5 origin steps
                   (dict(original_inference_steps=1001), 4),
                   ({}, 1001)):
        with pytest.raises(ValueError):
            s.set_timesteps(n, device="cpu", **bad)
    with pytest.raises(NotImplementedError, match="thresholding"):
        LCMScheduler(thresholding=True)
    with pytest.raises(NotImplementedError, match="zero-SNR"):
        LCMScheduler(rescale_betas_zero_snr=True)
    with pytest.raises(ValueError, match="prediction_type"):
        LCMScheduler(prediction_type="flow_prediction")
    with pytest.raises(TypeError, match="unexpected config keys"):
        LCMScheduler(use_karras_sigmas=True)
    x = torch.zeros(1, 4, 2, 2, dtype=bf16)
    with pytest.raises(ValueError, match="set_timesteps"):
        LCMScheduler().step(x, 999, x)
    s = _sched(4)
    with pytest.raises(ValueError, match="noise_table"):
        s.step_cfg(torch.zeros(2, 4, 2, 2, dtype=bf16), x, 1.5, out=x)
    with pytest.raises(ValueError, match="rows"):
        s.step_cfg(torch.zeros(2, 4, 2, 2, dtype=bf16), x, 1.5, out=x, noise_table=torch.zeros(3, 1, 4, 2, 2, dtype=bf16))
    for _ in range(4):
        s.step(x, s.timesteps[s.step_index or 0], x)
    with pytest.raises(IndexError):                                       # a step past the schedule would read a row that is not there
        s.step(x, s.timesteps[-1], x)


# ----------------------------------------------------------------------------------------------------------------------
# table rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, dict(timestep_scaling=1e-3), dict(clip_sample=True, clip_sample_range=2.5),
                                dict(beta_schedule="linear", beta_start=1e-4, beta_end=0.02)], ids=["default", "scaling1e-3", "clip", "linear"])
def test_table_rows_equal_the_restated_scalars(kw):
    for n in (1, 4, 8):
        s = _sched(n, **kw)
        ac = E.ref_alphas_cumprod(**{k: v for k, v in kw.items() if k.startswith("beta")})
        assert torch.equal(s.alphas_cumprod, ac)
        want = E.ref_rows(ac, s.timesteps.tolist(), kw.get("timestep_scaling", 10.0), kw.get("clip_sample_range", 0.0))
        rows = s.device_table[:n]
        assert torch.equal(rows, want), (n, kw)
        assert rows[-1, 4:6].tolist() == [1.0, 0.0] and (rows[:-1, 5] > 0).all()
        # the rows behind them: the same steps without the re-noising (what the eager step() reads `denoised` from)
        den = want.clone()
        den[:, 4], den[:, 5] = 1.0, 0.0
        assert torch.equal(s.device_table[n:], den)


def test_spot_values():
    s = _sched(4)
    assert float(s.alphas_cumprod[999]) == pytest.approx(0.0046601, rel=1e-4)
    assert float(s.alphas_cumprod[259]) == pytest.approx(0.6589752, rel=1e-5)
    r = s.device_table
    assert float(r[0, 3]) == pytest.approx(2.505e-9, rel=1e-3) and float(r[0, 2]) == 1.0 and float(r[0, 7]) == 999.0
    assert float(r[0, 0]) == pytest.approx((1 - 0.0046601) ** 0.5, rel=1e-5) and float(r[0, 1]) == pytest.approx(0.0046601 ** 0.5, rel=1e-4)
    assert float(r[2, 4]) == pytest.approx(0.6589752 ** 0.5, rel=1e-5) and float(r[2, 5]) == pytest.approx((1 - 0.6589752) ** 0.5, rel=1e-5)
    s = _sched(4, timestep_scaling=1e-3)                                  # t = 499: both terms of `denoised` matter
    assert float(r[2, 7]) == 499.0
    assert float(s.device_table[2, 3]) == pytest.approx(0.25 / (0.499 ** 2 + 0.25), rel=1e-5) == pytest.approx(0.50, abs=0.01)
    assert float(s.device_table[2, 2]) == pytest.approx(0.499 / (0.499 ** 2 + 0.25) ** 0.5, rel=1e-5) == pytest.approx(0.706, abs=0.001)


# ----------------------------------------------------------------------------------------------------------------------
# step
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("dtype", [bf16, torch.float32], ids=["bf16", "f32"])
def test_step_equals_the_restated_chain_and_draws_like_the_reference(pred, dtype):
    n = 4
    s = _sched(n, prediction_type=pred, timestep_scaling=1e-3, clip_sample=True, clip_sample_range=3.0)
    rows = E.ref_rows(s.alphas_cumprod, s.timesteps.tolist(), 1e-3, 3.0)
    g0 = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 8, 8, generator=g0).to(dtype)
    gen, twin = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    for i, t in enumerate(s.timesteps):
        e = torch.randn(1, 4, 8, 8, generator=g0).to(dtype)
        out = s.step(e, t, x, generator=gen)
        assert isinstance(out, LCMSchedulerOutput) and s.step_index == i + 1 and int(s.device_step) == i + 1
        den_row = rows[i].clone()
        den_row[4], den_row[5] = 1.0, 0.0
        den = E.ref_step_row(e, x, None, den_row, pred_type=L.PRED_LCM + L.PRED_TYPES[pred])
        assert torch.equal(out.denoised, den)
        if i == n - 1:
            assert torch.equal(out.prev_sample, den)                      # the last step returns `denoised`, draws nothing
        else:
            noise = torch.randn(x.shape, generator=twin, dtype=dtype)
            want = E.ref_step_row(e, x, noise, rows[i], pred_type=L.PRED_LCM + L.PRED_TYPES[pred])
            assert torch.equal(out.prev_sample, want) and not torch.equal(want, den)
        x = out.prev_sample
    assert torch.equal(gen.get_state(), twin.get_state())                 # advanced by exactly n - 1 draws
    s.set_timesteps(n, device="cpu")
    tup = s.step(e, s.timesteps[0], x, generator=gen, return_dict=False)
    assert isinstance(tup, tuple) and len(tup) == 2 and tup[0].shape == x.shape and tup[1].shape == x.shape
    assert not torch.equal(tup[0], tup[1])


def test_step_cfg_reads_the_row_of_the_step_counter_and_combines():
    n, numel = 4, 4 * 6 * 6
    s = _sched(n)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, 6, 6, generator=g).to(bf16)
    e2 = torch.randn(2, 4, 6, 6, generator=g).to(bf16)
    table = torch.randn(n, 1, 4, 6, 6, generator=g).to(bf16)
    table[n - 1] = float("nan")                                            # never read
    rows = s.device_table[:n]
    s.set_begin_index(1)
    for i in range(1, n):
        want = E.ref_step_row(e2, x, table[i], rows[i], cfg=True, guidance=1.5)
        got = s.step_cfg(e2, x.clone(), 1.5, noise_table=table)
        assert torch.equal(got, want) and torch.isfinite(got.float()).all(), i
        buf = x.clone()
        s.reset(i)
        assert s.step_cfg(e2[1:].contiguous(), buf, 1.5, out=buf, cfg=False, noise_table=table) is buf
        assert torch.equal(buf, E.ref_step_row(e2[1], x, table[i], rows[i])), i
    assert s.step_noise_draws(0, 4) == 3 and s.step_noise_draws(2, 2) == 1 and s.step_noise_draws(0, 2) == 2
    assert s.step_noise_draws(3, 1) == 0 and _sched(1).step_noise_draws(0, 1) == 0
    assert s.graph_token()[2] == L.PRED_LCM and _sched(prediction_type="v_prediction").graph_token()[2] == 5


def test_from_config_add_noise_and_export():
    import diffusers_amd
    assert diffusers_amd.LCMScheduler is LCMScheduler and "LCMScheduler" in diffusers_amd.__all__
    for src in (DDIMScheduler(**factory.SD15_SCHEDULER), EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)):
        s = LCMScheduler.from_config(src.config)
        assert (s.config.beta_schedule, s.config.beta_start, s.config.beta_end) == ("scaled_linear", 0.00085, 0.012)
        assert s.config.steps_offset == 1 and s.config.original_inference_steps == 50 and s.config.timestep_scaling == 10.0
        assert set(s.config) == set(LCMScheduler._defaults)
        back = type(src).from_config(s.config)
        assert back.config.beta_end == 0.012 and set(back.config) == set(type(src)._defaults)
    s = LCMScheduler.from_config(dict(factory.LCM_SCHEDULER, _class_name="LCMScheduler", _diffusers_version="0.40.0"), timestep_scaling=5.0)
    assert s.config.timestep_scaling == 5.0
    s.set_timesteps(4, device="cpu")
    d = DDIMScheduler(**E.SD_BETAS)
    d.set_timesteps(4, device="cpu")
    assert s._add_noise_coeffs(torch.tensor([499, 259]), bf16) == d._add_noise_coeffs(torch.tensor([499, 259]), bf16)
    t = s.add_noise_table(bf16)
    assert tuple(t.shape) == (5, 2) and t[4].tolist() == [1.0, 0.0]
    table, step = s.device_table, s.device_step
    s.set_begin_index(2)
    assert int(step) == 2
    s.set_timesteps(4, device="cpu")
    assert s.device_table.data_ptr() == table.data_ptr() and s.device_step.data_ptr() == step.data_ptr() and int(step) == 0


# ----------------------------------------------------------------------------------------------------------------------
# guidance-scale embedding
# ----------------------------------------------------------------------------------------------------------------------
def test_guidance_scale_embedding():
    from diffusers_amd.pipelines import get_guidance_scale_embedding
    e = get_guidance_scale_embedding(torch.tensor([7.5, 7.5]), embedding_dim=256)
    assert e.shape == (2, 256) and e.dtype == torch.float32 and torch.equal(e[0], e[1])
    for col, want in ((0, -0.851236), (1, 0.842131), (127, 0.681639), (128, -0.524783), (255, 0.731689)):
        assert float(e[0, col]) == pytest.approx(want, abs=2e-4), col
    # restated in float64: sin / cos of 1000 w at log-spaced frequencies
    f = np.exp(np.arange(128) * -(np.log(10000.0) / 127))
    want = np.concatenate([np.sin(7500.0 * f), np.cos(7500.0 * f)])
    assert np.abs(e[0].double().numpy() - want).max() < 2e-3             # (fp32 arguments of ~7500 rad: ~ 7500 x 2^-24 x a few ops)
    odd = get_guidance_scale_embedding(torch.tensor([0.5]), embedding_dim=33)
    assert odd.shape == (1, 33) and float(odd[0, 32]) == 0.0 and float(odd[0, 16]) != 0.0
    assert get_guidance_scale_embedding(torch.tensor([0.5]), 512).shape == (1, 512)
    with pytest.raises(ValueError):
        get_guidance_scale_embedding(torch.zeros(1, 1))


# ----------------------------------------------------------------------------------------------------------------------
# U-Net: time_cond_proj_dim / timestep_cond
# ----------------------------------------------------------------------------------------------------------------------
def _unet_inputs(kind, B=2):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 4, 16, 16, generator=g).to(bf16)
    ehs = torch.randn(B, 7, 64, generator=g).to(bf16)
    added = None
    if kind == "sdxl":
        added = {"text_embeds": torch.randn(B, 64, generator=g).to(bf16), "time_ids": torch.tensor([[32., 32, 0, 0, 32, 32]]).repeat(B, 1)}
    return x, ehs, added


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_unet_timestep_cond_host_logic(kind):
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    cfg, sd, tc = E.cond_unet_case(kind)
    x, ehs, added = _unet_inputs(kind)
    unet = UNet2DConditionModel(**cfg).load_state_dict(sd, device="cpu")
    assert unet.config.time_cond_proj_dim == E.COND_DIM and tuple(unet.time_cond_proj.shape) == (64, E.COND_DIM)
    out = unet(x, 499.0, ehs, timestep_cond=tc, added_cond_kwargs=added, return_dict=False)[0]
    assert torch.isfinite(out.float()).all()
    for bad in (None, tc[:1], tc[:, :16].contiguous(), tc.reshape(-1), torch.zeros(2, 8, dtype=bf16)):
        with pytest.raises(ValueError, match="timestep_cond"):
            unet(x, 499.0, ehs, timestep_cond=bad, added_cond_kwargs=added)
    # through precompute_conditioning: a static bf16 buffer of its own, and the same output
    cond = unet.precompute_conditioning(ehs, added, timestep_cond=tc.float())
    assert cond["timestep_cond"].dtype == bf16 and cond["timestep_cond"].data_ptr() != tc.data_ptr()
    assert torch.equal(unet(x, 499.0, None, conditioning=cond, return_dict=False)[0], out)
    with pytest.raises(ValueError, match="precompute_conditioning"):
        unet(x, 499.0, None, conditioning=cond, timestep_cond=tc)
    with pytest.raises(ValueError, match="timestep_cond"):
        unet(x, 499.0, None, conditioning={k: v for k, v in cond.items() if k != "timestep_cond"})
    # the drop-in cache keys on the embedding too
    other = (tc.float() * 0.5).to(bf16)
    assert not torch.equal(unet(x, 499.0, ehs, timestep_cond=other, added_cond_kwargs=added, return_dict=False)[0], out)
    assert torch.equal(unet(x, 499.0, ehs, timestep_cond=tc, added_cond_kwargs=added, return_dict=False)[0], out)
    # a zero cond_proj: bit-identical to the same weights without the key
    plain_sd = {k: v for k, v in sd.items() if k != "time_embedding.cond_proj.weight"}
    plain = UNet2DConditionModel(**{k: v for k, v in cfg.items() if k != "time_cond_proj_dim"}).load_state_dict(plain_sd, device="cpu")
    zero = UNet2DConditionModel(**cfg).load_state_dict(dict(sd, **{"time_embedding.cond_proj.weight": torch.zeros(64, E.COND_DIM, dtype=bf16)}),
                                                       device="cpu")
    base = plain(x, 499.0, ehs, added_cond_kwargs=added, return_dict=False)[0]
    assert torch.equal(zero(x, 499.0, ehs, timestep_cond=tc, added_cond_kwargs=added, return_dict=False)[0], base)
    assert not torch.equal(out, base)
    with pytest.raises(ValueError, match="timestep_cond"):               # unchanged: a U-Net without the key refuses the argument
        plain(x, 499.0, ehs, timestep_cond=tc, added_cond_kwargs=added)
    with pytest.raises(ValueError, match="timestep_cond"):
        plain.precompute_conditioning(ehs, added, timestep_cond=tc)
    with pytest.raises(KeyError, match="cond_proj"):
        UNet2DConditionModel(**cfg).load_state_dict(plain_sd, device="cpu")
    with pytest.raises(ValueError, match="shape"):
        UNet2DConditionModel(**cfg).load_state_dict(dict(sd, **{"time_embedding.cond_proj.weight": torch.zeros(64, 16, dtype=bf16)}), device="cpu")
    for bad in (0, -8, 12, True, 2.5):
        with pytest.raises(ValueError, match="time_cond_proj_dim"):
            UNet2DConditionModel(**dict(cfg, time_cond_proj_dim=bad))


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_cond_proj_moves_the_oracle_output_and_the_engine_follows(kind):
    """The seeded cond_proj (lcm_emulation.COND_PROJ_GAIN) changes the fp32 oracle's output by rel-RMS >= 0.25, so the device test's
    2.5e-2 gate against the oracle cannot pass with the term missing; on the stand-in ops the engine's host logic follows the oracle."""
    from oracle import reference_math as R
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    cfg, sd, tc = E.cond_unet_case(kind)
    full = dict(UNet2DConditionModel(**cfg).config)
    x, ehs, added = _unet_inputs(kind)
    f32 = lambda d: None if d is None else {k: v.float() for k, v in d.items()}     # noqa: E731
    with_term = R.unet_forward(E.oracle_state_dict(sd, tc), full, x.float(), 499.0, ehs.float(), f32(added))
    without = R.unet_forward({k: v.float() for k, v in sd.items()}, full, x.float(), 499.0, ehs.float(), f32(added))
    rel = lambda a, b: float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())   # noqa: E731
    moved = rel(with_term, without)
    print(f"[cond_proj] tiny {kind}: oracle with vs without the term rel_rms {moved:.3f}")
    assert moved >= 0.25
    unet = UNet2DConditionModel(**cfg).load_state_dict(sd, device="cpu")
    got = unet(x, 499.0, ehs, timestep_cond=tc, added_cond_kwargs=added, return_dict=False)[0].float()
    assert rel(got, with_term) < 2.5e-2 < rel(got, without)


# ----------------------------------------------------------------------------------------------------------------------
# pipelines on the stand-ins
# ----------------------------------------------------------------------------------------------------------------------
def _embeds(kind, seed=3):
    g = torch.Generator().manual_seed(seed)
    d = dict(prompt_embeds=torch.randn((1, 7, 64), generator=g).to(bf16), negative_prompt_embeds=torch.randn((1, 7, 64), generator=g).to(bf16),
             output_type="latent", use_graph=False)
    if kind == "sdxl":
        d.update(pooled_prompt_embeds=torch.randn((1, 64), generator=g).to(bf16),
                 negative_pooled_prompt_embeds=torch.randn((1, 64), generator=g).to(bf16))
    return d


def _pipe(kind, **kw):
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    return build(device="cpu", tiny=True, seed=0, scheduler="lcm", **kw)


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
@pytest.mark.parametrize("gs", [1.0, 1.5], ids=["no_cfg", "cfg"])
def test_text_to_image_draws_and_result_equal_a_reference_ordered_loop(kind, gs):
    pipe, n, seed = _pipe(kind), 4, 1234
    assert type(pipe.scheduler) is LCMScheduler
    emb = _embeds(kind)
    gen = torch.Generator().manual_seed(seed)
    out = pipe(num_inference_steps=n, guidance_scale=gs, height=32, width=32, generator=gen, **emb).images
    assert out.shape == (1, 4, 16, 16) and out.dtype == bf16 and torch.isfinite(out.float()).all()
    assert pipe.scheduler.timesteps.tolist() == [999, 759, 499, 259] and pipe.scheduler.step_index == n
    # the reference's loop: prepare_latents, then per step the U-Net, the CFG combine and scheduler.step(generator=...)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, 4, 16, 16), generator=g, dtype=bf16)
    sch = LCMScheduler.from_config(pipe.scheduler.config)
    sch.set_timesteps(n, device="cpu")
    added = None
    cfg = gs > 1.0
    ehs = torch.cat([emb["negative_prompt_embeds"], emb["prompt_embeds"]]) if cfg else emb["prompt_embeds"]
    if kind == "sdxl":
        te = torch.cat([emb["negative_pooled_prompt_embeds"], emb["pooled_prompt_embeds"]]) if cfg else emb["pooled_prompt_embeds"]
        added = {"text_embeds": te, "time_ids": torch.tensor([[32., 32, 0, 0, 32, 32]]).repeat(te.shape[0], 1)}
    rows = []
    for i, t in enumerate(sch.timesteps):
        e = pipe.unet(torch.cat([x] * 2) if cfg else x, float(t), ehs, added_cond_kwargs=added, return_dict=False)[0]
        if cfg:
            e = e[:1] + gs * (e[1:] - e[:1])
        before = g.get_state()
        x = sch.step(e, t, x, generator=g).prev_sample
        if i < n - 1:
            twin = torch.Generator()
            twin.set_state(before)
            rows.append(torch.randn((1, 4, 16, 16), generator=twin, dtype=bf16))
        else:
            assert torch.equal(g.get_state(), before)
    table = pipe._noise_table
    assert table.shape == (n, 1, 4, 16, 16) and table.dtype == bf16
    for i in range(n - 1):
        assert torch.equal(table[i], rows[i]), i
    assert torch.equal(gen.get_state(), g.get_state())                    # the generator is left where the reference leaves it
    assert torch.equal(out, x)


def test_one_step_call_draws_nothing_and_still_has_a_table():
    pipe = _pipe("sdxl")
    gen = torch.Generator().manual_seed(7)
    out = pipe(num_inference_steps=1, guidance_scale=1.0, height=32, width=32, generator=gen, **_embeds("sdxl")).images
    g = torch.Generator().manual_seed(7)
    torch.randn((1, 4, 16, 16), generator=g, dtype=bf16)
    assert torch.equal(gen.get_state(), g.get_state()) and pipe._noise_table.shape == (1, 1, 4, 16, 16)
    assert torch.isfinite(out.float()).all() and pipe.scheduler.timesteps.tolist() == [999]


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_img2img_rows_sit_where_the_loop_runs_and_the_last_is_not_drawn(kind):
    pipe, n, seed = _pipe(kind, img2img=True), 4, 77
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    gen = torch.Generator().manual_seed(seed)
    seen = []
    out = pipe(image=img, strength=0.5, num_inference_steps=n, guidance_scale=1.5, generator=gen,
               callback_on_step_end=lambda p, i, t, d: seen.append(int(t)) or {}, **_embeds(kind)).images
    assert torch.isfinite(out.float()).all() and seen == [499, 259] and pipe.scheduler.step_index == n
    g = torch.Generator().manual_seed(seed)
    ndt = torch.float32 if (kind == "sdxl" and pipe.vae.config.force_upcast) else bf16
    torch.randn((1, 4, 16, 16), generator=g, dtype=ndt)                   # the VAE posterior sample
    torch.randn((1, 4, 16, 16), generator=g, dtype=bf16)                  # the img2img noise
    table = pipe._noise_table
    assert float(table[:2].float().abs().max()) == 0.0 and float(table[3].float().abs().max()) == 0.0
    assert torch.equal(table[2], torch.randn((1, 4, 16, 16), generator=g, dtype=bf16))
    assert torch.equal(gen.get_state(), g.get_state())


def test_schedule_arguments_pass_through_and_the_other_pipelines_run():
    pipe = _pipe("sdxl")
    seen = []
    cb = lambda p, i, t, d: seen.append(int(t)) or {}                     # noqa: E731
    kw = dict(guidance_scale=1.0, height=32, width=32, generator=torch.Generator().manual_seed(1), callback_on_step_end=cb)
    pipe(num_inference_steps=3, original_inference_steps=20, **kw, **_embeds("sdxl"))
    assert seen == [999, 699, 349]
    del seen[:]
    pipe(timesteps=[999, 600, 300], **kw, **_embeds("sdxl"))
    assert seen == [999, 600, 300] and pipe._noise_table.shape[0] == 3
    del seen[:]
    pipe(num_inference_steps=4, **kw, **_embeds("sdxl"))                    # (the option does not stick to the pipeline)
    assert seen == [999, 759, 499, 259]
    with pytest.raises(ValueError, match="does not support custom sigmas"):
        pipe(sigmas=[10.0, 1.0, 0.0], **kw, **_embeds("sdxl"))
    plain = factory.build_sdxl_pipeline(device="cpu", tiny=True, seed=0)
    with pytest.raises(ValueError, match="original_inference_steps"):
        plain(num_inference_steps=3, original_inference_steps=20, **kw, **_embeds("sdxl"))
    # inpainting (4-channel U-Net: the blend after every step) and ControlNet
    g = torch.Generator().manual_seed(3)
    img = torch.rand(1, 3, 32, 32, generator=g)
    ip = _pipe("sd15", inpaint=True, unet_in_channels=4)
    out = ip(image=img, mask_image=torch.zeros(32, 32), strength=0.5, num_inference_steps=4, guidance_scale=1.5,
             generator=torch.Generator().manual_seed(5), **_embeds("sd15")).images
    assert torch.equal(out, ip._inpaint["image_latents"])                  # mask == 0: the last blend row un-noises
    with pytest.raises(ValueError, match="scheduler must be"):
        factory.build_sdxl_pipeline(device="cpu", tiny=True, scheduler="tcd")


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_controlnet_pipelines_run_with_the_scheduler(kind, monkeypatch):
    import controlnet_emulation
    for name in ("conv2d_nhwc", "linear"):                                 # the gated zero convs of the residual hand-off
        monkeypatch.setattr(ops, name, getattr(controlnet_emulation, name))
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    cn = _pipe(kind, controlnet=True)
    gen = torch.Generator().manual_seed(5)
    o = cn(image=img, num_inference_steps=3, guidance_scale=1.5, generator=gen, **_embeds(kind)).images
    assert torch.isfinite(o.float()).all() and type(cn.scheduler) is LCMScheduler
    g = torch.Generator().manual_seed(5)
    torch.randn((1, 4, 16, 16), generator=g, dtype=bf16)
    rows = [torch.randn((1, 4, 16, 16), generator=g, dtype=bf16) for _ in range(2)]
    assert torch.equal(cn._noise_table[0], rows[0]) and torch.equal(cn._noise_table[1], rows[1])
    assert torch.equal(gen.get_state(), g.get_state())


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_a_cond_unet_turns_cfg_off_and_a_new_guidance_scale_refreshes_the_static_embedding(kind):
    from diffusers_amd.pipelines import get_guidance_scale_embedding
    pipe = _pipe(kind, time_cond_proj_dim=E.COND_DIM)
    assert pipe.unet.config.time_cond_proj_dim == E.COND_DIM
    emb = {k: v for k, v in _embeds(kind).items() if not k.startswith("negative")}      # no negative prompt is needed: no CFG batch
    batches = []
    fwd = pipe.unet.forward
    pipe.unet.forward = lambda sample, *a, **k: batches.append(sample.shape[0]) or fwd(sample, *a, **k)
    run = lambda gs: pipe(num_inference_steps=2, guidance_scale=gs, height=32, width=32, generator=torch.Generator().manual_seed(2),  # noqa: E731
                          **emb).images
    a = run(8.0)
    assert batches == [1, 1] and torch.isfinite(a.float()).all()
    assert pipe._arm(8.0, 0.0, None, None) is False
    # graph-key / refresh logic, as the captured loop applies it (tests/test_call_sequences_cpu.py does the same for the other inputs)
    lat = torch.zeros(1, 4, 16, 16, dtype=bf16)
    conds, keys = [], []
    for gs in (8.0, 4.0):
        pipe._arm(gs, 0.0, None, None)
        pe, added = pipe._conditioning_inputs(*([emb["prompt_embeds"], None] + ([emb["pooled_prompt_embeds"], None, torch.tensor([[32., 32, 0, 0, 32, 32]]),
                                                                                  None] if kind == "sdxl" else []) + [False]))
        cond = pipe._unet_conditioning(pe, added)
        want = get_guidance_scale_embedding(torch.tensor(gs - 1).repeat(1), embedding_dim=E.COND_DIM).to(bf16)
        assert torch.equal(cond["timestep_cond"], want)
        conds.append(cond)
        keys.append(pipe._make_graph_key(lat, cond, gs, False))
    assert keys[0] == keys[1]                                              # the scale is no by-value input of such a step ...
    assert not torch.equal(conds[0]["timestep_cond"], conds[1]["timestep_cond"])
    ptr = conds[0]["timestep_cond"].data_ptr()
    pipe._refresh_static((conds[0], 8.0, False), (conds[1], 4.0, False))   # ... it arrives through the static buffer
    assert conds[0]["timestep_cond"].data_ptr() == ptr and torch.equal(conds[0]["timestep_cond"], conds[1]["timestep_cond"])
    b = run(4.0)
    assert not torch.equal(a, b)
    # a U-Net without the key keeps the scale in the key
    plain = _pipe(kind)
    full = _embeds(kind)
    pe, added = plain._conditioning_inputs(*([full["prompt_embeds"], None] + ([full["pooled_prompt_embeds"], None, torch.tensor([[32., 32, 0, 0, 32, 32]]),
                                                                               None] if kind == "sdxl" else []) + [False]))
    cond = plain._unet_conditioning(pe, added)
    assert "timestep_cond" not in cond
    plain.scheduler.set_timesteps(2, device="cpu")
    assert plain._make_graph_key(lat, cond, 0.5, False) != plain._make_graph_key(lat, cond, 1.0, False)


def test_pipeline_directory_that_names_lcm_scheduler_loads(tmp_path):
    from diffusers_amd import init as dinit, loading
    from diffusers_amd.autoencoder_kl import AutoencoderKL
    from diffusers_amd.pipelines import StableDiffusionXLPipeline
    root = tmp_path / "pipe"
    cfg, usd, _ = E.cond_unet_case("sdxl")
    loading.save_reference_checkpoint(usd, dict(cfg, _class_name="UNet2DConditionModel"), root / "unet")
    vsd = dinit.random_state_dict(dinit.vae_decoder_param_shapes(AutoencoderKL(**dinit.TINY_VAE).config), seed=1)
    loading.save_reference_checkpoint(vsd, dict(dinit.TINY_VAE, _class_name="AutoencoderKL"), root / "vae")
    (root / "scheduler").mkdir(parents=True)
    (root / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(
        LCMScheduler._defaults, _class_name="LCMScheduler", _diffusers_version="0.40.0")))
    index = {"_class_name": "StableDiffusionXLPipeline", "_diffusers_version": "0.40.0", "force_zeros_for_empty_prompt": True,
             "unet": ["diffusers", "UNet2DConditionModel"], "vae": ["diffusers", "AutoencoderKL"],
             "scheduler": ["diffusers", "LCMScheduler"], "text_encoder": [None, None], "text_encoder_2": [None, None],
             "tokenizer": [None, None], "tokenizer_2": [None, None]}
    (root / "model_index.json").write_text(json.dumps(index))
    outs = []
    for _ in range(2):                                                    # the second load comes from the packed cache
        pipe = StableDiffusionXLPipeline.from_pretrained(root, device="cpu")
        assert type(pipe.scheduler) is LCMScheduler and pipe.scheduler.config.original_inference_steps == 50
        assert pipe.unet.config.time_cond_proj_dim == E.COND_DIM and tuple(pipe.unet.time_cond_proj.shape) == (64, E.COND_DIM)
        emb = {k: v for k, v in _embeds("sdxl").items() if not k.startswith("negative")}
        outs.append(pipe(num_inference_steps=2, guidance_scale=8.0, height=32, width=32, generator=torch.Generator().manual_seed(2), **emb).images)
    assert list((root / "unet" / "diffusers_amd_packed").glob("*.safetensors"))
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])
    with pytest.raises(NotImplementedError, match="LCM"):
        StableDiffusionXLPipeline._load_component(tmp_path, "scheduler", "diffusers", "TCDScheduler", "cpu", None, "none", False)


def test_fuse_lora_repacks_the_cond_proj_too():
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    cfg, sd, tc = E.cond_unet_case("sd15")
    # (on the CPU the packed tensor of an untouched weight IS the state dict's: pack a copy, so that `sd` stays the base)
    unet = UNet2DConditionModel(**cfg).load_state_dict({k_: v.clone() for k_, v in sd.items()}, device="cpu")
    w0 = unet.time_cond_proj.clone()
    g = torch.Generator().manual_seed(4)
    k = "time_embedding.cond_proj"
    lora = {f"{k}.lora_A.weight": torch.randn(4, E.COND_DIM, generator=g), f"{k}.lora_B.weight": torch.randn(64, 4, generator=g)}
    ptr = unet.time_cond_proj.data_ptr()
    unet.fuse_lora(lora, 0.5, base_state_dict=sd)
    want = (sd[f"{k}.weight"].float() + 0.5 * (lora[f"{k}.lora_B.weight"] @ lora[f"{k}.lora_A.weight"])).to(bf16)
    assert unet.time_cond_proj.data_ptr() == ptr and not torch.equal(unet.time_cond_proj, w0)
    assert torch.allclose(unet.time_cond_proj.float(), want.float(), rtol=1e-2, atol=1e-2)
    unet.unfuse_lora(base_state_dict=sd)
    assert torch.equal(unet.time_cond_proj, w0)


# ----------------------------------------------------------------------------------------------------------------------
# ABI
# ----------------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged_and_the_entry_point_refuses_bad_prediction_types():
    assert L.PRED_LCM == 4 and (L.PRED_EPSILON, L.PRED_V, L.PRED_SAMPLE) == (0, 1, 2)
    assert L.FN_COUNT == 36 and L.FN_IDS["da_dpmpp_2m_step"] == L.FN_COUNT - 1 and L.FN_IDS["da_x0_linear_step"] == 12
    header = (ROOT / "include" / "diffusers_amd.h").read_text()
    assert "#define DA_ABI_VERSION 9" in header
    proto = re.search(r"int da_x0_linear_step\((.*?)\);", header, re.S).group(1)
    assert " ".join(proto.split()) == ("const void* eps, const void* x, const void* noise, long long noise_step_stride, void* out, "
                                       "const float* table, const int* step_idx, int cfg, float guidance, long long n, int dtype, "
                                       "int pred_type, void* stream")
    lib = L.load()
    assert lib.da_version() == L.ABI_VERSION == 9
    assert lib.da_plan_arg_kinds(L.FN_IDS["da_x0_linear_step"]).decode() == "ppplpppiflii"
    one = 1 << 12       # any non-null value: a refused call dereferences nothing
    for bad in (3, 7, 8, -1):
        assert lib.da_x0_linear_step(one, one, one, 0, one, one, one, 0, 0.0, 16, 0, bad, None) == 1, bad
    for lcm in (4, 5, 6):                                                 # the consistency update needs its noise pointer
        assert lib.da_x0_linear_step(one, one, None, 0, one, one, one, 0, 0.0, 16, 0, lcm, None) == 1, lcm
    assert lib.da_x0_linear_step(one, one, one, 0, one, one, one, 0, 0.0, 0, 0, 4, None) == 1           # n <= 0
    assert lib.da_x0_linear_step(one, one, one, -1, one, one, one, 0, 0.0, 16, 0, 4, None) == 1          # a negative stride
