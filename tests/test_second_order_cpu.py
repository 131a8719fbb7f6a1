"""HeunDiscreteScheduler / KDPM2DiscreteScheduler, host side -- no kernel runs here.

The reference implementation is not available to the suite: the tables, the entry bookkeeping and the loops are checked against the
float64 restatement of the published algorithms in tests/second_order_emulation.py (Karras et al. 2022 Alg. 1, k-diffusion's
sample_dpm_2), and the fused step is stood in for by that file's torch fp32 restatement of the header's arithmetic, which the GPU
tests compare with the kernel to the bit.

Bounds.  A table value is a float64 value rounded once to fp32: 2^-23 relative covers the rounding (2^-24) and the last-digit
differences of two float64 evaluations.  The fp32 loop against float64: ``EPS32`` = 2^-20 per entry, the per-step fp32 rule of
test_dpmsolver_cpu.py (about ten roundings of 2^-24 with 16x headroom), times the 2n - 1 entries, of the largest sample."""
import json
import math

import numpy as np
import pytest
import torch

import diffusers_amd
from diffusers_amd import _lib as L
from diffusers_amd import factory, ops
from diffusers_amd.schedulers import EulerDiscreteScheduler, HeunDiscreteScheduler, KDPM2DiscreteScheduler

import second_order_emulation as E
from second_order_emulation import EPS32

bf16 = torch.bfloat16
SD_BETAS = dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)
KINDS = {"heun": HeunDiscreteScheduler, "kdpm2": KDPM2DiscreteScheduler}
TEN_BETAS = tuple(float(b) for b in np.linspace(0.05, 0.6, 10))


@pytest.fixture(autouse=True)
def _emulated_kernels(monkeypatch):
    E.install(monkeypatch, ops)


def _sched(kind, n=None, **kw):
    cfg = dict(SD_BETAS)
    cfg.update(kw)
    s = KINDS[kind](**cfg)
    if n is not None:
        s.set_timesteps(n, device="cpu")
    return s


# ----------------------------------------------------------------------------------------------------------------------
# 1. tables
# ----------------------------------------------------------------------------------------------------------------------
TABLE_CASES = {
    "linspace": (dict(timestep_spacing="linspace"), dict(spacing="linspace")),
    "leading": (dict(timestep_spacing="leading"), dict(spacing="leading")),
    "trailing": (dict(timestep_spacing="trailing"), dict(spacing="trailing")),
    "leading_offset1": (dict(timestep_spacing="leading", steps_offset=1), dict(spacing="leading", steps_offset=1)),
    "karras": (dict(use_karras_sigmas=True), dict(ladder="karras")),
    "exponential": (dict(use_exponential_sigmas=True), dict(ladder="exponential")),
    "karras_trailing": (dict(use_karras_sigmas=True, timestep_spacing="trailing"), dict(ladder="karras", spacing="trailing")),
    "v_prediction": (dict(prediction_type="v_prediction"), {}),
    "sample": (dict(prediction_type="sample"), {}),
    "default_betas": (dict(beta_schedule="linear", beta_start=0.00085, beta_end=0.012),
                      dict(beta_schedule="linear", beta_start=0.00085, beta_end=0.012)),
    "trained_betas_10": (dict(trained_betas=TEN_BETAS, num_train_timesteps=10), dict(trained_betas=TEN_BETAS)),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("case", sorted(TABLE_CASES))
def test_tables_equal_the_float64_restatement(kind, case):
    opts, ref_opts = TABLE_CASES[case]
    betas = {} if "trained_betas" in ref_opts or "beta_schedule" in ref_opts else SD_BETAS
    sig_all = E.ref_training_sigmas(**{k: v for k, v in {**betas, **ref_opts}.items()
                                       if k in ("trained_betas", "beta_schedule", "beta_start", "beta_end")})
    lad = {k: v for k, v in ref_opts.items() if k in ("spacing", "ladder", "steps_offset")}
    for n in (1, 2, 3, 10):
        s = _sched(kind, n, **opts)
        ts, sig = E.ref_ladder(n, sig_all=sig_all, **lad)
        want = E.entries(kind, ts, sig, sig_all)
        got = s.device_table.double().numpy()
        assert got.shape == (2 * n - 1, 8) and s.device_table.dtype == torch.float32
        assert (got[:, 6] == want[:, 6]).all()
        err = np.abs(got - want)
        assert (err <= 2.0 ** -23 * np.abs(want)).all(), (n, float((err / np.maximum(np.abs(want), 1e-300)).max()))
        # what the pipelines read besides the table: one timestep and one sigma per entry (and the terminal 0)
        assert np.array_equal(s.timesteps.numpy(), got[:, 7].astype(np.float32))
        assert np.array_equal(s.sigmas.numpy(), np.concatenate([got[:, 0], [0.0]]).astype(np.float32))
        assert s.num_inference_steps == n and s.step_index is None and s.begin_index is None


def test_sigmas_are_the_euler_ladder():
    """The predictor entries sit on the sigmas EulerDiscreteScheduler forms for the same options (its fp32 training ladder against
    the float64 one here: a few 1e-5 relative, see DPMSolverMultistepScheduler), the final entry is Euler's final step."""
    for opts in (dict(timestep_spacing="leading", steps_offset=1), dict(use_karras_sigmas=True), dict(timestep_spacing="trailing")):
        eul = EulerDiscreteScheduler(**SD_BETAS, **opts)
        eul.set_timesteps(6, device="cpu")
        for kind in KINDS:
            s = _sched(kind, 6, **opts)
            rows = s.device_table.numpy()
            assert np.allclose(rows[0::2, 0], eul.sigmas.numpy()[:-1], rtol=1e-4, atol=0)
            assert np.allclose(rows[0::2, 7], eul.timesteps.numpy(), rtol=1e-4, atol=1e-3)
            assert np.allclose(rows[-1, [0, 2, 3, 4, 5]], eul.device_table.numpy()[-1, [0, 2, 3, 4, 5]], rtol=1e-4)
            assert abs(float(s.init_noise_sigma) / float(eul.init_noise_sigma) - 1) < 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# 2. entry bookkeeping
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_entry_bookkeeping(kind):
    assert KINDS[kind].order == 2 and _sched(kind).order == 2
    for n in (1, 2, 3, 10):
        s = _sched(kind, n, use_karras_sigmas=True)
        assert len(s.timesteps) == 2 * n - 1 == s.device_table.shape[0] and len(s.sigmas) == 2 * n
        assert s.phases == [1, 2] * (n - 1) + [0] == [int(p) for p in s.device_table[:, 6]]
        ts = s.timesteps.tolist()
        assert all(a >= b for a, b in zip(ts, ts[1:]))
        if kind == "heun":
            assert ts[1::2] == ts[2::2]                                    # [t0, t1, t1, t2, t2, ...]
            assert len(set(ts)) == n
        else:
            assert all(ts[j - 1] > ts[j] > ts[j + 1] for j in range(1, 2 * n - 1, 2))      # fractional mid timesteps, strictly between
            assert all(float(t) != round(float(t)) for t in ts[1::2])
        # sigma of an entry: the noise level of the latents that enter it
        sg = s.sigmas.tolist()
        assert all(a > b for a, b in zip(sg[0::2], sg[2::2])) and sg[-1] == 0.0
    s = _sched(kind, 3)
    assert s.state_in_first_order
    for bad in (1, 3):
        with pytest.raises(ValueError, match="corrector"):
            s.set_begin_index(bad)
        with pytest.raises(ValueError, match="corrector"):
            s.reset(bad)
    s.set_begin_index(2)
    assert s.begin_index == 2 and int(s.device_step) == 2
    x = torch.randn(1, 4, 4, 4, generator=torch.Generator().manual_seed(0))
    hist = s.history(x)
    assert hist.dtype == torch.float32 and hist.shape == x.shape and s.graph_buffers(x) == (hist.data_ptr(),)
    assert s.graph_token() == (type(s).__name__, s._serial, L.PRED_EPSILON)
    s.step_inplace(torch.zeros_like(x), x)
    assert (s.step_index, int(s.device_step), s.state_in_first_order) == (3, 3, False)
    s.step_inplace(torch.zeros_like(x), x)
    s.step_inplace(torch.zeros_like(x), x)
    assert s.step_index == 5 and s.history(x) is hist
    with pytest.raises(IndexError, match="entry 5"):
        s.step_inplace(torch.zeros_like(x), x)
    table, step = s.device_table, s.device_step
    s.set_timesteps(3, device="cpu")                                       # same length: the device buffers keep their addresses
    assert (s.device_table.data_ptr(), s.device_step.data_ptr(), int(s.device_step)) == (table.data_ptr(), step.data_ptr(), 0)
    # the eager step() of the reference's signature finds its entry from the timestep; a repeated timestep is its predictor
    out = s.step(torch.zeros_like(x), s.timesteps[2], x)
    assert s.step_index == 3 and out.prev_sample.data_ptr() != x.data_ptr()
    assert isinstance(s.step(torch.zeros_like(x), s.timesteps[3], x, return_dict=False), tuple)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_options_that_are_not_built_are_refused_by_name(kind):
    cls = KINDS[kind]
    with pytest.raises(NotImplementedError, match="use_beta_sigmas"):
        cls(use_beta_sigmas=True)
    with pytest.raises(NotImplementedError, match="beta_schedule='squaredcos_cap_v2'"):
        cls(beta_schedule="squaredcos_cap_v2")
    with pytest.raises(ValueError, match="prediction_type='flow'"):
        cls(prediction_type="flow")
    with pytest.raises(ValueError, match="Only one of"):
        cls(use_karras_sigmas=True, use_exponential_sigmas=True)
    with pytest.raises(NotImplementedError, match="custom timesteps"):
        cls().set_timesteps(device="cpu", timesteps=[900, 500, 100])
    with pytest.raises(ValueError, match="is not supported"):
        cls(timestep_spacing="middle").set_timesteps(3, device="cpu")
    with pytest.raises(ValueError, match="set_timesteps"):
        cls().step(torch.zeros(1, 4, 2, 2), 10.0, torch.zeros(1, 4, 2, 2))
    s = cls()
    s.set_timesteps(2, device="cpu")
    with pytest.raises(ValueError, match="in place"):
        s.step_cfg(torch.zeros(2, 4, 2, 2), torch.zeros(1, 4, 2, 2), 5.0, out=torch.zeros(1, 4, 2, 2))
    if kind == "heun":
        with pytest.raises(NotImplementedError, match="clip_sample"):
            cls(clip_sample=True)
        assert cls(clip_sample=False, clip_sample_range=2.0).config.clip_sample_range == 2.0
    else:
        with pytest.raises(TypeError, match="clip_sample"):
            cls(clip_sample=False)
    ref_keys = {"num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "prediction_type",
                "use_karras_sigmas", "use_exponential_sigmas", "use_beta_sigmas", "timestep_spacing", "steps_offset"}
    assert set(cls._defaults) == ref_keys | ({"clip_sample", "clip_sample_range"} if kind == "heun" else set())
    d = cls().config
    assert (d.num_train_timesteps, d.beta_start, d.beta_end, d.beta_schedule, d.timestep_spacing, d.steps_offset) == \
        (1000, 0.00085, 0.012, "linear", "linspace", 0)
    # from another sampler's config, as users switch samplers
    eul = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    s = cls.from_config(eul.config, use_karras_sigmas=True)
    assert s.config.steps_offset == 1 and s.config.timestep_spacing == "leading" and s.config.use_karras_sigmas
    assert getattr(diffusers_amd, cls.__name__) is cls and cls.__name__ in diffusers_amd.__all__
    assert L.PRED_SECOND_ORDER == 8


# ----------------------------------------------------------------------------------------------------------------------
# 3. the one-buffer identity
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("pred", E.PREDS)
def test_row_form_with_one_history_buffer_is_the_textbook_step(kind, pred):
    """x + dt (d + d') / 2 = (x + (dt/2) d) + (dt/2) d' and x + dt d_mid with m1 = x: the loop over the rows, one buffer, against the
    loop over the steps in their published two-evaluation form, in float64 -- equal up to float64 rounding."""
    rng = np.random.default_rng(7)
    for n, ladder in ((1, "plain"), (2, "karras"), (5, "plain"), (8, "karras")):
        sig_all = E.ref_training_sigmas(**SD_BETAS)
        ts, sig = E.ref_ladder(n, ladder=ladder, sig_all=sig_all)
        rows = E.entries(kind, ts, sig, sig_all)
        es = rng.standard_normal((2 * n, 64))
        x = rng.standard_normal(64) * sig[0]
        model = lambda x_, s_, j: es[j] + 0.05 * np.tanh(x_ / (1 + s_))      # noqa: E731  (depends on x, sigma and the entry)
        want = E.ref_loop(kind, x, model, sig, pred)
        got = E.row_loop(x, model, rows, pred)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(x).max()), (n, ladder)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the fp32 loop against float64; order
# ----------------------------------------------------------------------------------------------------------------------
def _gauss_model(s_data, pred="epsilon"):
    """Model outputs of the exact denoiser of N(0, s^2) data, D(x, sigma) = x s^2 / (s^2 + sigma^2)."""
    def model(x, sigma, _=None):
        den = x * s_data ** 2 / (s_data ** 2 + sigma ** 2)
        if pred == "epsilon":
            return (x - den) / sigma
        if pred == "sample":
            return den
        return (den - x / (sigma ** 2 + 1)) / (-sigma / math.sqrt(sigma ** 2 + 1))
    return model


def _scheduler_loop(s, x, model):
    """The scheduler's loop on fp32 tensors: the model is evaluated in float64 at the sigma of the entry, its output rounded to fp32."""
    rows = s.device_table.double().numpy()
    x = torch.from_numpy(np.asarray(x, np.float64)).float().reshape(1, 4, 4, 4)
    s.reset(0)
    for j in range(len(rows)):
        e = model(x.double().numpy(), float(rows[j, 0]), j)
        s.step_inplace(torch.from_numpy(e).float(), x)
    return x.double().numpy().reshape(-1)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("pred", E.PREDS)
def test_fp32_loop_equals_the_float64_restatement(kind, pred):
    rng = np.random.default_rng(3)
    for n, opts, lad in ((3, {}, {}), (10, dict(use_karras_sigmas=True), dict(ladder="karras")),
                         (1, dict(timestep_spacing="trailing"), dict(spacing="trailing"))):
        s = _sched(kind, n, prediction_type=pred, **opts)
        ts, sig = E.ref_ladder(n, **lad, **SD_BETAS)
        for s_data in (0.5, 1.0, 2.0):
            x = rng.standard_normal(64) * math.sqrt(s_data ** 2 + sig[0] ** 2)
            x = x.astype(np.float32).astype(np.float64)
            model = _gauss_model(s_data, pred)
            want = E.ref_loop(kind, x, model, sig, pred)
            got = _scheduler_loop(s, x, model)
            err = np.abs(got - want).max()
            assert err <= (2 * n - 1) * EPS32 * np.abs(x).max(), (n, s_data, err / ((2 * n - 1) * EPS32 * np.abs(x).max()))


@pytest.mark.parametrize("n", [10, 25])
@pytest.mark.parametrize("s_data", [0.5, 1.0, 2.0])
def test_second_order_beats_euler_at_the_same_number_of_model_calls(n, s_data):
    """Karras ladder, exact Gaussian denoiser: the solution of the probability-flow ODE at sigma = 0 is x sqrt(s^2 / (s^2 + sigma_0^2)).
    n Heun / DPM2 steps are 2n - 1 model calls: their error is below that of Euler with 2n - 1 steps, which is below Euler with n."""
    rng = np.random.default_rng(11)
    model = _gauss_model(s_data)
    errs = {}
    x = None
    for name, steps in (("heun", n), ("kdpm2", n), ("euler_same_calls", 2 * n - 1), ("euler_same_steps", n)):
        ts, sig = E.ref_ladder(steps, ladder="karras", **SD_BETAS)
        if x is None:
            x = (rng.standard_normal(64) * math.sqrt(s_data ** 2 + sig[0] ** 2)).astype(np.float32).astype(np.float64)
        exact = x * math.sqrt(s_data ** 2 / (s_data ** 2 + sig[0] ** 2))
        if name in KINDS:
            got = _scheduler_loop(_sched(name, steps, use_karras_sigmas=True), x, model)
        else:
            got = E.ref_loop("euler", x, model, sig)
        errs[name] = float(np.sqrt(np.mean((got - exact) ** 2)))
    print(f"[order] n={n} s={s_data}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["heun"] < errs["euler_same_calls"] and errs["kdpm2"] < errs["euler_same_calls"], errs
    assert errs["euler_same_calls"] < errs["euler_same_steps"], errs


# ----------------------------------------------------------------------------------------------------------------------
# 5. pipelines on the stand-in
# ----------------------------------------------------------------------------------------------------------------------
def _embeds(kind):
    g = torch.Generator().manual_seed(3)
    d = dict(prompt_embeds=torch.randn((1, 7, 64), generator=g).to(bf16), negative_prompt_embeds=torch.randn((1, 7, 64), generator=g).to(bf16),
             output_type="latent", use_graph=False)
    if kind == "sdxl":
        d.update(pooled_prompt_embeds=torch.randn((1, 64), generator=g).to(bf16),
                 negative_pooled_prompt_embeds=torch.randn((1, 64), generator=g).to(bf16))
    return d


def _pipe(kind, scheduler, **kw):
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    return build(device="cpu", tiny=True, seed=0, scheduler=scheduler, **kw)


@pytest.fixture
def step_log(monkeypatch):
    """Every call of the fused step: (device step counter, phase of its row, cfg)."""
    log = []
    inner = ops.second_order_step_

    def logged(eps, x, m1, table, step_idx, begin_idx, **kw):
        log.append((int(step_idx), int(table[int(step_idx), 6]), kw["cfg"]))
        return inner(eps, x, m1, table, step_idx, begin_idx, **kw)
    monkeypatch.setattr(ops, "second_order_step_", logged)
    return log


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
@pytest.mark.parametrize("scheduler", sorted(KINDS))
def test_text_to_image_runs_one_fused_step_per_entry(kind, scheduler, step_log):
    pipe = _pipe(kind, scheduler)
    assert isinstance(pipe.scheduler, KINDS[scheduler])
    seen = []
    call = dict(num_inference_steps=3, guidance_scale=5.0, height=32, width=32, **_embeds(kind))
    out = pipe(generator=torch.Generator().manual_seed(1), callback_on_step_end=lambda p, i, t, d: seen.append((i, float(t))) or {},
               **call).images
    assert out.shape == (1, 4, 16, 16) and out.dtype == bf16 and torch.isfinite(out.float()).all()
    assert step_log == [(0, 1, True), (1, 2, True), (2, 1, True), (3, 2, True), (4, 0, True)]
    assert seen == list(enumerate(pipe.scheduler.timesteps.tolist())) and len(seen) == 5
    assert pipe.scheduler.step_index == 5 and int(pipe.scheduler.device_step) == 5
    # the same call again: the same latents (what the first call left in the history is not read)
    assert torch.equal(pipe(generator=torch.Generator().manual_seed(1), **call).images, out)
    # guidance_rescale and guidance_scale <= 1 hand the step a plain model output
    for kw in (dict(guidance_rescale=0.7), dict(guidance_scale=1.0)):
        del step_log[:]
        o = pipe(generator=torch.Generator().manual_seed(1), **{**call, **kw}).images
        assert torch.isfinite(o.float()).all() and not torch.equal(o, out)
        assert [c for _, _, c in step_log] == [False] * 5
    if kind == "sdxl":
        for kw in (dict(timesteps=[900, 500, 100]), dict(sigmas=[10.0, 1.0, 0.0])):
            with pytest.raises(ValueError, match="does not support custom timestep or sigma schedules"):
                pipe(**{**call, **kw})
        del step_log[:]
        pipe(generator=torch.Generator().manual_seed(1), denoising_end=0.5, **{**call, "num_inference_steps": 6})
        ts = pipe.scheduler.timesteps.tolist()
        assert [j for j, _, _ in step_log] == list(range(len([t for t in ts if t >= 500]))) and 0 < len(step_log) < 11


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
@pytest.mark.parametrize("scheduler", sorted(KINDS))
def test_img2img_begins_on_a_predictor(kind, scheduler, step_log):
    pipe = _pipe(kind, scheduler, img2img=True)
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    seen = []
    out = pipe(image=img, strength=0.67, num_inference_steps=3, guidance_scale=5.0, generator=torch.Generator().manual_seed(2),
               callback_on_step_end=lambda p, i, t, d: seen.append(float(t)) or {}, **_embeds(kind)).images
    sch = pipe.scheduler
    # int(3 * 0.67) = 2 of the 3 steps run: entries 2, 3, 4 -- a predictor, its corrector, the final Euler entry
    assert torch.isfinite(out.float()).all() and sch.begin_index == 2 and step_log == [(2, 1, True), (3, 2, True), (4, 0, True)]
    assert seen == sch.timesteps.tolist()[2:]
    assert pipe.get_timesteps(3, 0.67)[1] == 2                                            # the reference's: in steps
    del step_log[:]
    pipe(image=img, strength=1.0, num_inference_steps=3, generator=torch.Generator().manual_seed(2), **_embeds(kind))
    assert [j for j, _, _ in step_log] == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="< 1"):
        pipe(image=img, strength=0.2, num_inference_steps=3, generator=torch.Generator().manual_seed(2), **_embeds(kind))
    if kind == "sdxl":
        # the refiner side of a hand-off: the entries below the cut-off, one more when their number is even (the order-2 rule)
        for start in (0.3, 0.5, 0.7):
            del step_log[:]
            pipe(image=out, denoising_start=start, num_inference_steps=4, generator=torch.Generator().manual_seed(2), **_embeds(kind))
            ts = sch.timesteps.tolist()
            below = len([t for t in ts if t < int(round(1000 - start * 1000))])
            want = below + (below % 2 == 0)
            assert [j for j, _, _ in step_log] == list(range(7 - want, 7)) and step_log[0][1] == 1, start


@pytest.mark.parametrize("scheduler", sorted(KINDS))
def test_inpainting_renoises_the_known_region_to_the_level_after_each_entry(scheduler, monkeypatch):
    pipe = _pipe("sd15", scheduler, inpaint=True, unet_in_channels=4)
    reads = []
    inner = ops.inpaint_blend_

    def logged(latents, image_latents, noise, mask, coef, step_idx):
        reads.append((int(step_idx), tuple(coef[int(step_idx)].tolist())))
        return inner(latents, image_latents, noise, mask, coef, step_idx)
    monkeypatch.setattr(ops, "inpaint_blend_", logged)
    img = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    out = pipe(image=img, mask_image=torch.zeros(32, 32), strength=1.0, num_inference_steps=3,
               generator=torch.Generator().manual_seed(5), **_embeds("sd15")).images
    sch = pipe.scheduler
    table = sch.add_noise_table(bf16)
    assert table.shape == (6, 2)
    sig = sch.sigmas.to(bf16).float().tolist()
    assert [tuple(r) for r in table.tolist()] == [(1.0, sig[j]) for j in range(5)] + [(1.0, 0.0)]
    # after entry j the blend reads row j + 1: sigma_eval of the next entry, the clean latents after the last one
    assert reads == [(j + 1, (1.0, sig[j + 1])) for j in range(5)]
    assert torch.equal(out, pipe._inpaint["image_latents"])                                # mask == 0 everywhere
    pipe9 = _pipe("sdxl", scheduler, inpaint=True, unet_in_channels=9)
    o = pipe9(image=img, mask_image=torch.ones(32, 32), strength=0.67, num_inference_steps=3, generator=torch.Generator().manual_seed(5),
              **_embeds("sdxl")).images
    assert torch.isfinite(o.float()).all() and pipe9.scheduler.begin_index == 2


def test_add_noise_is_sigma_of_the_entry_at_the_begin_index():
    for kind in KINDS:
        s = _sched(kind, 4)
        x = torch.ones(1, 4, 2, 2, dtype=bf16)
        sig = s.sigmas.to(bf16)
        s.set_begin_index(2)
        a, b = s._add_noise_coeffs(s.timesteps[5:6], bf16)
        assert (a, b) == ([1.0], [float(sig[2])])
        assert torch.equal(s.add_noise(torch.zeros_like(x), x, s.timesteps[2:3]), x * sig[2])
        assert float(s.init_noise_sigma) == float(s.sigmas.max())
        got = s.scale_model_input(x.float(), s.timesteps[2])
        assert torch.allclose(got, x.float() / float((s.sigmas[2] ** 2 + 1) ** 0.5), rtol=1e-6)


def test_pipeline_directory_that_names_the_scheduler_loads(tmp_path):
    from diffusers_amd.pipelines import StableDiffusionXLPipeline
    for name, cls in (("HeunDiscreteScheduler", HeunDiscreteScheduler), ("KDPM2DiscreteScheduler", KDPM2DiscreteScheduler)):
        root = tmp_path / name
        (root / "scheduler").mkdir(parents=True)
        cfg = dict(factory.SECOND_ORDER_SCHEDULER, _class_name=name, _diffusers_version="0.40.0", use_karras_sigmas=True,
                   trained_betas=None, prediction_type="v_prediction", num_train_timesteps=1000)
        (root / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
        sch = StableDiffusionXLPipeline._load_component(root, "scheduler", "diffusers", name, "cpu", None, "none", False)
        assert type(sch) is cls and sch.config.use_karras_sigmas and sch.config.steps_offset == 1 and sch._pred == L.PRED_V
    with pytest.raises(NotImplementedError, match="HeunDiscrete, KDPM2Discrete"):
        StableDiffusionXLPipeline._load_component(tmp_path, "scheduler", "diffusers", "KDPM2AncestralDiscreteScheduler", "cpu", None,
                                                  "none", False)
    with pytest.raises(ValueError, match="'heun' or 'kdpm2'"):
        factory.build_sdxl_pipeline(device="cpu", tiny=True, scheduler="dpm3")
