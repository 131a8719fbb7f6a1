"""DPMSolverMultistepScheduler (DPM-Solver++ 2M), host side -- no kernel runs here.

The reference implementation is not available to the suite, so this file restates the algorithm in float64 numpy (``ref_*`` below:
schedule, one step, a whole loop) from its published form -- Lu et al., "DPM-Solver++", Alg. 2 (data prediction, multistep), the
Karras et al. rho = 7 sigma ladder, the k-diffusion sigma <-> (alpha, sigma) change of variables -- and checks the scheduler's
tables and loops against it, plus facts that do not depend on the restatement (k-diffusion's sigma_max / sigma_min of SD, the
closed form of a constant-x0 model, second order beating first order on Gaussian data).  ``tests/test_dpmsolver_gpu.py`` imports
the restatement from here.  The CPU stand-in of the step op lives here too and is installed with ``monkeypatch``."""
import itertools
import json
import math

import numpy as np
import pytest
import torch

from diffusers_amd import _lib as L
from diffusers_amd import factory, ops
from diffusers_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler

import ops_emulation

bf16 = torch.bfloat16
SD_BETAS = dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)
EPS32 = 2.0 ** -20          # fp32 step bound: ~10 roundings of 2^-24 each, 16x headroom (see step_terms)


# ----------------------------------------------------------------------------------------------------------------------
# float64 restatement
# ----------------------------------------------------------------------------------------------------------------------
def ref_sig_all(beta_schedule="linear", beta_start=1e-4, beta_end=0.02, N=1000):
    """sqrt((1 - abar) / abar) of the training schedule, float64 throughout."""
    if beta_schedule == "linear":
        betas = np.linspace(beta_start, beta_end, N)
    else:
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, N) ** 2
    ac = np.cumprod(1.0 - betas)
    return np.sqrt((1 - ac) / ac)


def ref_sigma_to_t(sigma, log_sigmas):
    """Fractional training timestep of a sigma: piecewise-linear inverse of log sigma(t)."""
    ls = math.log(max(float(sigma), 1e-10))
    below = np.nonzero(log_sigmas <= ls)[0]
    lo = min(int(below[-1]) if len(below) else 0, len(log_sigmas) - 2)
    # (log_sigmas is increasing, so "last index with log_sigmas <= ls" is the count-based index the scheduler uses)
    low, high = log_sigmas[lo], log_sigmas[lo + 1]
    w = min(max((low - ls) / (low - high), 0.0), 1.0)
    return (1 - w) * lo + w * (lo + 1)


def ref_schedule(n, spacing="linspace", ladder="plain", final="zero", steps_offset=0, N=1000, **betas):
    """(timesteps int64 [n], sigmas float32 [n + 1])."""
    sig_all = ref_sig_all(N=N, **betas)
    if spacing == "linspace":
        ts = np.linspace(0, N - 1, n + 1).round()[::-1][:-1]
    elif spacing == "leading":
        ts = (np.arange(0, n + 1) * (N // (n + 1))).round()[::-1][:-1] + steps_offset
    else:
        ts = np.arange(N, 0, -N / n).round() - 1
    ts = ts.astype(np.int64)
    smin, smax = float(sig_all[0]), float(sig_all[-1])
    if ladder == "plain":
        sig = np.interp(ts, np.arange(N), sig_all)
    else:
        if ladder == "karras":
            rho, ramp = 7.0, np.linspace(0, 1, n)
            sig = (smax ** (1 / rho) + ramp * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
        else:
            sig = np.exp(np.linspace(math.log(smax), math.log(smin), n))
        log_sigmas = np.log(sig_all)
        ts = np.array([ref_sigma_to_t(s, log_sigmas) for s in sig]).round().astype(np.int64)
    last = 0.0 if final == "zero" else smin
    return ts, np.concatenate([sig, [last]]).astype(np.float32)


def ref_alpha_sigma(s):
    s = np.float64(s)
    a = 1.0 / np.sqrt(s * s + 1.0)
    return a, s * a


def ref_lambda(s):
    a, b = ref_alpha_sigma(s)
    return np.log(a) - np.log(b)


def ref_first_order(i, n, first_of_loop, solver_order=2, lower_order_final=True, euler_at_final=False, final="zero"):
    return bool(solver_order == 1 or first_of_loop
                or (i == n - 1 and (euler_at_final or final == "zero" or (lower_order_final and n < 15))))


def ref_x0(x, e, s0, pred):
    a0, b0 = ref_alpha_sigma(s0)
    if pred == "epsilon":
        return (x - b0 * e) / a0
    if pred == "v_prediction":
        return a0 * x - b0 * e
    return e


def ref_step(x, e, m1, sig, i, first, solver_type="midpoint", pred="epsilon"):
    """One step from row i in float64: (next sample, this step's x0)."""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    s0, t = np.float64(sig[i]), np.float64(sig[i + 1])
    x0 = ref_x0(x, e, s0, pred)
    if t == 0:                                      # h = inf: exp(-h) - 1 = -1, sigma_vp(t) = 0, alpha(t) = 1
        assert first
        return x0.copy(), x0
    if t == s0:                                     # a step of no length
        return x.copy(), x0
    at, bt = ref_alpha_sigma(t)
    _, b0 = ref_alpha_sigma(s0)
    h = ref_lambda(t) - ref_lambda(s0)
    em1 = np.exp(-h) - 1.0
    xn = (bt / b0) * x - at * em1 * x0
    if not first:
        r0 = (ref_lambda(s0) - ref_lambda(np.float64(sig[i - 1]))) / h
        d1 = (x0 - np.asarray(m1, np.float64)) / r0
        xn = xn - 0.5 * at * em1 * d1 if solver_type == "midpoint" else xn + at * (em1 / h + 1.0) * d1
    return xn, x0


def ref_loop(x, model, sig, begin=0, steps=None, **cfg):
    """The whole loop from row ``begin``: every intermediate sample.  ``model(x, i)`` returns the model output at row i."""
    n = len(sig) - 1
    steps = n - begin if steps is None else steps
    sk = {k: cfg[k] for k in ("solver_order", "lower_order_final", "euler_at_final", "final") if k in cfg}
    m1, out = None, []
    for i in range(begin, begin + steps):
        first = ref_first_order(i, n, i == begin, **sk)
        x, m1 = ref_step(x, model(x, i), m1, sig, i, first, cfg.get("solver_type", "midpoint"), cfg.get("pred", "epsilon"))
        out.append(x)
    return out


def row_step(x, e, m1, row, second, pred):
    """The update in float64 from the fp32 table row the kernel reads -> (next sample, x0, T).  T = the sum of the absolute values of
    the terms of the update, every product expanded down to the inputs: the quantity fp32 rounding errors are relative to."""
    x, e, m1 = (np.asarray(v, np.float64) for v in (x, e, m1))
    a0, b0, cx, c0, cd = (np.float64(v) for v in row[:5])
    if pred == 0:
        x0, t0 = (x - b0 * e) / a0, (np.abs(x) + np.abs(b0 * e)) / a0
    elif pred == 1:
        x0, t0 = a0 * x - b0 * e, np.abs(a0 * x) + np.abs(b0 * e)
    else:
        x0, t0 = e, np.abs(e)
    xn, T = cx * x + c0 * x0, np.abs(cx * x) + np.abs(c0) * t0
    if second:
        xn, T = xn + cd * (x0 - m1), T + np.abs(cd) * (t0 + np.abs(m1))
    return xn, x0, T, t0


# ----------------------------------------------------------------------------------------------------------------------
# CPU stand-in of ops.dpmpp_2m_step_ (fp32 torch ops, one rounding at the store of x; the history stays fp32)
# ----------------------------------------------------------------------------------------------------------------------
def dpmpp_2m_step_(eps, x, m1, table, step_idx, begin_idx, *, cfg=False, guidance=0.0, pred_type=0):
    r = table[int(step_idx)].float()
    e = ops_emulation._cfg(eps, cfg, guidance, x.numel()).view(x.shape).float()
    xf = x.float()
    if pred_type == 0:
        x0 = (xf - r[1] * e) / r[0]
    elif pred_type == 1:
        x0 = r[0] * xf - r[1] * e
    else:
        x0 = e
    xn = r[2] * xf + r[3] * x0
    if float(r[6]) != 0.0 and int(step_idx) != int(begin_idx):
        xn = xn + r[4] * (x0 - m1)
    m1.copy_(x0)
    x.copy_(xn.to(x.dtype))
    return x


@pytest.fixture(autouse=True)
def _emulated_kernels(monkeypatch):
    ops_emulation.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "dpmpp_2m_step_", dpmpp_2m_step_)
    monkeypatch.setattr(ops, "TUNING", False)


def _sched(n=None, **kw):
    cfg = dict(SD_BETAS)
    cfg.update(kw)
    s = DPMSolverMultistepScheduler(**cfg)
    if n is not None:
        s.set_timesteps(n, device="cpu")
    return s


LADDERS = {"plain": {}, "karras": {"use_karras_sigmas": True}, "exponential": {"use_exponential_sigmas": True}}


# ----------------------------------------------------------------------------------------------------------------------
# 1. tables against the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["linspace", "leading", "trailing"])
@pytest.mark.parametrize("ladder", ["plain", "karras", "exponential"])
def test_timesteps_and_sigmas_equal_the_restatement(spacing, ladder):
    for n, final in itertools.product((1, 2, 5, 14, 15, 25, 50), ("zero", "sigma_min")):
        off = 1 if spacing == "leading" else 0
        s = _sched(n, timestep_spacing=spacing, steps_offset=off, final_sigmas_type=final, **LADDERS[ladder])
        ts, sig = ref_schedule(n, spacing, ladder, final, steps_offset=off, **SD_BETAS)
        assert s.timesteps.dtype == torch.int64 and s.sigmas.dtype == torch.float32
        assert np.array_equal(s.timesteps.numpy(), ts), (n, final)
        assert np.array_equal(s.sigmas.numpy(), sig), (n, final)
        assert np.array_equal(s.device_table[:, 7].numpy(), ts.astype(np.float32))      # what the U-Net reads
        assert s.num_inference_steps == n and s.order == 1 and s.init_noise_sigma == 1.0


# ----------------------------------------------------------------------------------------------------------------------
# 2. known answers that do not come from the restatement
# ----------------------------------------------------------------------------------------------------------------------
def test_known_sigmas_of_stable_diffusion():
    """k-diffusion's sigma_max / sigma_min of the SD betas (14.614641 / 0.029167) bound the Karras ladder; `leading` with
    steps_offset = 1 and 10 steps starts at training timestep 901 and ends at 91."""
    s = _sched(25, use_karras_sigmas=True)
    sig = s.sigmas.double().numpy()
    assert abs(sig[0] / 14.614641 - 1) < 1e-5 and abs(sig[-2] / 0.029167 - 1) < 1e-5 and sig[-1] == 0.0
    s = _sched(10, timestep_spacing="leading", steps_offset=1)
    sig = s.sigmas.double().numpy()
    assert s.timesteps.tolist() == list(range(901, 90, -90))
    assert abs(sig[0] / 8.390685 - 1) < 1e-5 and abs(sig[-2] / 0.323533 - 1) < 1e-5


# ----------------------------------------------------------------------------------------------------------------------
# 3. coefficient rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver_type", ["midpoint", "heun"])
def test_rows_are_finite_flagged_by_the_order_rule_and_equal_the_restatement(solver_type):
    probe_x, probe_e, probe_m = np.float64(0.7), np.float64(-0.3), np.float64(0.45)
    for n, lof, eaf, final, order in itertools.product((2, 14, 15, 16), (True, False), (True, False), ("zero", "sigma_min"), (1, 2)):
        s = _sched(n, lower_order_final=lof, euler_at_final=eaf, final_sigmas_type=final, solver_order=order, solver_type=solver_type)
        rows = s.device_table.numpy()
        assert rows.dtype == np.float32 and rows.shape == (n, 8) and np.isfinite(rows).all()
        sig = s.sigmas.numpy()
        for i in range(n):
            want_second = not ref_first_order(i, n, i == 0, order, lof, eaf, final)
            assert bool(rows[i, 6]) == want_second == s.second_order_rows[i], (n, lof, eaf, final, order, i)
            if not want_second:
                assert rows[i, 4] == 0.0
            # the row applied to a probe equals the restated step (fp32 storage of five coefficients: a few 2^-24)
            got = row_step(probe_x, probe_e, probe_m, rows[i], want_second, 0)
            want, _ = ref_step(probe_x, probe_e, probe_m, sig, i, not want_second, solver_type)
            assert abs(got[0] - want) <= 2.0 ** -21 * got[2], (n, i)
        if final == "zero":                     # x' = x0 exactly: cx = 0, c0 = 1, no second-order term
            assert rows[-1, 2] == 0.0 and rows[-1, 3] == 1.0 and rows[-1, 4] == 0.0 and rows[-1, 6] == 0.0


def test_a_step_of_no_length_is_the_identity_row():
    """A Karras ladder ends at sigma_min; with final_sigmas_type="sigma_min" the last step goes from sigma_min to sigma_min (h = 0,
    r0 = 1 / 0): the row is x' = x, first order, and finite."""
    for st in ("midpoint", "heun"):
        s = _sched(16, use_karras_sigmas=True, final_sigmas_type="sigma_min", lower_order_final=False, solver_type=st)
        rows = s.device_table.numpy()
        assert s.sigmas[-1] == s.sigmas[-2] and np.isfinite(rows).all()
        assert rows[-1, 2] == 1.0 and rows[-1, 3] == 0.0 and rows[-1, 4] == 0.0 and rows[-1, 6] == 0.0 and rows[-2, 6] == 1.0


# ----------------------------------------------------------------------------------------------------------------------
# 4. closed form: a model that always predicts x0 = c
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,solver_type", [(1, "midpoint"), (2, "midpoint"), (2, "heun")])
@pytest.mark.parametrize("ladder", ["plain", "karras"])
def test_constant_x0_model_follows_the_closed_form(order, solver_type, ladder):
    """x_i = alpha(s_i) c + sigma(s_i) z for every i and x_n = c: exactly for the float64 restatement (round-off only), and through the
    scheduler (CPU stand-in of the kernel, fp32 latents) within the fp32 step bound of the GPU test G1, per step."""
    n = 12
    rng = np.random.default_rng(0)
    c, z = rng.standard_normal((2, 4, 8, 8)), rng.standard_normal((2, 4, 8, 8))
    s = _sched(n, solver_order=order, solver_type=solver_type, **LADDERS[ladder])
    sig = s.sigmas.double().numpy()

    def closed(i):
        a, b = ref_alpha_sigma(sig[i])
        return a * c + b * z

    def model(x, i):
        a, b = ref_alpha_sigma(sig[i])
        return (x - a * c) / b

    xs = ref_loop(closed(0), model, sig, solver_order=order, solver_type=solver_type)
    for i, x in enumerate(xs):
        assert np.abs(x - closed(i + 1)).max() <= 1e-12 * (1 + sig[i]), i         # round-off of float64 at |x| ~ sigma
    assert np.abs(xs[-1] - c).max() <= 1e-12

    x = torch.from_numpy(closed(0)).float()
    rows = s.device_table.numpy()
    for i, t in enumerate(s.timesteps):
        e = torch.from_numpy(model(x.double().numpy(), i)).float()
        m1 = s.history(x).clone().numpy()
        second = bool(rows[i, 6]) and i != 0
        want, want_x0, T, t0 = row_step(x.numpy(), e.numpy(), m1, rows[i], second, 0)
        x_next = s.step(e, t, x).prev_sample
        assert x_next is not x and x_next.dtype == torch.float32
        assert (np.abs(x_next.double().numpy() - want) <= EPS32 * T).all(), i
        assert (np.abs(s.history(x).double().numpy() - want_x0) <= EPS32 * t0).all(), i
        x = x_next
    assert s.step_index == n
    # the fp32 loop ends at c: per-step errors (kernel arithmetic 2^-20 T, the fp32 rounding of the model output 2^-24 T) pass through
    # cx < 1 of the later steps, and the last step returns its x0, whose own cancellation is (|x| + sigma |e|) / alpha ~ 2 sigma |z| + |c|
    a_l, b_l = ref_alpha_sigma(sig[n - 1])
    tol = 2.0 ** -19 * (2 * b_l * np.abs(z) + np.abs(c)) / a_l + 2.0 ** -19 * 2 * sig[n - 1] * (n - 1) * np.abs(z).max()
    assert (np.abs(x.double().numpy() - c) <= tol).all()
    with pytest.raises(IndexError):
        s.step(e, s.timesteps[-1], x)


# ----------------------------------------------------------------------------------------------------------------------
# 5. second order is better than first
# ----------------------------------------------------------------------------------------------------------------------
def test_second_order_beats_first_order_on_gaussian_data(capsys):
    """Data ~ N(0, 0.5^2): the exact x0 predictor is x alpha s^2 / (alpha^2 s^2 + sigma^2), the exact end point of the probability-flow
    ODE from x_T = sqrt(alpha_T^2 s^2 + sigma_T^2) z is s z.  20 steps, float64 restatement."""
    sd, n = 0.5, 20
    z = np.random.default_rng(1).standard_normal(4096)
    for ladder in ("plain", "karras"):
        _, sig = ref_schedule(n, "linspace", ladder, "zero", **SD_BETAS)
        sig = sig.astype(np.float64)

        def model(x, i):
            a, b = ref_alpha_sigma(sig[i])
            return x * a * sd ** 2 / (a ** 2 * sd ** 2 + b ** 2)

        a0, b0 = ref_alpha_sigma(sig[0])
        start = np.sqrt(a0 ** 2 * sd ** 2 + b0 ** 2) * z
        err = {}
        for order, st in ((1, "midpoint"), (2, "midpoint"), (2, "heun")):
            out = ref_loop(start, model, sig, solver_order=order, solver_type=st, pred="sample")[-1]
            err[order, st] = float(np.sqrt(np.mean((out - sd * z) ** 2)) / np.sqrt(np.mean((sd * z) ** 2)))
        with capsys.disabled():
            print(f"\n[dpmpp] gaussian data, {n} steps, {ladder}: rel rms order 1 {err[1, 'midpoint']:.4f}, "
                  f"order 2 midpoint {err[2, 'midpoint']:.4f}, order 2 heun {err[2, 'heun']:.4f}")
        assert err[2, "midpoint"] < err[1, "midpoint"] and err[2, "heun"] < err[1, "midpoint"], (ladder, err)


# ----------------------------------------------------------------------------------------------------------------------
# 6. configuration, refusals, add_noise, begin index, loading
# ----------------------------------------------------------------------------------------------------------------------
def test_from_config_of_other_schedulers_and_of_a_reference_config_file():
    eul = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    d = DPMSolverMultistepScheduler.from_config(eul.config, use_karras_sigmas=True)
    assert (d.config.beta_schedule, d.config.beta_start, d.config.beta_end) == ("scaled_linear", 0.00085, 0.012)
    assert d.config.timestep_spacing == "leading" and d.config.steps_offset == 1 and d.config.use_karras_sigmas
    assert "interpolation_type" not in d.config and d.config.solver_order == 2 and d.config.algorithm_type == "dpmsolver++"
    ddim = DDIMScheduler(**factory.SD15_SCHEDULER)
    d = DPMSolverMultistepScheduler.from_config(ddim.config)
    assert "clip_sample" not in d.config and "set_alpha_to_one" not in d.config
    assert d.config.timestep_spacing == "leading" and d.config.steps_offset == 1 and d.config.beta_schedule == "scaled_linear"
    back = EulerDiscreteScheduler.from_config(d.config)
    assert back.config.beta_end == 0.012 and back.config.timestep_spacing == "leading"
    # every key of the reference's scheduler_config.json is known (json writes lambda_min_clipped as -Infinity)
    ref_cfg = json.loads(json.dumps(dict(
        _class_name="DPMSolverMultistepScheduler", _diffusers_version="0.40.0", num_train_timesteps=1000, beta_start=0.00085,
        beta_end=0.012, beta_schedule="scaled_linear", trained_betas=None, solver_order=2, prediction_type="epsilon",
        thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0, algorithm_type="dpmsolver++",
        solver_type="midpoint", lower_order_final=True, euler_at_final=False, use_karras_sigmas=True, use_exponential_sigmas=False,
        use_beta_sigmas=False, use_lu_lambdas=False, use_flow_sigmas=False, flow_shift=1.0, final_sigmas_type="zero",
        lambda_min_clipped=-math.inf, variance_type=None, timestep_spacing="leading", steps_offset=1, rescale_betas_zero_snr=False,
        use_dynamic_shifting=False, time_shift_type="exponential")))
    d = DPMSolverMultistepScheduler.from_config(ref_cfg)
    assert set(ref_cfg) - {"_class_name", "_diffusers_version"} == set(d.config) == set(DPMSolverMultistepScheduler._defaults)
    assert d.config == DPMSolverMultistepScheduler(**factory.SDXL_DPM_SCHEDULER).config
    assert factory.SD15_DPM_SCHEDULER["use_karras_sigmas"] and factory.SD15_DPM_SCHEDULER["steps_offset"] == 1
    import diffusers_amd
    assert diffusers_amd.DPMSolverMultistepScheduler is DPMSolverMultistepScheduler
    with pytest.raises(TypeError, match="unexpected config keys"):
        DPMSolverMultistepScheduler(sigma_min=0.1)


@pytest.mark.parametrize("kw,name", [
    (dict(algorithm_type="sde-dpmsolver++"), "sde-dpmsolver\\+\\+"), (dict(algorithm_type="dpmsolver"), "algorithm_type='dpmsolver'"),
    (dict(solver_order=3), "solver_order=3"), (dict(thresholding=True), "thresholding"), (dict(use_beta_sigmas=True), "use_beta_sigmas"),
    (dict(use_flow_sigmas=True), "use_flow_sigmas"), (dict(use_lu_lambdas=True), "use_lu_lambdas"),
    (dict(rescale_betas_zero_snr=True), "rescale_betas_zero_snr"), (dict(use_dynamic_shifting=True), "use_dynamic_shifting"),
    (dict(lambda_min_clipped=-5.1), "lambda_min_clipped"), (dict(variance_type="learned_range"), "variance_type"),
    (dict(solver_type="bh2"), "solver_type"), (dict(prediction_type="flow_prediction"), "prediction_type")])
def test_unsupported_options_are_refused_by_name(kw, name):
    with pytest.raises(NotImplementedError, match=name):
        _sched(**kw)


def test_other_refusals():
    with pytest.raises(NotImplementedError, match="custom timesteps"):
        _sched().set_timesteps(device="cpu", timesteps=[900, 500, 100])
    with pytest.raises(ValueError, match="Only one of"):
        _sched(use_karras_sigmas=True, use_exponential_sigmas=True)
    with pytest.raises(ValueError, match="final_sigmas_type"):
        _sched(final_sigmas_type="one")
    with pytest.raises(ValueError, match="is not supported"):
        _sched(5, timestep_spacing="middle")
    s = _sched()
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(torch.zeros(1, 4, 2, 2), 10, torch.zeros(1, 4, 2, 2))
    s = _sched(4)
    x = torch.zeros(1, 4, 2, 2)
    with pytest.raises(ValueError, match="in place"):
        s.step_cfg(torch.zeros(2, 4, 2, 2), x, 5.0, out=torch.zeros_like(x))


def test_add_noise_coefficients():
    """a = alpha(sigma), b = sigma alpha(sigma) of the row the loop starts at, evaluated in the latents' dtype."""
    s = _sched(10, use_karras_sigmas=True)
    for idx in (0, 4, 9):
        a, b = s._add_noise_coeffs(s.timesteps[idx:idx + 1], bf16)
        sg = s.sigmas[idx].to(bf16)
        al = 1 / ((sg ** 2 + 1) ** 0.5)
        assert a == [float(al)] and b == [float(sg * al)]
        ra, rb = ref_alpha_sigma(float(s.sigmas[idx]))
        assert abs(a[0] / ra - 1) < 2.0 ** -6 and abs(b[0] / rb - 1) < 2.0 ** -6      # four bf16 roundings
    s.set_begin_index(3)                                                              # img2img: the begin row whatever the timestep
    a, b = s._add_noise_coeffs(s.timesteps[7:8].repeat(2), torch.float32)
    ra, rb = ref_alpha_sigma(float(s.sigmas[3]))
    assert len(a) == 2 and abs(a[0] / ra - 1) < 1e-6 and abs(b[1] / rb - 1) < 1e-6


def test_begin_index_reset_and_first_step_move_both_device_words():
    s = _sched(10)
    table, step, begin = s.device_table, s.device_step, s.device_begin
    assert begin.dtype == torch.int32 and int(step) == 0 and int(begin) == 0
    s.set_begin_index(4)
    assert (int(step), int(begin)) == (4, 4) and s.begin_index == 4
    s.reset(6)
    assert (int(step), int(begin), s.step_index) == (6, 6, 6)
    x = torch.randn(1, 4, 4, 4, generator=torch.Generator().manual_seed(0))
    s.step_inplace(torch.zeros_like(x), x)
    assert (int(step), int(begin), s.step_index) == (7, 6, 7)
    # the same length again: every device buffer keeps its address (captured graphs stay valid) and both words rewind
    s.set_timesteps(10, device="cpu")
    assert (s.device_table.data_ptr(), s.device_step.data_ptr(), s.device_begin.data_ptr()) == \
        (table.data_ptr(), step.data_ptr(), begin.data_ptr())
    assert (int(step), int(begin)) == (0, 0) and s.step_index is None
    # without a begin index the first step() finds its row from the timestep and starts the loop there
    hist = s.history(x)
    s.step(torch.zeros_like(x), s.timesteps[5], x)
    assert (int(s.device_step), int(s.device_begin)) == (6, 5) and s.history(x) is hist
    assert s.graph_buffers(x) == (begin.data_ptr(), hist.data_ptr())
    s.set_timesteps(12, device="cpu")
    assert s.device_table.shape == (12, 8) and int(s.device_begin) == 0


def test_a_loop_started_past_row_0_ignores_stale_history():
    """The scheduler's loop from row 5 after a full earlier loop equals the restated loop from row 5 (first step first order)."""
    n = 12
    s = _sched(n, use_karras_sigmas=True)
    sig = s.sigmas.double().numpy()
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(1, 4, 8, 8, generator=g)
    es = [torch.randn(1, 4, 8, 8, generator=g) for _ in range(n)]
    x = x0.clone() * float(sig[0])
    for i in range(n):
        s.step_inplace(es[i], x)
    s.reset(5)
    x = x0.clone() * float(sig[5])
    want = ref_loop(x.double().numpy(), lambda _, i: es[i].double().numpy(), sig, begin=5)
    for i in range(5, n):
        s.step_inplace(es[i], x)
        ref = want[i - 5]
        # (fp32 against float64 over at most seven steps: a few 1e-6; a second-order first step on the stale history is off by O(1))
        assert np.abs(x.double().numpy() - ref).max() <= 1e-4 * (1 + np.abs(ref).max()), i


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
        factory.SDXL_DPM_SCHEDULER, _class_name="DPMSolverMultistepScheduler", _diffusers_version="0.40.0", solver_order=2,
        algorithm_type="dpmsolver++", lambda_min_clipped=-math.inf, variance_type=None)))
    index = {"_class_name": "StableDiffusionXLPipeline", "_diffusers_version": "0.40.0", "force_zeros_for_empty_prompt": True,
             "unet": ["diffusers", "UNet2DConditionModel"], "vae": ["diffusers", "AutoencoderKL"],
             "scheduler": ["diffusers", "DPMSolverMultistepScheduler"], "text_encoder": [None, None], "text_encoder_2": [None, None],
             "tokenizer": [None, None], "tokenizer_2": [None, None]}
    (root / "model_index.json").write_text(json.dumps(index))
    return root


def _inputs(**kw):
    g = torch.Generator().manual_seed(3)
    d = dict(prompt_embeds=torch.randn((1, 77, 64), generator=g).to(bf16), negative_prompt_embeds=torch.randn((1, 77, 64), generator=g).to(bf16),
             pooled_prompt_embeds=torch.randn((1, 64), generator=g).to(bf16),
             negative_pooled_prompt_embeds=torch.randn((1, 64), generator=g).to(bf16),
             latents=torch.randn((1, 4, 16, 16), generator=g).to(bf16), num_inference_steps=4, guidance_scale=5.0, height=128,
             width=128, use_graph=False, output_type="latent")
    d.update(kw)
    return d


def test_pipeline_directory_that_names_the_scheduler_loads_and_runs(tmp_path):
    from diffusers_amd.pipelines import StableDiffusionXLPipeline
    pipe = StableDiffusionXLPipeline.from_pretrained(_sdxl_dir(tmp_path), device="cpu")
    sch = pipe.scheduler
    assert isinstance(sch, DPMSolverMultistepScheduler) and sch.config.use_karras_sigmas and sch.config.steps_offset == 1
    seen = []
    out = pipe(callback_on_step_end=lambda p, i, t, d: seen.append((i, int(t))) or {}, **_inputs()).images
    assert out.shape == (1, 4, 16, 16) and out.dtype == bf16 and torch.isfinite(out.float()).all()
    assert [i for i, _ in seen] == [0, 1, 2, 3] and [t for _, t in seen] == sch.timesteps.tolist() and sch.step_index == 4
    assert int(sch.device_begin) == 0 and int(sch.device_step) == 4
    # the same call again gives the same latents (the history of the first call is not read)
    assert torch.equal(pipe(**_inputs()).images, out)
    # without CFG and with guidance_rescale the step takes a plain model output
    for kw in (dict(guidance_scale=1.0), dict(guidance_rescale=0.7)):
        o = pipe(**_inputs(**kw)).images
        assert torch.isfinite(o.float()).all() and not torch.equal(o, out)
    # denoising_end stops the same loop early
    n = []
    pipe(callback_on_step_end=lambda p, i, t, d: n.append(i) or {}, **_inputs(num_inference_steps=10, denoising_end=0.5))
    assert 0 < len(n) < 10
    for kw in (dict(timesteps=[900, 500, 100]), dict(sigmas=[10.0, 1.0, 0.0])):
        with pytest.raises(ValueError, match="does not support custom timestep or sigma schedules"):
            pipe(**_inputs(**kw))
    # the list of samplers in the refusal of an unknown class names this one
    with pytest.raises(NotImplementedError, match="DPMSolverMultistep"):
        StableDiffusionXLPipeline._load_component(tmp_path, "scheduler", "diffusers", "PNDMScheduler", "cpu", None, "none", False)


def test_abi_tables_carry_the_new_entry_point():
    assert L.FN_IDS["da_dpmpp_2m_step"] == L.FN_COUNT - 1 and "da_dpmpp_2m_step" in L.SIGNATURES
    lib = L.load()
    assert lib.da_version() == L.ABI_VERSION and lib.da_plan_arg_kinds(L.FN_IDS["da_dpmpp_2m_step"]).decode() == "ppppppifliii"
    # host-side argument checks of the entry point (no launch happens for a refused call)
    assert lib.da_dpmpp_2m_step(None, None, None, None, None, None, 0, 0.0, 16, 0, 0, 0, None) == 1
    import diffusers_amd.torch_ops as T
    assert "dpmpp_2m_step" in T.OPS and not torch.ops.mi355x.dpmpp_2m_step.default._schema.is_mutable
