"""HeunDiscreteScheduler / KDPM2DiscreteScheduler: the two restatements the tests check against.

1. float64 numpy, from the published algorithms -- Karras et al. 2022, "Elucidating the Design Space of Diffusion-Based Generative
   Models", Alg. 1 without churn (``heun_step``), and k-diffusion's ``sample_dpm_2`` (``dpm2_step``) -- in their textbook form: the
   whole step from x_i, two derivative evaluations, nothing kept between two calls.  The sigma ladder is EulerDiscreteScheduler's
   (its timestep spacings, sigmas interpolated from the training ladder, the Karras / exponential ladder between the interpolated
   extremes, the fractional timestep of a sigma), restated in float64 the way ``test_dpmsolver_cpu.ref_schedule`` restates
   DPM-Solver++'s.  ``entries`` lists the 2n - 1 schedule entries the reference's loop runs and the table row of each.
2. torch fp32, the per-element arithmetic of include/diffusers_amd.h (da_dpmpp_2m_step with DA_PRED_SECOND_ORDER): the same ops
   in the same order, every one a correctly rounded fp32 op, the model output's dtype rounded where the header rounds it
   (``ref_entry``).  The GPU tests compare the kernel with it to the bit; wrapped as ``second_order_step_`` it is the CPU stand-in
   of ``ops.second_order_step_``, installed with ``monkeypatch``."""
import math

import numpy as np
import torch

from test_dpmsolver_cpu import EPS32, ref_sig_all, ref_sigma_to_t   # noqa: F401  (EPS32: the per-step fp32 rule, re-exported)

bf16 = torch.bfloat16
PRED_SECOND_ORDER = 8
PREDS = ("epsilon", "v_prediction", "sample")


# ----------------------------------------------------------------------------------------------------------------------
# 1. float64
# ----------------------------------------------------------------------------------------------------------------------
def ref_training_sigmas(trained_betas=None, **betas):
    if trained_betas is not None:
        ac = np.cumprod(1.0 - np.asarray(trained_betas, dtype=np.float64))
        return np.sqrt((1 - ac) / ac)
    return ref_sig_all(**betas)


def ref_ladder(n, spacing="linspace", ladder="plain", steps_offset=0, sig_all=None, **betas):
    """(timesteps float64 [n], sigmas float64 [n + 1], terminal 0 included)."""
    sig_all = ref_training_sigmas(**betas) if sig_all is None else sig_all
    N = len(sig_all)
    if spacing == "linspace":
        ts = np.linspace(0, N - 1, n)[::-1]
    elif spacing == "leading":
        ts = (np.arange(0, n) * (N // n)).round()[::-1] + steps_offset
    else:
        ts = np.arange(N, 0, -N / n).round() - 1
    ts = ts.astype(np.float32).astype(np.float64)                 # the model timesteps are float32 numbers
    sig = np.interp(ts, np.arange(N), sig_all)
    if ladder != "plain":
        smax, smin = float(sig[0]), float(sig[-1])
        if ladder == "karras":
            rho, ramp = 7.0, np.linspace(0, 1, n)
            sig = (smax ** (1 / rho) + ramp * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
        else:
            sig = np.exp(np.linspace(math.log(smax), math.log(smin), n))
        ts = np.array([ref_sigma_to_t(s, np.log(sig_all)) for s in sig])
    return ts, np.concatenate([sig, [0.0]])


def ref_x0(x, e, sigma, pred):
    """The denoised sample from a model output (k-diffusion's epsilon / v wrappers; ``sample``: the model predicts it)."""
    if pred == "epsilon":
        return x - sigma * e
    if pred == "v_prediction":
        return e * (-sigma / np.sqrt(sigma * sigma + 1)) + x / (sigma * sigma + 1)
    return e


def heun_step(x, model, s, s_next, pred="epsilon", at=(None, None)):
    """Karras et al. Alg. 1, gamma = 0: lines 6-11.  ``model(x, sigma, tag)`` -> the model output; ``at`` tags the two calls."""
    d = (x - ref_x0(x, model(x, s, at[0]), s, pred)) / s
    dt = s_next - s
    x_next = x + dt * d
    if s_next != 0:
        d2 = (x_next - ref_x0(x_next, model(x_next, s_next, at[1]), s_next, pred)) / s_next
        x_next = x + dt * (d + d2) / 2
    return x_next


def dpm2_step(x, model, s, s_next, pred="epsilon", at=(None, None)):
    """k-diffusion sample_dpm_2 without churn."""
    d = (x - ref_x0(x, model(x, s, at[0]), s, pred)) / s
    if s_next == 0:
        return x + d * (s_next - s)
    s_mid = math.exp((math.log(s) + math.log(s_next)) / 2)
    x_2 = x + d * (s_mid - s)
    d_2 = (x_2 - ref_x0(x_2, model(x_2, s_mid, at[1]), s_mid, pred)) / s_mid
    return x + d_2 * (s_next - s)


def euler_step(x, model, s, s_next, pred="epsilon", at=(None, None)):
    return x + (s_next - s) * (x - ref_x0(x, model(x, s, at[0]), s, pred)) / s


STEPS = {"heun": heun_step, "kdpm2": dpm2_step, "euler": euler_step}


def ref_loop(kind, x, model, sig, pred="epsilon", begin=0):
    """The whole loop from step ``begin`` in float64.  ``model(x, sigma, j)``: j = the schedule entry of the call (2 i, 2 i + 1)."""
    x = np.asarray(x, np.float64)
    for i in range(begin, len(sig) - 1):
        x = STEPS[kind](x, model, float(sig[i]), float(sig[i + 1]), pred, at=(2 * i, 2 * i + 1))
    return x


def entries(kind, ts, sig, sig_all):
    """The 2n - 1 entries as table rows, float64 [2n - 1][8]:
    [sigma_eval, c_hist, dt_x, sqrt(sigma_eval^2+1), c_out, sigma_eval^2+1, phase, timestep]."""
    n = len(ts)
    ent = []
    for i in range(n - 1):
        s, s_next = sig[i], sig[i + 1]
        if kind == "heun":
            dt = s_next - s
            ent += [(s, dt / 2, dt, 1, ts[i]), (s_next, 0.0, dt / 2, 2, ts[i + 1])]
        else:
            mid = math.exp((math.log(s) + math.log(s_next)) / 2)
            ent += [(s, 0.0, mid - s, 1, ts[i]), (mid, 0.0, s_next - s, 2, ref_sigma_to_t(mid, np.log(sig_all)))]
    ent.append((sig[n - 1], 0.0, -sig[n - 1], 0, ts[n - 1]))
    rows = np.zeros((len(ent), 8))
    for j, (s, ch, dx, ph, t) in enumerate(ent):
        rows[j] = s, ch, dx, math.sqrt(s * s + 1), -s / math.sqrt(s * s + 1), s * s + 1, ph, t
    return rows


def row_loop(x, model, rows, pred="epsilon"):
    """The loop in the ROW form of the kernel, float64: one history buffer.  ``model(x, sigma, j)`` as in ``ref_loop``."""
    x = np.asarray(x, np.float64)
    m1 = None
    for j, r in enumerate(rows):
        s, c_hist, dt_x, phase = float(r[0]), float(r[1]), float(r[2]), int(r[6])
        d = (x - ref_x0(x, model(x, s, j), s, pred)) / s
        if phase == 1:
            m1 = x + c_hist * d
        x = (m1 if phase == 2 else x) + dt_x * d
    return x


# ----------------------------------------------------------------------------------------------------------------------
# 2. torch fp32: the header's per-element arithmetic
# ----------------------------------------------------------------------------------------------------------------------
def ref_entry(eps, x, m1, row, *, cfg=False, guidance=0.0, pred_type=0):
    """One entry -> (x' in x's dtype, m1' fp32), flat.  ``row``: the 8 fp32 values of the entry.  Every line below is one fp32 op
    of the header, in its order; ``.to(T)`` are the roundings in the model output's dtype T."""
    n = x.numel()
    e = eps.reshape(-1)
    T = e.dtype
    if cfg:
        u, c = e[:n], e[n:]
        e = u + guidance * (c - u)                              # torch rounds c - u, g * (.), u + (.) in T: the kernel's cfg_combine
    e = e.float()
    s = x.reshape(-1).float()
    sigma, c_hist, dt_x, _, c_out, s2p1, phase, _ = (float(v) for v in row)
    if pred_type == 0:
        x0 = s - (sigma * e).to(T).float()
    elif pred_type == 1:
        x0 = (e * c_out).to(T).float() + s / s2p1
    else:
        x0 = e
    d = (s - x0) / sigma
    m1 = m1.reshape(-1)
    m1_new = s + c_hist * d if int(phase) == 1 else m1.clone()
    base = m1 if int(phase) == 2 else s
    return (base + dt_x * d).to(x.dtype), m1_new


def second_order_step_(eps, x, m1, table, step_idx, begin_idx, *, cfg=False, guidance=0.0, pred_type=0):
    """CPU stand-in of ops.second_order_step_ (in place on x and m1)."""
    assert pred_type in (0, 1, 2) and m1.dtype == torch.float32 and m1.numel() == x.numel()
    xn, mn = ref_entry(eps, x, m1, table[int(step_idx)].cpu(), cfg=cfg, guidance=float(guidance), pred_type=pred_type)
    m1.copy_(mn.view(m1.shape))
    x.copy_(xn.view(x.shape))
    return x


def install(monkeypatch, ops_module):
    import inpaint_emulation
    inpaint_emulation.install(monkeypatch, ops_module)
    monkeypatch.setattr(ops_module, "second_order_step_", second_order_step_)
    monkeypatch.setattr(ops_module, "TUNING", False)
