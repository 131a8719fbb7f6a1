"""The latent-consistency step restated, and a CPU stand-in for ``ops.x0_linear_step`` that knows it.

The reference implementation (``scheduling_lcm.py``) is not available to the suite, so its arithmetic is written down once here:

  ``ref_schedule``  the timesteps of ``LCMScheduler.set_timesteps`` (numpy integers)
  ``ref_row``       the eight scalars of a step from 0-d fp32 torch tensors, in the order ``step`` and
                    ``get_scalings_for_boundary_condition_discrete`` form them (sigma_data = 0.5)
  ``ref_step_row``  the op chain of ``step`` on one table row: pred_original_sample, ``denoised = c_out x0 + c_skip sample``,
                    ``prev = sqrt(abar_prev) denoised + sqrt(1 - abar_prev) noise``.  Every torch op on a tensor of dtype T rounds
                    its result to T and a 0-d fp32 scalar promotes nothing; the chain is spelled in fp32 with each rounding explicit
                    (``_rnd``), because torch's CPU kernels do not treat a 0-d scalar operand the same way in every position.

``ref_step_row`` serves twice: ``x0_linear_step`` below wraps it for ``pred_type`` 4-6 (and defers to tests/ops_emulation.py for
0-2), and tests/test_lcm_gpu.py holds the kernel to it bit for bit: the same IEEE operations in the same order."""
import numpy as np
import torch

import ops_emulation

bf16 = torch.bfloat16
PRED_LCM = 4
SD_BETAS = dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)


def ref_alphas_cumprod(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012, N=1000):
    if beta_schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, N, dtype=torch.float32)
    else:
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, N, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def ref_schedule(n, original_inference_steps=50, strength=1.0, N=1000):
    k = N // original_inference_steps
    origin = (np.arange(1, int(original_inference_steps * strength) + 1) * k - 1)[::-1]
    idx = np.floor(np.linspace(0, len(origin), num=n, endpoint=False)).astype(np.int64)
    return origin[idx].astype(np.int64)


def ref_row(alphas_cumprod, t, prev_t, timestep_scaling=10.0, clip=0.0):
    """``prev_t`` None: the last step of a schedule (``prev_sample = denoised``: slots 4, 5 = 1, 0)."""
    a_t = alphas_cumprod[int(t)]
    b_t = 1 - a_t
    scaled = torch.tensor(int(t)) * timestep_scaling
    c_skip = 0.5 ** 2 / (scaled ** 2 + 0.5 ** 2)
    c_out = scaled / (scaled ** 2 + 0.5 ** 2) ** 0.5
    assert c_skip.dtype == torch.float32 and c_out.dtype == torch.float32 and a_t.dtype == torch.float32
    if prev_t is None:
        pa, pb = 1.0, 0.0
    else:
        a_prev = alphas_cumprod[int(prev_t)]
        pa, pb = float(a_prev ** 0.5), float((1 - a_prev) ** 0.5)
    return torch.tensor([float(b_t ** 0.5), float(a_t ** 0.5), float(c_out), float(c_skip), pa, pb, float(clip), float(t)],
                        dtype=torch.float32)


def ref_rows(alphas_cumprod, ts, timestep_scaling=10.0, clip=0.0):
    ts = [int(t) for t in ts]
    return torch.stack([ref_row(alphas_cumprod, t, ts[i + 1] if i + 1 < len(ts) else None, timestep_scaling, clip)
                        for i, t in enumerate(ts)])


def _rnd(v, dtype):
    return v.to(dtype).to(torch.float32)


def ref_combine(model_output, cfg, guidance, dtype):
    """noise_pred = uncond + g (text - uncond), every op in the tensor dtype ([2][n] = (uncond, cond)); fp32 values out."""
    e = model_output.to(torch.float32)
    if not cfg:
        return e.reshape(-1)
    u, c = e.reshape(2, -1)
    g = torch.tensor(guidance, dtype=torch.float32)
    return _rnd(u + _rnd(g * _rnd(c - u, dtype), dtype), dtype)


def ref_denoised(e, s, row, pred, dtype):
    sb_t, sa_t, c_out, c_skip, clip = row[0], row[1], row[2], row[3], row[6]
    if pred == 0:
        x0 = _rnd(_rnd(s - _rnd(sb_t * e, dtype), dtype) / sa_t, dtype)
    elif pred == 1:
        x0 = _rnd(_rnd(sa_t * s, dtype) - _rnd(sb_t * e, dtype), dtype)
    else:
        x0 = e
    if float(clip) > 0:
        x0 = x0.clamp(-float(clip), float(clip))
    return _rnd(_rnd(c_out * x0, dtype) + _rnd(c_skip * s, dtype), dtype)


def ref_step_row(model_output, sample, noise, row, *, cfg=False, guidance=0.0, pred_type=PRED_LCM):
    """One step from a table row; ``noise`` (the step's block) may be None when slot 5 is 0.  Returns the sample's dtype and shape."""
    assert pred_type in (4, 5, 6)
    dtype = sample.dtype
    row = torch.as_tensor(row, dtype=torch.float32)
    e = ref_combine(model_output, cfg, guidance, dtype)
    s = sample.to(torch.float32).reshape(-1)
    den = ref_denoised(e, s, row, pred_type - PRED_LCM, dtype)
    if float(row[5]) == 0.0:
        out = den
    else:
        nz = noise.to(torch.float32).reshape(-1)
        out = _rnd(_rnd(row[4] * den, dtype) + _rnd(row[5] * nz, dtype), dtype)
    return out.to(dtype).view(sample.shape)


# CPU stand-in of ops.x0_linear_step
def x0_linear_step(eps, x, noise, table, step_idx, *, cfg, guidance, out=None, noise_step_stride=0, pred_type=0):
    if pred_type not in (4, 5, 6):
        assert pred_type in (0, 1, 2)
        return ops_emulation.x0_linear_step(eps, x, noise, table, step_idx, cfg=cfg, guidance=guidance, out=out,
                                            noise_step_stride=noise_step_stride, pred_type=pred_type)
    assert noise is not None and noise.dtype == eps.dtype == x.dtype and table.shape[1] == 8
    i, n = int(step_idx), x.numel()
    row = table[i].cpu()
    nz = None
    if float(row[5]) != 0.0:
        nz = noise.reshape(-1)[i * noise_step_stride:i * noise_step_stride + n]
        assert nz.numel() == n
    prev = ref_step_row(eps, x, nz, row, cfg=cfg, guidance=guidance, pred_type=pred_type)
    if out is not None:
        out.copy_(prev)
        return out
    return prev


def install(monkeypatch, ops_module):
    ops_emulation.install(monkeypatch, ops_module)
    monkeypatch.setattr(ops_module, "x0_linear_step", x0_linear_step)


# ----------------------------------------------------------------------------------------------------------------------
# a tiny U-Net with time_cond_proj_dim, and the same model for the unedited oracle
# ----------------------------------------------------------------------------------------------------------------------
COND_DIM = 32
COND_PROJ_GAIN = 8.0     # on the seeded U(-1/sqrt(K), 1/sqrt(K)) weight: the term then moves the output by rel-RMS >= 0.25 (asserted in
                         # tests/test_lcm_cpu.py; a trained cond_proj is not small either)


def cond_unet_case(kind="sdxl", seed=0, guidance_scale=7.5, batch=2):
    """``(config, state_dict, timestep_cond [batch][COND_DIM] bf16)`` of a tiny U-Net with ``time_cond_proj_dim``: the factory's
    seeded weights with ``time_embedding.cond_proj.weight`` scaled by COND_PROJ_GAIN, the pipelines' embedding of one guidance scale."""
    from diffusers_amd import init as dinit
    from diffusers_amd.pipelines import get_guidance_scale_embedding
    from diffusers_amd.unet_2d_condition import UNet2DConditionModel
    cfg = dict(dinit.TINY_SDXL_UNET if kind == "sdxl" else dinit.TINY_SD15_UNET, time_cond_proj_dim=COND_DIM)
    sd = dinit.random_state_dict(dinit.unet_param_shapes(UNet2DConditionModel(**cfg).config), seed=seed)
    key = "time_embedding.cond_proj.weight"
    sd[key] = (sd[key].float() * COND_PROJ_GAIN).to(bf16)
    tc = get_guidance_scale_embedding(torch.tensor(guidance_scale - 1).repeat(batch), embedding_dim=COND_DIM).to(bf16)
    return cfg, sd, tc


def oracle_state_dict(sd, timestep_cond):
    """The fp32 state dict ``oracle.reference_math.unet_forward`` (which has no ``timestep_cond``) computes the same model from:
    ``linear_1(t_emb + P c) = linear_1(t_emb) + W1 (P c)``, so the term is a shift of ``linear_1.bias`` -- for a ``timestep_cond`` whose
    rows are equal, as the pipelines' are."""
    assert all(torch.equal(timestep_cond[0], r) for r in timestep_cond)
    out = {k: v.float() for k, v in sd.items() if k != "time_embedding.cond_proj.weight"}
    pc = sd["time_embedding.cond_proj.weight"].float() @ timestep_cond[0].float()
    out["time_embedding.linear_1.bias"] = out["time_embedding.linear_1.bias"] + out["time_embedding.linear_1.weight"] @ pc
    return out
