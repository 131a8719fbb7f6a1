"""Schedulers with the reference's SchedulerMixin surface (set_timesteps / scale_model_input / step / timesteps / sigmas /
init_noise_sigma / order / config) whose per-step tensor update is ONE fused HIP kernel (csrc/sampler.hip).

Host side (schedule construction) is numpy / torch-CPU scalar math written to follow the reference formulas exactly:
  EulerDiscreteScheduler          schedulers/scheduling_euler_discrete.py:203-276, :350-481, :326-348, :685-800
  EulerAncestralDiscreteScheduler schedulers/scheduling_euler_ancestral_discrete.py (stochastic: per-step noise, pre-drawn)
  DDIMScheduler                   schedulers/scheduling_ddim.py:212-236, :334-382, :384-514
  DDPMScheduler                   schedulers/scheduling_ddpm.py:348-416, :461-567
  FlowMatchEulerDiscreteScheduler schedulers/scheduling_flow_match_euler_discrete.py:283-382, :423-523
  DPMSolverMultistepScheduler     schedulers/scheduling_dpmsolver_multistep.py (dpmsolver++, order <= 2; float64 host scalars)
  LCMScheduler                    schedulers/scheduling_lcm.py (latent-consistency sampling; per-step noise, pre-drawn)
  HeunDiscreteScheduler           schedulers/scheduling_heun_discrete.py (second order: 2n - 1 entries, one fused two-phase step)
  KDPM2DiscreteScheduler          schedulers/scheduling_k_dpm_2_discrete.py (DPM2; the same step, another table)
Per-step scalars are evaluated once with fp32 torch scalar ops (same ops, same order as the reference evaluates them
every step) and stored in a device table of 8 floats per step; a device-resident step counter selects the row, so a
denoising step is HIP-graph replayable.  ``step_cfg`` additionally fuses the classifier-free-guidance combine.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from . import ops
from .unet_2d_condition import FrozenConfig


@dataclass
class SchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: Optional[torch.Tensor] = None


def _betas(beta_schedule, beta_start, beta_end, n, trained_betas=None):
    if trained_betas is not None:
        return torch.tensor(trained_betas, dtype=torch.float32)
    if beta_schedule == "linear":
        return torch.linspace(beta_start, beta_end, n, dtype=torch.float32)
    if beta_schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    raise NotImplementedError(f"{beta_schedule} is not implemented")


_INT_TIMESTEP_MSG = ("Passing integer indices (e.g. from `enumerate(timesteps)`) as timesteps to `{}.step()` is not supported. "
                     "Make sure to pass one of the `scheduler.timesteps` as a timestep.")

_SERIAL = itertools.count(1)     # one number per scheduler object ever built in this process (graph_token)


class _SchedulerBase:
    order = 1
    init_noise_sigma = 1.0        # (the two Euler classes: a property of their sigmas)
    _defaults: dict = {}
    # what the pipelines ask a scheduler instead of looking at its class
    needs_step_noise = False      # a stochastic sampler: the pipelines pre-draw one randn per step (see EulerAncestralDiscreteScheduler)
    scales_model_input = False    # ``scale_model_input`` divides by sqrt(sigma^2 + 1) (slot 3 of the table row); identity otherwise
    takes_eta = False             # ``step`` / ``step_cfg`` take DDIM's ``eta``
    _tuple_tail = ()              # what ``step(return_dict=False)`` returns after the sample: the reference's (prev,) or (prev, None)
    _bounded_steps = False        # a step past the end of the schedule is refused (it would read a table row that is not there)

    def __init__(self, **kwargs):
        self._serial = next(_SERIAL)
        unknown = set(kwargs) - set(self._defaults)
        if unknown:
            raise TypeError(f"{type(self).__name__}: unexpected config keys {sorted(unknown)}")
        cfg = dict(self._defaults)
        cfg.update(kwargs)
        self.config = FrozenConfig(cfg)
        self._step_index = None
        self._begin_index = None
        self._table = None          # device [n_steps][8] fp32
        self._step_dev = None       # device int32 scalar
        self._device = None
        self._noise_coef = None     # device [n_steps + 1][2] fp32 (add_noise_table)
        self.num_inference_steps = None

    @classmethod
    def from_config(cls, config, **kwargs):
        """``SchedulerMixin.from_config`` (configuration_utils.py:179-260): build from another scheduler's ``config``
        (a mapping; the reference's FrozenDict or this package's FrozenConfig).  Private entries (``_class_name``,
        ``_diffusers_version`` ...) and options this class does not have are dropped, as the reference does when a config
        is handed to a compatible scheduler class; ``kwargs`` override."""
        src = dict(config)
        src.update(kwargs)
        known = {k: (tuple(v) if isinstance(v, list) else v) for k, v in src.items() if k in cls._defaults}
        return cls(**known)

    def _set_vp_ladder(self):
        """The fp32 variance-preserving training ladder of Euler, Euler a, DDIM and DDPM: ``betas`` -> ``alphas`` ->
        ``alphas_cumprod``.  (DPM-Solver++ builds its own in float64 and rounds once: not bit-equal to this one.)"""
        c = self.config
        self.betas = _betas(c.beta_schedule, c.beta_start, c.beta_end, c.num_train_timesteps, c.trained_betas)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)

    # -- reference-compatible index bookkeeping (scheduling_euler_discrete.py:293-324, :640-683) --
    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index
        if self._step_dev is not None and self._step_index is None:
            # the captured step reads the DEVICE counter: the first step of an img2img loop is row `begin_index` of the table
            self._step_dev.fill_(int(begin_index))

    def _add_noise_coeffs(self, timesteps, dtype):
        """(a, b) per sample of ``add_noise`` = a x + b n, each rounded to ``dtype`` as the reference's tensors are."""
        raise NotImplementedError(f"{type(self).__name__}.add_noise is not implemented")

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps) -> torch.Tensor:
        """The reference's ``add_noise`` on bf16 latents, every torch op's bf16 rounding kept (ops.add_noise: one kernel per
        distinct coefficient pair).  The coefficients are computed on the host in the latents' dtype, as the reference does."""
        if original_samples.dtype != torch.bfloat16:
            raise ValueError(f"{type(self).__name__}.add_noise: bf16 latents expected, got {original_samples.dtype}")
        a, b = self._add_noise_coeffs(timesteps, original_samples.dtype)
        B = original_samples.shape[0]
        if len(a) == 1:
            a, b = a * B, b * B
        if len(a) != B:
            raise ValueError(f"add_noise: {len(a)} timesteps for a batch of {B}")
        if len(set(zip(a, b))) == 1:
            return ops.add_noise(original_samples, noise, a[0], b[0])
        return torch.cat([ops.add_noise(original_samples[i:i + 1], noise[i:i + 1], a[i], b[i]) for i in range(B)], 0)

    def add_noise_table(self, dtype=torch.bfloat16) -> torch.Tensor:
        """Engine extension: the ``add_noise`` coefficients of every step of the current schedule as a device table, fp32
        [n_steps + 1][2].  Row ``j`` = the (a, b) of ``_add_noise_coeffs(timesteps[j], dtype)`` with the scheduler standing at step
        ``j`` of a loop with a begin index -- what the inpainting loop's ``add_noise(image_latents, noise, timesteps[i + 1])`` uses
        after step ``i`` -- and the last row is (1, 0): the clean latents after the final step.  ops.inpaint_blend_ picks its row with
        the device step counter.  Refreshed IN PLACE while the schedule length is unchanged (like the step table), so captured
        graphs keep the address."""
        n = len(self.timesteps)
        rows = np.zeros((n + 1, 2), dtype=np.float32)
        keep = (self._begin_index, self._step_index)
        try:
            self._begin_index = 0
            for j in range(n):
                self._step_index = j
                a, b = self._add_noise_coeffs(self.timesteps[j:j + 1], dtype)
                rows[j] = a[0], b[0]
        finally:
            self._begin_index, self._step_index = keep
        rows[n] = 1.0, 0.0
        self._refresh_device("_noise_coef", torch.from_numpy(rows), self.timesteps.device)
        return self._noise_coef

    def _noise_index(self, timesteps):
        """The schedule entry whose sigma ``add_noise`` uses, per timestep (scheduling_euler_discrete.py add_noise and its copies):
        the step at ``begin_index`` (img2img: before the first step), at ``step_index`` (after it), or each timestep's own index
        when no begin index is set."""
        ts = torch.as_tensor(timesteps).reshape(-1).cpu()
        if self.begin_index is None:
            return [self.index_for_timestep(t) for t in ts]
        return [self.step_index if self.step_index is not None else self.begin_index] * ts.shape[0]

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        ts = self._timesteps_host if schedule_timesteps is None else np.asarray(schedule_timesteps.cpu())
        tv = float(timestep) if not torch.is_tensor(timestep) else float(timestep.item())
        idx = np.nonzero(ts == np.float32(tv))[0] if ts.dtype == np.float32 else np.nonzero(ts == tv)[0]
        if len(idx) == 0:
            raise ValueError(f"timestep {tv} is not in the schedule")
        return int(idx[1] if len(idx) > 1 else idx[0])

    def _init_step_index(self, timestep):
        self._step_index = self.index_for_timestep(timestep) if self._begin_index is None else self._begin_index
        self._sync_device_step()

    def _sync_device_step(self):
        if self._step_dev is not None:
            self._step_dev.fill_(int(self._step_index))

    def _refresh_device(self, attr: str, host: torch.Tensor, device, same_device=None) -> bool:
        """Device buffer ``self.<attr>`` <- ``host``: IN PLACE while its shape and device are unchanged, so that HIP graphs that
        captured its address (the pipelines' per-step graph) stay valid across set_timesteps() calls; a new buffer otherwise.
        True when the old buffer was kept."""
        old = getattr(self, attr)
        if same_device is None:
            same_device = old is not None and old.device == device
        if old is not None and same_device and tuple(old.shape) == tuple(host.shape):
            old.copy_(host)
            return True
        setattr(self, attr, host.to(device))
        return False

    def _upload(self, rows: np.ndarray, device):
        dev = torch.device(device) if device is not None else torch.device("cuda")
        host = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32))
        # (the table and the step counter are one pair: a captured step holds both addresses)
        if self._refresh_device("_table", host, dev, same_device=self._device == dev):
            self._step_dev.zero_()
            return
        self._device = dev
        self._step_dev = torch.zeros((), dtype=torch.int32, device=dev)

    def _set_schedule(self, n: int, timesteps: torch.Tensor, timesteps_host: np.ndarray, rows, device):
        """The common tail of every ``set_timesteps``: the new schedule, no step or begin index, the rows uploaded (``None``: the
        caller uploads them itself -- classes whose row math can still refuse the schedule, and DDIM, later, per eta)."""
        self.num_inference_steps = n
        self.timesteps = timesteps
        self._timesteps_host = timesteps_host
        self._step_index = None
        self._begin_index = None
        if rows is not None:
            self._upload(rows, device)

    def _require_schedule(self):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the "
                             "scheduler")

    def _refuse_int_timestep(self, timestep):
        if isinstance(timestep, int) or (torch.is_tensor(timestep) and timestep.dtype in (torch.int32, torch.int64)):
            raise ValueError(_INT_TIMESTEP_MSG.format(type(self).__name__))

    def _before_step(self, timestep):
        """What every fused-step entry point does first: the loop's first call finds its row (host index + device counter)."""
        if self._bounded_steps:
            self._require_schedule()
        if self._step_index is None:
            self._init_step_index(timestep)
        if self._bounded_steps and not 0 <= self._step_index < self.num_inference_steps:
            raise IndexError(f"{type(self).__name__}: step {self._step_index} of a {self.num_inference_steps}-step "
                             "schedule (call set_timesteps() or reset() before another loop)")

    def _advance(self):
        self._step_index += 1
        ops.advance_step(self._step_dev)

    @staticmethod
    def _draw_like_reference(model_output, generator):
        """The reference's randn_tensor inside ``step()``: drawn on the generator's device when one is given, in the model output's
        dtype, then moved to the model output."""
        gdev = generator.device if generator is not None else model_output.device
        return torch.randn(model_output.shape, generator=generator, device=gdev, dtype=model_output.dtype).to(model_output.device)

    def _result(self, prev, return_dict: bool):
        if not return_dict:
            return (prev,) + self._tuple_tail
        return SchedulerOutput(prev_sample=prev)

    # engine extension: handles for graph capture
    @property
    def device_table(self):
        return self._table

    @property
    def device_step(self):
        return self._step_dev

    def set_model_timesteps(self, values) -> None:
        """Engine extension: overwrite column 7 of the device table (what the denoiser's sinusoidal embedding reads in
        the graph-replayed step) with the pipeline's own transform of ``timesteps`` -- e.g. Flux feeds
        ``bf16(bf16(t) / 1000) * 1000`` (pipeline_flux.py:902-907, transformer_flux.py:725)."""
        v = torch.as_tensor(values, dtype=torch.float32).reshape(-1)
        if self._table is None or v.numel() != self._table.shape[0]:
            raise ValueError("set_model_timesteps: call set_timesteps() first; one value per step")
        self._table[:, 7].copy_(v.to(self._table.device))

    def graph_buffers(self, sample):
        """Engine extension: addresses of device state a captured step reads besides the table and the step counter."""
        return ()

    def ensure_table(self, eta: float = 0.0) -> None:
        """Engine extension: have the table a step with this ``eta`` reads in place before ``device_table``'s address is taken.
        Only DDIM's rows depend on a ``step`` argument."""

    def graph_token(self):
        """Engine extension: what a captured step takes from this scheduler BY VALUE -- its class picks the sampler kernel and
        ``scale_model_input``, ``_pred`` is a kernel argument -- and the object's serial.  The addresses of the table and the step
        counter do not identify a scheduler: one built after another was dropped gets buffers of the same sizes, which the caching
        allocator may place where the old ones were.  ``id()`` is reused the same way; the serial never is."""
        return (type(self).__name__, self._serial, getattr(self, "_pred", None))

    def reset(self, index: int = 0):
        """Rewind to step ``index`` (host mirror + device counter)."""
        self._step_index = index
        self._sync_device_step()

    def scale_model_input(self, sample, timestep=None):
        return sample


# ----------------------------------------------------------------------------------------------------------------------
def _sigma_to_t(sigma, log_sigmas):
    """Fractional training timestep whose log sigma equals ``log(sigma)`` (piecewise-linear inverse,
    scheduling_euler_discrete.py:483-517)."""
    log_sigma = np.log(np.maximum(sigma, 1e-10))
    dists = log_sigma - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return ((1 - w) * low_idx + w * high_idx).reshape(np.shape(sigma))


def _respaced_sigmas(smin: float, smax: float, n: int, karras: bool):
    """``n`` sigmas from ``smax`` down to ``smin``: Karras et al. (rho = 7) or uniform in log sigma
    (scheduling_euler_discrete.py:520-585, the same two functions in scheduling_dpmsolver_multistep.py)."""
    if karras:
        rho = 7.0
        ramp = np.linspace(0, 1, n)
        return (smax ** (1 / rho) + ramp * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
    return np.exp(np.linspace(math.log(smax), math.log(smin), n))


def _euler_spaced_timesteps(spacing: str, n_train: int, n: int, steps_offset: int) -> np.ndarray:
    """The float32 model timesteps of an ``n``-step schedule (scheduling_euler_discrete.py:409-431, the same three branches in
    scheduling_euler_ancestral_discrete.py)."""
    if spacing == "linspace":
        return np.linspace(0, n_train - 1, n, dtype=np.float32)[::-1].copy()
    if spacing == "leading":
        ratio = n_train // n
        ts = (np.arange(0, n) * ratio).round()[::-1].copy().astype(np.float32)
        ts += steps_offset
        return ts
    if spacing == "trailing":
        ratio = n_train / n
        ts = (np.arange(n_train, 0, -ratio)).round().copy().astype(np.float32)
        ts -= 1
        return ts
    raise ValueError(f"{spacing} is not supported. Please make sure to choose one of 'linspace', "
                     "'leading' or 'trailing'.")


def _euler_rows(sigmas: torch.Tensor, ts, n: int) -> np.ndarray:
    """[sigma, sigma_next, dt, sqrt(sigma^2+1), c_out, sigma^2+1, 0, timestep] per step from the fp32 CPU sigma ladder (terminal
    value included)."""
    rows = np.zeros((n, 8), dtype=np.float32)
    for i in range(n):
        s, s_next = sigmas[i], sigmas[i + 1]
        rows[i, 0] = float(s)
        rows[i, 1] = float(s_next)
        rows[i, 2] = float(s_next - s)                 # dt, fp32 torch scalar arithmetic as the reference
        rows[i, 3] = float((s ** 2 + 1) ** 0.5)        # scale_model_input denominator
        rows[i, 4] = float(-s / (s ** 2 + 1) ** 0.5)   # v_prediction: c_out (scheduling_euler_discrete.py:767)
        rows[i, 5] = float(s ** 2 + 1)                 # v_prediction: sample / (sigma^2 + 1)
        rows[i, 7] = float(ts[i])
    return rows


class _EulerBase(_SchedulerBase):
    """What EulerDiscreteScheduler and EulerAncestralDiscreteScheduler share (scheduling_euler_discrete.py and its copy
    scheduling_euler_ancestral_discrete.py): the fp32 VP training ladder as k-diffusion sigmas, ``init_noise_sigma``,
    ``scale_model_input``, add_noise = x + n sigma, and a schedule as float32 timesteps with sigmas interpolated from the ladder."""

    scales_model_input = True
    _tuple_tail = (None,)

    def _init_ladder(self):
        c = self.config
        self._set_vp_ladder()
        sig = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).flip(0)
        ts = np.linspace(0, c.num_train_timesteps - 1, c.num_train_timesteps, dtype=float)[::-1].copy()
        self.timesteps = torch.from_numpy(ts).to(dtype=torch.float32)
        self._timesteps_host = self.timesteps.numpy()
        self.sigmas = torch.cat([sig, torch.zeros(1)])
        self.is_scale_input_called = False

    @property
    def init_noise_sigma(self):
        max_sigma = self.sigmas.max()
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return max_sigma
        return (max_sigma ** 2 + 1) ** 0.5

    def _training_sigmas(self) -> np.ndarray:
        return (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()

    def _set_sigma_schedule(self, sig, ts, num_inference_steps, device) -> np.ndarray:
        """Sigma ladder (terminal value included) + model timesteps -> the scheduler's state; returns the Euler rows, which the
        caller uploads (Euler a after putting its own two slots in)."""
        self.sigmas = torch.from_numpy(sig).to(dtype=torch.float32)    # kept on the CPU like the reference
        ts32 = ts.astype(np.float32)
        self._set_schedule(num_inference_steps, torch.from_numpy(ts32).to(device=device), ts32, None, device)
        return _euler_rows(self.sigmas, ts, num_inference_steps)

    def _add_noise_coeffs(self, timesteps, dtype):
        """scheduling_euler_discrete.py add_noise: x + n sigma, sigma of the entry ``_noise_index`` picks; sigmas cast to
        ``dtype``."""
        sig = self.sigmas.to(dtype=dtype)
        idx = self._noise_index(timesteps)
        return [1.0] * len(idx), [float(sig[i]) for i in idx]

    def scale_model_input(self, sample, timestep=None, rep: int = 1):
        if self._step_index is None:
            self._init_step_index(timestep)
        self.is_scale_input_called = True
        return ops.euler_scale_model_input(sample, self._table, self._step_dev, rep=rep)


class EulerDiscreteScheduler(_EulerBase):
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, prediction_type="epsilon", interpolation_type="linear",
                     use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False, sigma_min=None,
                     sigma_max=None, timestep_spacing="linspace", timestep_type="discrete", steps_offset=0,
                     rescale_betas_zero_snr=False, final_sigmas_type="zero")

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.use_beta_sigmas or c.rescale_betas_zero_snr:
            raise NotImplementedError("EulerDiscreteScheduler: beta sigmas / zero-SNR rescaling are not on the hot path")
        if sum([bool(c.use_karras_sigmas), bool(c.use_exponential_sigmas)]) > 1:
            raise ValueError("Only one of `config.use_beta_sigmas`, `config.use_exponential_sigmas`, "
                             "`config.use_karras_sigmas` can be used.")
        if c.timestep_type != "discrete" or c.interpolation_type != "linear":
            raise NotImplementedError("EulerDiscreteScheduler: only discrete timesteps / linear interpolation")
        if c.prediction_type == "original_sample":       # backwards-compatible alias (scheduling_euler_discrete.py:762)
            self._pred = L.PRED_SAMPLE
        elif c.prediction_type in L.PRED_TYPES:
            self._pred = L.PRED_TYPES[c.prediction_type]
        else:
            raise ValueError(f"prediction_type given as {c.prediction_type} must be one of `epsilon`, or `v_prediction`")
        self._init_ladder()

    def set_timesteps(self, num_inference_steps: int = None, device=None, timesteps=None, sigmas=None):
        c = self.config
        # custom schedules (scheduling_euler_discrete.py:378-407): `timesteps` = the model timesteps, sigmas interpolated from the
        # training ladder; `sigmas` = the whole ladder INCLUDING its terminal value, timesteps found by inverting log sigma(t)
        if num_inference_steps is None and timesteps is None and sigmas is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `timesteps` or `sigmas.")
        if num_inference_steps is not None and (timesteps is not None or sigmas is not None):
            raise ValueError("Can only pass one of `num_inference_steps` or `timesteps` or `sigmas`.")
        if timesteps is not None and sigmas is not None:          # scheduling_euler_discrete.py:381-382
            raise ValueError("Only one of `timesteps` or `sigmas` should be set.")
        if timesteps is not None and c.use_karras_sigmas:
            raise ValueError("Cannot set `timesteps` with `config.use_karras_sigmas = True`.")
        if timesteps is not None and c.use_exponential_sigmas:
            raise ValueError("Cannot set `timesteps` with `config.use_exponential_sigmas = True`.")
        if num_inference_steps is None:
            num_inference_steps = len(timesteps) if timesteps is not None else len(sigmas) - 1
        self.num_inference_steps = num_inference_steps
        base = self._training_sigmas()
        log_base = np.log(base)
        if sigmas is not None:
            sig_full = np.array(sigmas).astype(np.float32)
            ts = np.array([_sigma_to_t(s_, log_base) for s_ in sig_full[:-1]])
            self._upload(self._set_sigma_schedule(sig_full, ts, num_inference_steps, device), device)
            return
        if timesteps is not None:
            ts = np.array(timesteps).astype(np.float32)
        else:
            ts = _euler_spaced_timesteps(c.timestep_spacing, c.num_train_timesteps, num_inference_steps, c.steps_offset)
        sig = np.interp(ts, np.arange(0, len(base)), base)
        if c.use_karras_sigmas or c.use_exponential_sigmas:
            # a re-spaced sigma ladder between the interpolated extremes (scheduling_euler_discrete.py:446-452, :520-585);
            # the model then sees fractional timesteps found by inverting log sigma(t) (:483-517).  Host tables only:
            # the step kernel reads sigma / dt / timestep from the same table as before.
            smin = c.sigma_min if c.sigma_min is not None else sig[-1].item()
            smax = c.sigma_max if c.sigma_max is not None else sig[0].item()
            sig = _respaced_sigmas(smin, smax, num_inference_steps, karras=c.use_karras_sigmas)
            ts = np.array([_sigma_to_t(s_, log_base) for s_ in sig])
        if c.final_sigmas_type == "sigma_min":
            last = float(((1 - self.alphas_cumprod[0]) / self.alphas_cumprod[0]) ** 0.5)
        elif c.final_sigmas_type == "zero":
            last = 0
        else:
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {c.final_sigmas_type}")
        sig = np.concatenate([sig, [last]]).astype(np.float32)
        self._upload(self._set_sigma_schedule(sig, ts, num_inference_steps, device), device)

    def _run(self, model_output, sample, cfg, guidance, out=None):
        """The one caller of this class's fused step (da_euler_step)."""
        prev = ops.euler_step(model_output, sample, self._table, self._step_dev, cfg=cfg, guidance=guidance, out=out,
                              pred_type=self._pred)
        self._advance()
        return prev

    def step(self, model_output, timestep, sample, s_churn: float = 0.0, s_tmin: float = 0.0,
             s_tmax: float = float("inf"), s_noise: float = 1.0, generator=None, return_dict: bool = True):
        self._refuse_int_timestep(timestep)
        if s_churn != 0.0:
            raise NotImplementedError("s_churn > 0 (stochastic Euler) is not on the hot path")
        self._before_step(timestep)
        return self._result(self._run(model_output.contiguous(), sample.contiguous(), False, 0.0), return_dict)

    def step_cfg(self, model_output_2b, sample, guidance_scale: float, out=None, cfg: bool = True):
        """Engine extension: CFG combine + Euler step in one kernel; model_output_2b = [uncond ; cond] (``cfg=False``:
        a plain model output -- the ``guidance_scale <= 1`` loop of the pipelines -- with the same in-place ``out``)."""
        self._before_step(self.timesteps[0])
        return self._run(model_output_2b, sample, cfg, float(guidance_scale), out)


# ----------------------------------------------------------------------------------------------------------------------
class EulerAncestralDiscreteScheduler(_EulerBase):
    """schedulers/scheduling_euler_ancestral_discrete.py ("Euler a"): the Euler step towards ``sigma_down`` plus fresh noise of
    scale ``sigma_up`` per step, with sigma_down^2 + sigma_up^2 = sigma_to^2.  The table row is the Euler row with
    dt = sigma_down - sigma in slot 2 and sigma_up in slot 6, both evaluated with fp32 torch scalar ops in the reference's order;
    ONE kernel per step (da_euler_ancestral_step) does the CFG combine, the update and the noise add with the reference's rounding
    points.  ``step()`` draws the noise as the reference does; ``step_cfg`` (the pipelines' captured step) reads row
    ``device_step`` of a pre-drawn ``noise_table`` [steps][numel], so the step stays HIP-graph replayable."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0, rescale_betas_zero_snr=False)
    needs_step_noise = True          # the pipelines pre-draw one randn per step that runs, after every other draw of the call ...
    step_noise_dtype = "model_output"  # ... in the model output's dtype (scheduling_euler_ancestral_discrete.py: randn_tensor(dtype=))
    _bounded_steps = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.rescale_betas_zero_snr:
            raise NotImplementedError("EulerAncestralDiscreteScheduler: zero-SNR rescaling is not on the hot path")
        if c.prediction_type == "sample":
            raise NotImplementedError("prediction_type not implemented yet: sample")
        if c.prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {c.prediction_type} must be one of `epsilon`, or `v_prediction`")
        self._pred = L.PRED_TYPES[c.prediction_type]
        self._init_ladder()

    def set_timesteps(self, num_inference_steps: int, device=None):
        c = self.config
        n = int(num_inference_steps)
        self.num_inference_steps = n
        ts = _euler_spaced_timesteps(c.timestep_spacing, c.num_train_timesteps, n, c.steps_offset)
        base = self._training_sigmas()
        sig = np.interp(ts, np.arange(0, len(base)), base)
        rows = self._set_sigma_schedule(np.concatenate([sig, [0.0]]).astype(np.float32), ts, n, device)
        for i in range(n):
            sigma, sigma_to = self.sigmas[i], self.sigmas[i + 1]      # 0-d fp32 tensors: every op below rounds to fp32
            sigma_up = (sigma_to ** 2 * (sigma ** 2 - sigma_to ** 2) / sigma ** 2) ** 0.5
            sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
            rows[i, 2] = float(sigma_down - sigma)
            rows[i, 6] = float(sigma_up)
        if not np.isfinite(rows).all():
            raise ValueError("EulerAncestralDiscreteScheduler: non-finite step coefficients (a sigma of 0 before the last row?)")
        self._upload(rows, device)

    def _run(self, model_output, sample, noise, noise_step_stride, cfg, guidance, out=None):
        """The one caller of this class's fused step (da_euler_ancestral_step)."""
        prev = ops.euler_ancestral_step(model_output, sample, noise, self._table, self._step_dev, cfg=cfg, guidance=guidance,
                                        out=out, pred_type=self._pred, noise_step_stride=noise_step_stride)
        self._advance()
        return prev

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True):
        self._refuse_int_timestep(timestep)
        self._before_step(timestep)
        noise = self._draw_like_reference(model_output, generator)
        # (the reference upcasts the sample and returns the model output's dtype; here the two share one dtype)
        prev = self._run(model_output.contiguous(), sample.contiguous(), noise.contiguous(), 0, False, 0.0)
        return self._result(prev, return_dict)

    def step_cfg(self, model_output_2b, sample, guidance_scale: float, out=None, cfg: bool = True, noise_table=None):
        """Engine extension: CFG combine (``cfg=False``: a plain model output) + the ancestral step in one kernel, in place when
        ``out`` is the sample.  ``noise_table`` [steps][numel of the sample], in the model output's dtype, holds every step's
        noise drawn up front; the kernel reads the row of the device step counter."""
        if noise_table is None:
            raise ValueError("EulerAncestralDiscreteScheduler.step_cfg needs the pre-drawn `noise_table` [steps][numel]: the "
                             "sampler adds fresh noise every step")
        self._before_step(self.timesteps[0])
        if noise_table.shape[0] != self.num_inference_steps:
            raise ValueError(f"EulerAncestralDiscreteScheduler.step_cfg: `noise_table` has {noise_table.shape[0]} rows for a "
                             f"{self.num_inference_steps}-step schedule")
        return self._run(model_output_2b, sample, noise_table, sample.numel(), cfg, float(guidance_scale), out)


# ----------------------------------------------------------------------------------------------------------------------
class _AlphaBarBase(_SchedulerBase):
    """What DDIMScheduler and DDPMScheduler share: the fp32 VP ladder read at int64 timesteps, add_noise from it, the int64
    timestep spacing, ``step()`` indexed by timestep (the reference's two are stateless), and the fused step da_x0_linear_step."""

    _tuple_tail = (None,)

    def _init_ladder(self):
        self._set_vp_ladder()
        self.timesteps = torch.from_numpy(np.arange(0, self.config.num_train_timesteps)[::-1].copy().astype(np.int64))
        self._timesteps_host = self.timesteps.numpy()

    def _add_noise_coeffs(self, timesteps, dtype):
        """DDIM / DDPM add_noise (scheduling_ddim.py, scheduling_ddpm.py): sqrt(abar_t) and sqrt(1 - abar_t) of abar cast to the
        latents' dtype, each op in that dtype."""
        ac = self.alphas_cumprod.to(dtype=dtype)
        t = torch.as_tensor(timesteps).reshape(-1).cpu().long()
        return [float(v) for v in ac[t] ** 0.5], [float(v) for v in (1 - ac[t]) ** 0.5]

    def _spaced_timesteps(self, n: int, too_many: str = "", unsupported: str = "") -> np.ndarray:
        """The int64 model timesteps of an ``n``-step schedule (scheduling_ddim.py:347-371, the same three branches in
        scheduling_ddpm.py); ``too_many`` / ``unsupported``: how the calling class's wording of the two refusals goes on."""
        c = self.config
        n_train = c.num_train_timesteps
        if n > n_train:
            raise ValueError(f"`num_inference_steps`: {n} cannot be larger than `self.config.train_timesteps`: {n_train}{too_many}")
        self.num_inference_steps = n
        if c.timestep_spacing == "linspace":
            return np.linspace(0, n_train - 1, n).round()[::-1].copy().astype(np.int64)
        if c.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (n_train // n)).round()[::-1].copy().astype(np.int64)
            ts += c.steps_offset
            return ts
        if c.timestep_spacing == "trailing":
            ts = np.round(np.arange(n_train, 0, -(n_train / n))).astype(np.int64)
            ts -= 1
            return ts
        raise ValueError(f"{c.timestep_spacing} is not supported.{unsupported}")

    def _seek(self, timestep) -> int:
        """``step()`` is stateless in the reference (indexed by timestep): honour out-of-order calls."""
        idx = self.index_for_timestep(timestep)
        if idx != self._step_index:
            self._step_index = idx
            self._sync_device_step()
        return idx

    def _run(self, model_output, sample, noise, noise_step_stride, cfg, guidance, out=None):
        """The one caller of these classes' fused step (da_x0_linear_step)."""
        prev = ops.x0_linear_step(model_output, sample, noise, self._table, self._step_dev, cfg=cfg, guidance=guidance, out=out,
                                  noise_step_stride=noise_step_stride, pred_type=self._pred)
        self._advance()
        return prev


class DDIMScheduler(_AlphaBarBase):
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                     prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     clip_sample_range=1.0, sample_max_value=1.0, timestep_spacing="leading",
                     rescale_betas_zero_snr=False)
    takes_eta = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.thresholding or c.rescale_betas_zero_snr:
            raise NotImplementedError("DDIMScheduler: dynamic thresholding / zero-SNR rescaling are not on the hot path")
        if c.prediction_type not in L.PRED_TYPES:
            raise ValueError(f"prediction_type given as {c.prediction_type} must be one of `epsilon`, `sample`, or "
                             "`v_prediction`")
        self._pred = L.PRED_TYPES[c.prediction_type]
        self._init_ladder()
        self.final_alpha_cumprod = torch.tensor(1.0) if c.set_alpha_to_one else self.alphas_cumprod[0]
        self._eta = None

    def _get_variance(self, timestep, prev_timestep):
        a_t = self.alphas_cumprod[timestep]
        a_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        b_t = 1 - a_t
        b_prev = 1 - a_prev
        return (b_prev / b_t) * (1 - a_t / a_prev)

    def set_timesteps(self, num_inference_steps: int, device=None):
        ts = self._spaced_timesteps(
            num_inference_steps,
            f" as the unet model trained with this scheduler can only handle maximal {self.config.num_train_timesteps} timesteps.",
            " Please make sure to choose one of 'leading' or 'trailing'.")
        self._set_schedule(num_inference_steps, torch.from_numpy(ts).to(device), ts, None, device)
        self._device_req = device
        self._eta = None   # table rows are rebuilt lazily for the eta of the first step(); buffers are reused in place

    def _build(self, eta: float):
        c = self.config
        ts = self._timesteps_host
        n = len(ts)
        rows = np.zeros((n, 8), dtype=np.float32)
        for i, t in enumerate(ts):
            t = int(t)
            prev_t = t - c.num_train_timesteps // self.num_inference_steps
            a_t = self.alphas_cumprod[t]
            a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
            b_t = 1 - a_t
            variance = self._get_variance(t, prev_t)
            std = eta * variance ** 0.5
            rows[i, 0] = float(b_t ** 0.5)
            rows[i, 1] = float(a_t ** 0.5)
            rows[i, 2] = float(a_prev ** 0.5)
            rows[i, 3] = float((1 - a_prev - std ** 2) ** 0.5)
            rows[i, 4] = 0.0
            rows[i, 5] = float(std) if eta > 0 else 0.0
            rows[i, 6] = float(c.clip_sample_range) if c.clip_sample else 0.0
            rows[i, 7] = float(t)
        self._upload(rows, self._device_req)
        self._eta = eta

    def _rebuild(self, eta):
        """_build, keeping the step index: refreshing the table in place zeroes the device counter, which a loop that starts past
        step 0 (img2img, scheduler.set_begin_index) must not lose."""
        keep = self._step_index
        self._build(eta)
        self._step_index = keep
        if keep is not None:
            self._sync_device_step()

    def _ensure(self, eta, timestep):
        if self._table is None or self._eta != eta:
            self._rebuild(eta)
        self._before_step(timestep)

    def ensure_table(self, eta: float = 0.0) -> None:
        """Engine extension: the rows of ``eta`` built (in place where the buffers exist) and the loop's first row found, before a
        captured step's key reads ``device_table``'s address -- reading it first builds the rows of eta 0."""
        self._ensure(eta, self.timesteps[0])

    def step(self, model_output, timestep, sample, eta: float = 0.0, use_clipped_model_output: bool = False,
             generator=None, variance_noise=None, return_dict: bool = True):
        self._require_schedule()
        if use_clipped_model_output:
            raise NotImplementedError("use_clipped_model_output is not on the hot path")
        self._ensure(eta, timestep)
        self._seek(timestep)
        noise = None
        if eta > 0:
            if variance_noise is not None and generator is not None:
                raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either "
                                 "`generator` or `variance_noise` stays `None`.")
            noise = variance_noise if variance_noise is not None else self._draw_like_reference(model_output, generator)
        prev = self._run(model_output.contiguous(), sample.contiguous(), noise, 0, False, 0.0)
        return self._result(prev, return_dict)

    def step_cfg(self, model_output_2b, sample, guidance_scale: float, eta: float = 0.0, out=None, cfg: bool = True,
                 noise_table=None):
        """Engine extension: CFG combine (``cfg=False``: plain model output) + DDIM update in one kernel, in place when
        ``out`` is the sample.  ``eta > 0`` needs ``noise_table`` [steps][numel]: every step's variance noise drawn up
        front (the kernel picks the row of the device step counter, so the step stays HIP-graph replayable)."""
        self.ensure_table(eta)
        if eta > 0 and noise_table is None:
            raise ValueError("DDIMScheduler.step_cfg: eta > 0 needs the pre-drawn `noise_table` [steps][numel]")
        return self._run(model_output_2b, sample, noise_table if eta > 0 else None, sample.numel() if eta > 0 else 0, cfg,
                         float(guidance_scale), out)

    def _built(self):
        """(a table nobody asked an eta for yet is eta 0's)"""
        if self._table is None or self._eta is None:
            self._rebuild(0.0)
        return self

    @property
    def device_table(self):
        return self._built()._table

    @property
    def device_step(self):
        return self._built()._step_dev


# ----------------------------------------------------------------------------------------------------------------------
class DDPMScheduler(_AlphaBarBase):
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, variance_type="fixed_small", clip_sample=True, prediction_type="epsilon",
                     thresholding=False, dynamic_thresholding_ratio=0.995, clip_sample_range=1.0,
                     sample_max_value=1.0, timestep_spacing="leading", steps_offset=0, rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.thresholding or c.rescale_betas_zero_snr:
            raise NotImplementedError("DDPMScheduler: dynamic thresholding / zero-SNR rescaling are not on the hot path")
        if c.prediction_type not in L.PRED_TYPES:
            raise ValueError(f"prediction_type given as {c.prediction_type} must be one of `epsilon`, `sample` or "
                             "`v_prediction`  for the DDPMScheduler.")
        self._pred = L.PRED_TYPES[c.prediction_type]
        if c.variance_type not in ("fixed_small", "fixed_large"):
            raise NotImplementedError("DDPMScheduler: only fixed_small / fixed_large variance")
        self._init_ladder()
        self.one = torch.tensor(1.0)
        self.custom_timesteps = False
        self.variance_type = c.variance_type

    def set_timesteps(self, num_inference_steps: int = None, device=None, timesteps=None):
        c = self.config
        if timesteps is not None:
            raise NotImplementedError("custom timesteps are not supported by the HIP DDPMScheduler")
        ts = self._spaced_timesteps(num_inference_steps)
        rows = np.zeros((len(ts), 8), dtype=np.float32)
        for i, t in enumerate(ts):
            t = int(t)
            # previous_timestep() (scheduling_ddpm.py:648-668): the NEXT entry of the schedule, -1 after the last one --
            # not t - n_train // n_steps, which differs for 'linspace' / 'trailing' spacings
            prev_t = int(ts[i + 1]) if i + 1 < len(ts) else -1
            a_t = self.alphas_cumprod[t]
            a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
            b_t = 1 - a_t
            b_prev = 1 - a_prev
            cur_a = a_t / a_prev
            cur_b = 1 - cur_a
            k0 = (a_prev ** 0.5 * cur_b) / b_t
            kx = cur_a ** 0.5 * b_prev / b_t
            var = (1 - a_prev) / (1 - a_t) * cur_b
            var = torch.clamp(var, min=1e-20)
            if self.variance_type == "fixed_large":
                var = cur_b
            rows[i, 0] = float(b_t ** 0.5)
            rows[i, 1] = float(a_t ** 0.5)
            rows[i, 2] = float(k0)
            rows[i, 3] = 0.0
            rows[i, 4] = float(kx)
            rows[i, 5] = float(var ** 0.5) if t > 0 else 0.0
            rows[i, 6] = float(c.clip_sample_range) if c.clip_sample else 0.0
            rows[i, 7] = float(t)
        self._set_schedule(num_inference_steps, torch.from_numpy(ts).to(device), ts, rows, device)

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True, noise=None):
        """scheduling_ddpm.py:461-567.  ``noise`` (engine extension): this step's variance noise instead of a draw from
        ``generator`` (which, like the reference's randn_tensor, draws in the dtype of ``model_output``)."""
        t = int(self._timesteps_host[self._seek(timestep)])
        if t > 0 and noise is None:
            noise = self._draw_like_reference(model_output, generator)
        prev = self._run(model_output.contiguous(), sample.contiguous(), noise if t > 0 else None, 0, False, 0.0)
        return self._result(prev, return_dict)

    def step_inplace(self, model_output, sample, noise_table):
        """Engine extension for HIP-graph replay: the update written over ``sample``; ``noise_table`` [steps][numel]
        holds every step's pre-drawn variance noise, the kernel picks row ``step`` (kn = 0 on the last step)."""
        if self._step_index is None:
            self._step_index = 0
            self._sync_device_step()
        self._run(model_output, sample, noise_table, sample.numel(), False, 0.0, out=sample)
        return sample


# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class LCMSchedulerOutput:
    prev_sample: torch.Tensor
    denoised: Optional[torch.Tensor] = None


def _lcm_rows(alphas_cumprod: torch.Tensor, ts, timestep_scaling: float, clip: float) -> np.ndarray:
    """[sqrt(1 - abar_t), sqrt(abar_t), c_out, c_skip, sqrt(abar_prev), sqrt(1 - abar_prev), clip_range, timestep] per step, every
    scalar a 0-d fp32 torch tensor formed in the order ``LCMScheduler.step`` and ``get_scalings_for_boundary_condition_discrete``
    form it (sigma_data = 0.5).  The last step returns ``denoised``: slots 4, 5 = 1, 0."""
    n = len(ts)
    rows = np.zeros((n, 8), dtype=np.float32)
    for i in range(n):
        t = int(ts[i])
        a_t = alphas_cumprod[t]
        b_t = 1 - a_t
        scaled = torch.tensor(t) * timestep_scaling          # int64 0-d tensor x Python float -> fp32
        c_skip = 0.5 ** 2 / (scaled ** 2 + 0.5 ** 2)
        c_out = scaled / (scaled ** 2 + 0.5 ** 2) ** 0.5
        rows[i, 0] = float(b_t ** 0.5)
        rows[i, 1] = float(a_t ** 0.5)
        rows[i, 2] = float(c_out)
        rows[i, 3] = float(c_skip)
        if i + 1 < n:
            a_prev = alphas_cumprod[int(ts[i + 1])]
            rows[i, 4] = float(a_prev ** 0.5)
            rows[i, 5] = float((1 - a_prev) ** 0.5)
        else:
            rows[i, 4], rows[i, 5] = 1.0, 0.0
        rows[i, 6] = clip
        rows[i, 7] = float(t)
    return rows


class LCMScheduler(_AlphaBarBase):
    """schedulers/scheduling_lcm.py: multistep latent-consistency sampling (Luo et al., "Latent Consistency Models"), 1-8 steps.
    A step predicts x0, applies the consistency boundary condition ``denoised = c_out x0 + c_skip x`` and, on every step but the
    schedule's last, re-noises ``denoised`` to the next timestep with fresh noise.  ONE kernel per step (da_x0_linear_step with
    ``pred_type = PRED_LCM + prediction type``) does the CFG combine and the update with the reference's rounding points.
    ``step()`` draws its noise as the reference does; ``step_cfg`` (the pipelines' captured step) reads row ``device_step`` of a
    pre-drawn ``noise_table`` [steps][numel].  The device table holds the ``n`` step rows and, behind them, the same ``n`` rows with
    slots 4, 5 = 1, 0: the eager ``step()`` reads ``denoised`` for its output from those with a second launch."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                     trained_betas=None, original_inference_steps=50, clip_sample=False, clip_sample_range=1.0,
                     set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon", thresholding=False,
                     dynamic_thresholding_ratio=0.995, sample_max_value=1.0, timestep_spacing="leading",
                     timestep_scaling=10.0, rescale_betas_zero_snr=False)
    needs_step_noise = True
    _bounded_steps = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.thresholding or c.rescale_betas_zero_snr:
            raise NotImplementedError("LCMScheduler: dynamic thresholding / zero-SNR rescaling are not on the hot path")
        if c.prediction_type not in L.PRED_TYPES:
            raise ValueError(f"prediction_type given as {c.prediction_type} must be one of `epsilon`, `sample` or "
                             "`v_prediction` for `LCMScheduler`.")
        self._pred = L.PRED_LCM + L.PRED_TYPES[c.prediction_type]
        self._init_ladder()
        self.final_alpha_cumprod = torch.tensor(1.0) if c.set_alpha_to_one else self.alphas_cumprod[0]
        self.custom_timesteps = False
        self._den_step = None        # device int32: the row the eager step()'s second launch reads (n + step)

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, original_inference_steps: Optional[int] = None,
                      timesteps: Optional[List[int]] = None, strength: float = 1.0):
        c = self.config
        n_train = c.num_train_timesteps
        if num_inference_steps is None and timesteps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `custom_timesteps`.")
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError("Can only pass one of `num_inference_steps` or `custom_timesteps`.")
        orig = original_inference_steps if original_inference_steps is not None else c.original_inference_steps
        if orig > n_train:
            raise ValueError(f"`original_steps`: {orig} cannot be larger than `self.config.train_timesteps`: {n_train} as the unet "
                             f"model trained with this scheduler can only handle maximal {n_train} timesteps.")
        # the schedule the model was distilled on: every k-th training timestep, cut to `strength`
        k = n_train // orig
        origin = np.asarray(list(range(1, int(orig * strength) + 1)), dtype=np.int64) * k - 1
        if timesteps is not None:
            ts = np.array(timesteps, dtype=np.int64)
            if len(ts) == 0 or (np.diff(ts) >= 0).any():
                raise ValueError("`custom_timesteps` must be in descending order.")
            if ts[0] >= n_train:
                raise ValueError(f"`timesteps` must start before `self.config.train_timesteps`: {n_train}.")
            n = len(ts)
            self.custom_timesteps = True
            # img2img: the tail that `strength` leaves, as the reference cuts a custom schedule
            ts = ts[max(n - min(int(n * strength), n), 0):].copy()
        else:
            n = int(num_inference_steps)
            if n > n_train:
                raise ValueError(f"`num_inference_steps`: {n} cannot be larger than `self.config.train_timesteps`: {n_train} as "
                                 f"the unet model trained with this scheduler can only handle maximal {n_train} timesteps.")
            if len(origin) // n < 1:
                raise ValueError(f"The combination of `original_steps x strength`: {orig} x {strength} is smaller than "
                                 f"`num_inference_steps`: {n}. Make sure to either reduce `num_inference_steps` to a value smaller "
                                 f"than {int(orig * strength)} or increase `strength` to a value higher than {float(n / orig)}.")
            if n > orig:
                raise ValueError(f"`num_inference_steps`: {n} cannot be larger than `original_inference_steps`: {orig} because the "
                                 "final timestep schedule will be a subset of the `original_inference_steps`-sized initial "
                                 "timestep schedule.")
            self.custom_timesteps = False
            origin = origin[::-1].copy()
            ts = origin[np.floor(np.linspace(0, len(origin), num=n, endpoint=False)).astype(np.int64)]
        rows = _lcm_rows(self.alphas_cumprod, ts, c.timestep_scaling, float(c.clip_sample_range) if c.clip_sample else 0.0)
        den = rows.copy()
        den[:, 4], den[:, 5] = 1.0, 0.0
        self._set_schedule(len(ts), torch.from_numpy(ts).to(device), ts, np.concatenate([rows, den]), device)
        if self._den_step is None or self._den_step.device != self._step_dev.device:
            self._den_step = torch.zeros_like(self._step_dev)

    def step_noise_draws(self, begin: int, n_steps: int) -> int:
        """Engine extension: how many of the ``n_steps`` steps from schedule entry ``begin`` draw noise -- every step but the
        schedule's last (scheduling_lcm.py step: ``if self.step_index != self.num_inference_steps - 1``)."""
        return max(min(begin + n_steps, self.num_inference_steps - 1) - begin, 0)

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = True):
        self._before_step(timestep)
        i, n = self._step_index, self.num_inference_steps
        model_output, sample = model_output.contiguous(), sample.contiguous()
        # `denoised` first, from row n + i (its slots 4, 5 = 1, 0: no noise read; the pointer only has to be there)
        self._den_step.fill_(n + i)
        denoised = ops.x0_linear_step(model_output, sample, sample, self._table, self._den_step, cfg=False, guidance=0.0,
                                      pred_type=self._pred)
        if i == n - 1:
            self._advance()
            prev = denoised
        else:
            noise = self._draw_like_reference(model_output, generator).contiguous()
            prev = self._run(model_output, sample, noise, 0, False, 0.0)
        if not return_dict:
            return (prev, denoised)
        return LCMSchedulerOutput(prev_sample=prev, denoised=denoised)

    def step_cfg(self, model_output_2b, sample, guidance_scale: float, out=None, cfg: bool = True, noise_table=None):
        """Engine extension: CFG combine (``cfg=False``: a plain model output) + the consistency step in one kernel, in place when
        ``out`` is the sample.  ``noise_table`` [steps][numel of the sample], in the sample's dtype, holds every step's noise drawn
        up front (the last step's row is not read); the kernel picks the row of the device step counter."""
        if noise_table is None:
            raise ValueError("LCMScheduler.step_cfg needs the pre-drawn `noise_table` [steps][numel]: the sampler adds fresh "
                             "noise on every step but the last")
        self._before_step(self.timesteps[0])
        if noise_table.shape[0] != self.num_inference_steps:
            raise ValueError(f"LCMScheduler.step_cfg: `noise_table` has {noise_table.shape[0]} rows for a "
                             f"{self.num_inference_steps}-step schedule")
        return self._run(model_output_2b, sample, noise_table, sample.numel(), cfg, float(guidance_scale), out)


# ----------------------------------------------------------------------------------------------------------------------
class FlowMatchEulerDiscreteScheduler(_SchedulerBase):
    _defaults = dict(num_train_timesteps=1000, shift=1.0, use_dynamic_shifting=False, base_shift=0.5, max_shift=1.15,
                     base_image_seq_len=256, max_image_seq_len=4096, invert_sigmas=False, shift_terminal=None,
                     use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False,
                     time_shift_type="exponential", stochastic_sampling=False)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.use_karras_sigmas or c.use_exponential_sigmas or c.use_beta_sigmas or c.invert_sigmas \
                or c.shift_terminal or c.stochastic_sampling:
            raise NotImplementedError("FlowMatchEulerDiscreteScheduler: option not on the hot path")
        if c.time_shift_type not in {"exponential", "linear"}:
            raise ValueError("`time_shift_type` must either be 'exponential' or 'linear'.")
        ts = np.linspace(1, c.num_train_timesteps, c.num_train_timesteps, dtype=np.float32)[::-1].copy()
        ts = torch.from_numpy(ts).to(dtype=torch.float32)
        sig = ts / c.num_train_timesteps
        if not c.use_dynamic_shifting:
            sig = c.shift * sig / (1 + (c.shift - 1) * sig)
        self.timesteps = sig * c.num_train_timesteps
        self._timesteps_host = self.timesteps.numpy()
        self._shift = c.shift
        self.sigmas = sig
        self.sigma_min = self.sigmas[-1].item()
        self.sigma_max = self.sigmas[0].item()

    @property
    def shift(self):
        return self._shift

    def set_shift(self, shift: float):
        self._shift = shift

    def time_shift(self, mu: float, sigma: float, t):
        if self.config.time_shift_type == "exponential":
            return math.exp(mu) / (math.exp(mu) + (1 / t - 1) ** sigma)
        return mu / (mu + (1 / t - 1) ** sigma)

    def set_timesteps(self, num_inference_steps: int = None, device=None, sigmas: Optional[List[float]] = None,
                      mu: Optional[float] = None, timesteps: Optional[List[float]] = None):
        c = self.config
        if c.use_dynamic_shifting and mu is None:
            raise ValueError("`mu` must be passed when `use_dynamic_shifting` is set to be `True`")
        if timesteps is not None:
            raise NotImplementedError("custom timesteps are not supported by the HIP FlowMatch scheduler")
        if sigmas is not None and num_inference_steps is not None and len(sigmas) != num_inference_steps:
            raise ValueError("`sigmas` and `timesteps` should have the same length as num_inference_steps, if "
                             "`num_inference_steps` is provided")
        if num_inference_steps is None:
            num_inference_steps = len(sigmas)
        if sigmas is None:
            ts = np.linspace(self.sigma_max * c.num_train_timesteps, self.sigma_min * c.num_train_timesteps,
                             num_inference_steps)
            sig = ts / c.num_train_timesteps
        else:
            sig = np.array(sigmas).astype(np.float32)
        if c.use_dynamic_shifting:
            sig = self.time_shift(mu, 1.0, sig)
        else:
            sig = self.shift * sig / (1 + (self.shift - 1) * sig)
        sig_t = torch.from_numpy(np.asarray(sig)).to(dtype=torch.float32)
        ts_t = sig_t * c.num_train_timesteps
        sig_t = torch.cat([sig_t, torch.zeros(1)])
        self.sigmas = sig_t.to(device)          # on the device like the reference's (the other schedulers keep theirs on the CPU)
        rows = np.zeros((num_inference_steps, 8), dtype=np.float32)
        for i in range(num_inference_steps):
            s, s_next = sig_t[i], sig_t[i + 1]
            rows[i, 0] = float(s)
            rows[i, 1] = float(s_next)
            rows[i, 2] = float(s_next - s)
            rows[i, 7] = float(ts_t[i])
        self._set_schedule(num_inference_steps, ts_t.to(device), ts_t.numpy(), rows, device)

    def _add_noise_coeffs(self, timesteps, dtype):
        """scale_noise (scheduling_flow_match_euler_discrete.py): ``sigma * noise + (1.0 - sigma) * sample`` with sigma cast to the
        sample's dtype, so a = dtype(1 - dtype(sigma)) and b = dtype(sigma); sigma of the entry ``_noise_index`` picks."""
        sig = self.sigmas.to(device="cpu", dtype=dtype)
        idx = self._noise_index(timesteps)
        return [float(1.0 - sig[i]) for i in idx], [float(sig[i]) for i in idx]

    def scale_noise(self, sample: torch.Tensor, timestep, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The reference's forward process of flow matching, ``sigma * noise + (1.0 - sigma) * sample`` on bf16 tensors (every torch
        op's bf16 rounding kept: ops.add_noise)."""
        if noise is None:
            raise ValueError("FlowMatchEulerDiscreteScheduler.scale_noise: `noise` is required")
        return self.add_noise(sample, noise, timestep)

    def step(self, model_output, timestep, sample, s_churn: float = 0.0, s_tmin: float = 0.0,
             s_tmax: float = float("inf"), s_noise: float = 1.0, generator=None, per_token_timesteps=None,
             return_dict: bool = True):
        self._refuse_int_timestep(timestep)
        if per_token_timesteps is not None:
            raise NotImplementedError("per_token_timesteps is not on the hot path")
        self._before_step(timestep)
        return self._result(self._run(model_output, sample), return_dict)

    def _run(self, model_output, sample, cfg=False, guidance=0.0, out=None):
        """The one caller of this class's fused step (da_flowmatch_step)."""
        prev = ops.flowmatch_step(model_output, sample, self._table, self._step_dev, cfg=cfg, guidance=guidance, out=out)
        self._advance()
        return prev

    def step_inplace(self, model_output, sample):
        """Engine extension: the update written over ``sample`` (same buffer every HIP-graph replay)."""
        self._before_step(self.timesteps[0])
        self._run(model_output, sample, out=sample)
        return sample

    def step_cfg(self, model_output_2b, sample, guidance_scale: float, out=None):
        self._before_step(self.timesteps[0])
        return self._run(model_output_2b, sample, True, float(guidance_scale), out)


# ----------------------------------------------------------------------------------------------------------------------
class UniPCMultistepScheduler(_SchedulerBase):
    """schedulers/scheduling_unipc_multistep.py in the configuration Wan 2.1 ships (pipeline_wan.py:52-59):
    ``prediction_type="flow_prediction"``, ``use_flow_sigmas=True``, ``flow_shift``, ``solver_order`` <= 2, B(h) solver,
    ``predict_x0``, ``lower_order_final``.  The order-2 predictor-corrector keeps two x0 predictions and the pre-predictor
    sample; the host evaluates the per-step coefficients with the reference's fp32 scalar ops (set_timesteps :428-466,
    _coeffs = :868-905 / :1030-1067) and ONE kernel per step (da_unipc_flow_step) applies them in the reference's
    operation order and rolls the history in place, so the step is HIP-graph replayable."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                     dynamic_thresholding_ratio=0.995, sample_max_value=1.0, predict_x0=True, solver_type="bh2",
                     lower_order_final=True, disable_corrector=[], solver_p=None, use_karras_sigmas=False,
                     use_exponential_sigmas=False, use_beta_sigmas=False, use_flow_sigmas=False, flow_shift=1.0,
                     timestep_spacing="linspace", steps_offset=0, final_sigmas_type="zero",
                     rescale_betas_zero_snr=False, use_dynamic_shifting=False, time_shift_type="exponential",
                     sigma_min=None, sigma_max=None, shift_terminal=None)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.prediction_type != "flow_prediction" or not c.use_flow_sigmas:
            raise NotImplementedError("UniPCMultistepScheduler: only the flow-matching configuration "
                                      "(prediction_type='flow_prediction', use_flow_sigmas=True) is on the hot path")
        if (not c.predict_x0 or c.solver_order not in (1, 2) or c.solver_type not in ("bh1", "bh2") or c.thresholding
                or c.disable_corrector or c.solver_p is not None or c.use_karras_sigmas or c.use_exponential_sigmas
                or c.use_beta_sigmas or c.use_dynamic_shifting or c.shift_terminal or not c.lower_order_final
                or c.final_sigmas_type != "zero"):
            raise NotImplementedError("UniPCMultistepScheduler: unsupported option for the HIP step")
        ts = np.linspace(0, c.num_train_timesteps - 1, c.num_train_timesteps, dtype=np.float32)[::-1].copy()
        self.timesteps = torch.from_numpy(ts)
        self._timesteps_host = ts
        self._coef = None
        self._hist = None
        self.sigmas = None

    def _coeffs(self, sigma_t, sigma_s0, hist_sigmas, order):
        """The scalar part of multistep_uni_{p,c}_bh_update, fp32 torch ops in the reference's order."""
        alpha_t, alpha_s0 = 1 - sigma_t, 1 - sigma_s0
        lambda_t = torch.log(alpha_t) - torch.log(sigma_t)
        lambda_s0 = torch.log(alpha_s0) - torch.log(sigma_s0)
        h = lambda_t - lambda_s0
        rks = [((torch.log(1 - s_) - torch.log(s_)) - lambda_s0) / h for s_ in hist_sigmas[: order - 1]]
        rks.append(torch.ones(()))
        rks = torch.stack(rks)
        hh = -h
        h_phi_1 = torch.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        B_h = hh if self.config.solver_type == "bh1" else torch.expm1(hh)
        R, b, fact = [], [], 1
        for i in range(1, order + 1):
            R.append(torch.pow(rks, i - 1))
            b.append(h_phi_k * fact / B_h)
            fact *= i + 1
            h_phi_k = h_phi_k / hh - 1 / fact
        return sigma_t / sigma_s0, alpha_t * h_phi_1, alpha_t * B_h, rks, torch.stack(R), torch.stack(b)

    def set_timesteps(self, num_inference_steps: int = None, device=None, sigmas=None, mu=None):
        c = self.config
        if sigmas is not None:
            raise NotImplementedError("custom sigmas are not supported by the HIP UniPC scheduler")
        n = num_inference_steps
        sig = np.linspace(1, 1 / c.num_train_timesteps, n + 1)[:-1]
        sig = c.flow_shift * sig / (1 + (c.flow_shift - 1) * sig)
        if np.fabs(sig[0] - 1) < 1e-6:
            sig[0] -= 1e-6
        ts = (sig * c.num_train_timesteps).copy()
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0]]).astype(np.float32))
        timesteps = torch.from_numpy(ts).to(device=device, dtype=torch.int64)
        timesteps_host = timesteps.cpu().numpy()        # (what the device holds: the int64 cast truncates)
        S = self.sigmas
        coef = np.zeros((n, 16), dtype=np.float32)
        rows = np.zeros((n, 8), dtype=np.float32)
        lower, prev_order = 0, None
        for i in range(n):
            coef[i, 0] = float(S[i])
            if i > 0:      # corrector of step i runs with the predictor order of step i-1 (step(): :1262-1270)
                oc = prev_order
                c1, c2, c3, rks, R, b = self._coeffs(S[i], S[i - 1], [S[i - (k + 1)] for k in range(1, oc)], oc)
                rhos = torch.ones(1) * 0.5 if oc == 1 else torch.linalg.solve(R, b)
                coef[i, 1], coef[i, 2] = 1.0, float(oc)
                coef[i, 3], coef[i, 4], coef[i, 5] = float(c1), float(c2), float(c3)
                coef[i, 6] = float(rks[0]) if oc == 2 else 1.0
                coef[i, 7] = float(rhos[0]) if oc == 2 else 0.0
                coef[i, 8] = float(rhos[-1])
            op = min(min(c.solver_order, n - i), lower + 1)
            c1, c2, c3, rks, _, _ = self._coeffs(S[i + 1], S[i], [S[i - k] for k in range(1, op)], op)
            coef[i, 9], coef[i, 10], coef[i, 11], coef[i, 12] = float(op), float(c1), float(c2), float(c3)
            coef[i, 13] = float(rks[0]) if op == 2 else 1.0
            rows[i, 0], rows[i, 1], rows[i, 7] = float(S[i]), float(S[i + 1]), float(timesteps_host[i])
            prev_order = op
            if lower < c.solver_order:
                lower += 1
        self._set_schedule(n, timesteps, timesteps_host, rows, device)
        self._refresh_device("_coef", torch.from_numpy(coef), self._table.device)
        # the history tensors are kept (a captured graph holds their addresses); their stale content is never used:
        # step 0 runs without corrector at order 1, and every later read was written by an earlier step

    def _history(self, sample):
        if self._hist is None or self._hist[0].shape != sample.shape or self._hist[0].dtype != sample.dtype:
            self._hist = tuple(torch.zeros_like(sample) for _ in range(3))     # last_sample, m1, m2
        return self._hist

    def graph_buffers(self, sample):
        return (self._coef.data_ptr(),) + tuple(h.data_ptr() for h in self._history(sample))

    def _run(self, model_output, sample, cfg=False, guidance=0.0):
        """The one caller of this class's fused step (da_unipc_flow_step): ``sample`` is updated in place."""
        last, m1, m2 = self._history(sample)
        ops.unipc_flow_step_(model_output, sample, last, m1, m2, self._coef, self._step_dev, cfg=cfg, guidance=guidance)
        self._advance()
        return sample

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        self._require_schedule()
        self._before_step(timestep)
        return self._result(self._run(model_output, sample.clone()), return_dict)

    def step_cfg(self, model_output_2b, sample, guidance_scale: float, out=None):
        """Engine extension: CFG combine + UniPC step, written over ``sample`` (graph replay)."""
        self._before_step(self.timesteps[0])
        if out is not None and out.data_ptr() != sample.data_ptr():
            raise ValueError("UniPC step_cfg updates `sample` in place")
        return self._run(model_output_2b, sample, True, float(guidance_scale))

    def step_inplace(self, model_output, sample):
        self._before_step(self.timesteps[0])
        return self._run(model_output, sample)


# ----------------------------------------------------------------------------------------------------------------------
def _vp_alpha_sigma(s):
    """(alpha, sigma) of the variance-preserving form of a k-diffusion sigma ``s`` (float64):
    alpha = 1 / sqrt(s^2 + 1), sigma = s alpha (scheduling_dpmsolver_multistep.py _sigma_to_alpha_sigma_t)."""
    s = np.float64(s)
    a = 1.0 / np.sqrt(s * s + 1.0)
    return a, s * a


def _vp_lambda(s):
    """Half log-SNR log(alpha) - log(sigma) of a sigma > 0 (float64)."""
    a, b = _vp_alpha_sigma(s)
    return np.log(a) - np.log(b)


class DPMSolverMultistepScheduler(_SchedulerBase):
    """schedulers/scheduling_dpmsolver_multistep.py with ``algorithm_type="dpmsolver++"``, ``solver_order`` <= 2 -- "DPM++ 2M",
    usually run with Karras sigmas.  Every scalar of a step (alpha / sigma of the current row, the first-order pair and, where
    the row may run second order, the D1 coefficient with ``1 / r0`` and the midpoint / heun factor folded in) is evaluated on
    the host in float64 and stored as one fp32 row of the device table; ONE kernel per step (da_dpmpp_2m_step) converts the model
    output to x0, applies the row and rolls the fp32 x0 history in place, so the step is HIP-graph replayable.  The first step of
    a loop runs first order wherever it starts: the kernel compares the device step counter with a second device word, the loop's
    begin row, which ``reset`` / ``set_begin_index`` / the first ``step`` write."""

    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                     euler_at_final=False, use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False,
                     use_lu_lambdas=False, use_flow_sigmas=False, flow_shift=1.0, final_sigmas_type="zero",
                     lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0,
                     rescale_betas_zero_snr=False, use_dynamic_shifting=False, time_shift_type="exponential")
    _bounded_steps = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        name = type(self).__name__
        if c.algorithm_type != "dpmsolver++":
            raise NotImplementedError(f"{name}: algorithm_type={c.algorithm_type!r} is not implemented (only 'dpmsolver++')")
        if c.solver_order not in (1, 2):
            raise NotImplementedError(f"{name}: solver_order={c.solver_order} is not implemented (1 or 2)")
        if c.solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"{name}: solver_type={c.solver_type!r} is not implemented ('midpoint' or 'heun')")
        if c.prediction_type not in L.PRED_TYPES:
            raise NotImplementedError(f"{name}: prediction_type={c.prediction_type!r} is not implemented "
                                      "('epsilon', 'v_prediction' or 'sample')")
        for flag in ("thresholding", "use_beta_sigmas", "use_lu_lambdas", "use_flow_sigmas", "rescale_betas_zero_snr",
                     "use_dynamic_shifting"):
            if c[flag]:
                raise NotImplementedError(f"{name}: {flag}=True is not implemented")
        if not math.isinf(c.lambda_min_clipped) or c.lambda_min_clipped > 0:
            raise NotImplementedError(f"{name}: lambda_min_clipped={c.lambda_min_clipped} is not implemented (-inf only)")
        if c.variance_type is not None:
            raise NotImplementedError(f"{name}: variance_type={c.variance_type!r} is not implemented (None only)")
        if c.use_karras_sigmas and c.use_exponential_sigmas:
            raise ValueError("Only one of `config.use_beta_sigmas`, `config.use_exponential_sigmas`, "
                             "`config.use_karras_sigmas` can be used.")
        if c.final_sigmas_type not in ("zero", "sigma_min"):
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {c.final_sigmas_type}")
        self._pred = L.PRED_TYPES[c.prediction_type]
        # the training ladder in float64 like every other scalar of this class: in fp32, 1 - alphas_cumprod[0] cancels down to
        # four digits and sigma_min of the SD betas comes out 1.3e-5 high (0.0291675 for 0.0291672)
        if c.trained_betas is not None:
            betas = np.asarray(c.trained_betas, dtype=np.float64)
        elif c.beta_schedule == "linear":
            betas = np.linspace(c.beta_start, c.beta_end, c.num_train_timesteps, dtype=np.float64)
        elif c.beta_schedule == "scaled_linear":
            betas = np.linspace(c.beta_start ** 0.5, c.beta_end ** 0.5, c.num_train_timesteps, dtype=np.float64) ** 2
        else:
            raise NotImplementedError(f"{c.beta_schedule} is not implemented")
        ac = np.cumprod(1.0 - betas)
        self._sig_all = np.sqrt((1.0 - ac) / ac)
        self.betas = torch.from_numpy(betas).float()
        self.alphas = 1.0 - self.betas
        # (the float64 product rounded once: not bit-equal to the fp32 cumprod the other schedulers hold for the same betas)
        self.alphas_cumprod = torch.from_numpy(ac).float()
        ts = np.arange(0, c.num_train_timesteps)[::-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts)
        self._timesteps_host = ts
        self.sigmas = torch.from_numpy(np.concatenate([self._sig_all[::-1], [0.0]]).astype(np.float32))
        self._begin_dev = None      # device int32: the row the running loop started at
        self._hist = None           # fp32 x0 prediction of the previous step
        self.second_order_rows = None

    def set_timesteps(self, num_inference_steps: int = None, device=None, mu=None, timesteps=None):
        c = self.config
        if timesteps is not None:
            raise NotImplementedError("custom timesteps are not supported by the HIP DPMSolverMultistepScheduler")
        if num_inference_steps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `timesteps`.")
        n, N = int(num_inference_steps), c.num_train_timesteps
        if c.timestep_spacing == "linspace":
            ts = np.linspace(0, N - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif c.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (N // (n + 1))).round()[::-1][:-1].copy().astype(np.int64)
            ts += c.steps_offset
        elif c.timestep_spacing == "trailing":
            ts = np.arange(N, 0, -N / n).round().copy().astype(np.int64)
            ts -= 1
        else:
            raise ValueError(f"{c.timestep_spacing} is not supported. Please make sure to choose one of 'linspace', "
                             "'leading' or 'trailing'.")
        sig_all = self._sig_all
        if c.use_karras_sigmas or c.use_exponential_sigmas:
            sig = _respaced_sigmas(float(sig_all[0]), float(sig_all[-1]), n, karras=c.use_karras_sigmas)
            log_sigmas = np.log(sig_all)
            ts = np.array([_sigma_to_t(s_, log_sigmas) for s_ in sig]).round().astype(np.int64)
        else:
            sig = np.interp(ts, np.arange(0, N), sig_all)
        last = 0.0 if c.final_sigmas_type == "zero" else float(sig_all[0])
        sig = np.concatenate([sig, [last]]).astype(np.float32)
        self.sigmas = torch.from_numpy(sig)                      # kept on the CPU like the reference
        self._set_schedule(n, torch.from_numpy(ts).to(device=device, dtype=torch.int64), ts, None, device)
        rows = self._rows(sig, ts)
        self.second_order_rows = [bool(r[6]) for r in rows]
        self._upload(rows, device)

    def _rows(self, sig: np.ndarray, ts: np.ndarray) -> np.ndarray:
        """[alpha_s0, sigma_s0, cx, c0, cd, 0, second_order_allowed, timestep] per step, float64 host math on the fp32 sigmas.
        Row i steps from s0 = sig[i] to t = sig[i+1], h = lambda_t - lambda_s0:
          first order   x' = (sigma_t / sigma_s0) x - alpha_t (exp(-h) - 1) x0                     -> cx x + c0 x0
          second order  + cd (x0 - m1),  cd = -0.5 alpha_t (exp(-h) - 1) / r0 (midpoint) | alpha_t ((exp(-h) - 1) / h + 1) / r0 (heun),
                        r0 = (lambda_s0 - lambda_s1) / h, s1 = sig[i-1]
        A final sigma of 0 has h = inf: exp(-h) - 1 = -1 and sigma_t = 0 are set here, the row is x' = x0, nothing non-finite is
        stored.  A step of no length (t = s0) is the identity row.  A row may run second order unless solver_order == 1, it is
        row 0, or it is the last row and (euler_at_final or the final sigma is 0 or (lower_order_final and fewer than 15 steps));
        the kernel also runs the loop's first step first order."""
        c = self.config
        n = len(ts)
        rows = np.zeros((n, 8), dtype=np.float64)
        for i in range(n):
            s0, t = sig[i], sig[i + 1]
            a0, b0 = _vp_alpha_sigma(s0)
            at, bt = _vp_alpha_sigma(t)
            if t == 0:
                h, em1 = np.inf, -1.0
            else:
                h = _vp_lambda(t) - _vp_lambda(s0)
                em1 = np.exp(-h) - 1.0
            rows[i, :4] = a0, b0, bt / b0, -at * em1
            rows[i, 7] = float(ts[i])
            if h == 0:      # a step of no length (a ladder that ends at sigma_min, then final_sigmas_type="sigma_min"): x' = x
                continue
            last_first = i == n - 1 and (c.euler_at_final or c.final_sigmas_type == "zero" or (c.lower_order_final and n < 15))
            if c.solver_order == 2 and i > 0 and not last_first:
                r0 = (_vp_lambda(s0) - _vp_lambda(sig[i - 1])) / h
                d1 = -0.5 * at * em1 if c.solver_type == "midpoint" else at * (em1 / h + 1.0)
                rows[i, 4], rows[i, 6] = d1 / r0, 1.0
        rows = rows.astype(np.float32)
        if not np.isfinite(rows).all():
            raise ValueError("DPMSolverMultistepScheduler: non-finite step coefficients (repeated sigmas in the schedule?)")
        return rows

    def _upload(self, rows, device):
        super()._upload(rows, device)
        self._refresh_device("_begin_dev", torch.zeros((), dtype=torch.int32), self._table.device)

    def _sync_device_step(self):
        """reset() and the first step() of a loop come through here: the loop starts at this row."""
        super()._sync_device_step()
        if self._begin_dev is not None:
            self._begin_dev.fill_(int(self._step_index))

    def set_begin_index(self, begin_index: int = 0):
        super().set_begin_index(begin_index)
        if self._begin_dev is not None and self._step_index is None:
            self._begin_dev.fill_(int(begin_index))

    @property
    def device_begin(self):
        return self._begin_dev

    def history(self, sample):
        """The fp32 x0 history buffer for samples of this size (allocated once: captured graphs hold its address).  Its content
        is never read by the first step of a loop, so it is not cleared between loops."""
        if self._hist is None or self._hist.shape != sample.shape or self._hist.device != sample.device:
            self._hist = torch.zeros(sample.shape, dtype=torch.float32, device=sample.device)
        return self._hist

    def graph_buffers(self, sample):
        return (self._begin_dev.data_ptr(), self.history(sample).data_ptr())

    def _add_noise_coeffs(self, timesteps, dtype):
        """scheduling_dpmsolver_multistep.py add_noise: alpha_t x + sigma_t n of the sigma ``_noise_index`` picks; ops in ``dtype``."""
        s = self.sigmas.to(dtype=dtype)[self._noise_index(timesteps)]
        a = 1 / ((s ** 2 + 1) ** 0.5)
        b = s * a
        return [float(v) for v in a], [float(v) for v in b]

    def _run(self, model_output, sample, cfg, guidance_scale):
        """The one caller of this class's fused step (da_dpmpp_2m_step): ``sample`` is updated in place."""
        ops.dpmpp_2m_step_(model_output, sample, self.history(sample), self._table, self._step_dev, self._begin_dev, cfg=cfg,
                           guidance=float(guidance_scale), pred_type=self._pred)
        self._advance()
        return sample

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict: bool = True):
        """``generator`` / ``variance_noise`` belong to the SDE variants and are unused by dpmsolver++."""
        self._before_step(timestep)
        return self._result(self._run(model_output.contiguous(), sample.contiguous().clone(), False, 0.0), return_dict)

    def step_cfg(self, model_output_2b, sample, guidance_scale: float, out=None, cfg: bool = True):
        """Engine extension: CFG combine (``cfg=False``: a plain model output) + the step, written over ``sample`` (graph replay)."""
        if out is not None and out.data_ptr() != sample.data_ptr():
            raise ValueError("DPMSolverMultistepScheduler.step_cfg updates `sample` in place")
        self._before_step(self.timesteps[0])
        return self._run(model_output_2b, sample, cfg, guidance_scale)

    def step_inplace(self, model_output, sample):
        self._before_step(self.timesteps[0])
        return self._run(model_output, sample, False, 0.0)


# ----------------------------------------------------------------------------------------------------------------------
class _SecondOrderBase(_EulerBase):
    """What HeunDiscreteScheduler and KDPM2DiscreteScheduler share: second-order single-step samplers the reference runs as
    2n - 1 schedule entries for n steps -- predictor and corrector alternating, one model call per entry, the step into sigma = 0 a
    single Euler entry.  Every entry is one row of the device table,
      [sigma_eval, c_hist, dt_x, sqrt(sigma_eval^2+1), c_out, sigma_eval^2+1, phase, timestep]      phase 0 Euler, 1 predictor, 2 corrector
    (slots 0, 3, 4, 5, 7 as the Euler row, so ``scale_model_input`` and the U-Net's sinusoid read it unchanged), and ONE kernel
    (da_dpmpp_2m_step with DA_PRED_SECOND_ORDER) serves every entry: with d = (x - x0) / sigma_eval a predictor stores the history
    m1 = x + c_hist d and moves x by dt_x d, a corrector writes x = m1 + dt_x d.  The pipelines' captured step is replayed once per
    entry and never learns which kind it ran.  The sigmas are the ladder EulerDiscreteScheduler forms for the same options, evaluated
    -- with every other scalar of the rows -- in float64 on the host and rounded once to fp32 (as DPMSolverMultistepScheduler does).
    ``timesteps`` and ``sigmas`` have one value per entry (``sigmas`` the terminal 0 behind them), so ``add_noise``,
    ``add_noise_table`` and ``scale_model_input`` work on the noise level the latents of an entry actually have."""

    order = 2
    _common_defaults = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="linear", trained_betas=None,
                            prediction_type="epsilon", use_karras_sigmas=False, use_exponential_sigmas=False, use_beta_sigmas=False,
                            timestep_spacing="linspace", steps_offset=0)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        name = type(self).__name__
        if c.use_beta_sigmas:
            raise NotImplementedError(f"{name}: use_beta_sigmas=True is not implemented")
        if c.get("clip_sample", False):
            raise NotImplementedError(f"{name}: clip_sample=True is not implemented")
        if c.use_karras_sigmas and c.use_exponential_sigmas:
            raise ValueError("Only one of `config.use_beta_sigmas`, `config.use_exponential_sigmas`, "
                             "`config.use_karras_sigmas` can be used.")
        if c.prediction_type not in L.PRED_TYPES:
            raise ValueError(f"{name}: prediction_type={c.prediction_type!r} is not implemented ('epsilon', 'v_prediction' or "
                             "'sample')")
        self._pred = L.PRED_TYPES[c.prediction_type]
        if c.trained_betas is not None:
            betas = np.asarray(c.trained_betas, dtype=np.float64)
        elif c.beta_schedule == "linear":
            betas = np.linspace(c.beta_start, c.beta_end, c.num_train_timesteps, dtype=np.float64)
        elif c.beta_schedule == "scaled_linear":
            betas = np.linspace(c.beta_start ** 0.5, c.beta_end ** 0.5, c.num_train_timesteps, dtype=np.float64) ** 2
        else:
            raise NotImplementedError(f"{name}: beta_schedule={c.beta_schedule!r} is not implemented ('linear' or 'scaled_linear')")
        ac = np.cumprod(1.0 - betas)
        self._sig_all = np.sqrt((1.0 - ac) / ac)            # float64 training ladder, ascending
        self.betas = torch.from_numpy(betas).float()
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.from_numpy(ac).float()
        n_train = len(betas)
        ts = np.linspace(0, n_train - 1, n_train, dtype=float)[::-1].copy()
        self.timesteps = torch.from_numpy(ts).to(dtype=torch.float32)
        self._timesteps_host = self.timesteps.numpy()
        self.sigmas = torch.from_numpy(np.concatenate([self._sig_all[::-1], [0.0]]).astype(np.float32))
        self.is_scale_input_called = False
        self._hist = None           # fp32: what a predictor entry leaves for its corrector
        self.phases = None          # per entry: 0 Euler, 1 predictor, 2 corrector

    # -- the schedule ----------------------------------------------------------------------------------------------------
    def _ladder(self, n: int):
        """(sigmas float64 [n + 1] with the terminal 0, timesteps float64 [n]) as EulerDiscreteScheduler.set_timesteps forms them."""
        c = self.config
        base = self._sig_all
        ts = _euler_spaced_timesteps(c.timestep_spacing, len(base), n, c.steps_offset).astype(np.float64)
        sig = np.interp(ts, np.arange(0, len(base)), base)
        if c.use_karras_sigmas or c.use_exponential_sigmas:
            sig = _respaced_sigmas(float(sig[-1]), float(sig[0]), n, karras=c.use_karras_sigmas)     # between the extremes
            ts = np.array([float(_sigma_to_t(s_, np.log(base))) for s_ in sig])
        return np.concatenate([sig, [0.0]]), ts

    def _entries(self, sig: np.ndarray, ts: np.ndarray):
        """Per entry (sigma_eval, c_hist, dt_x, phase, timestep) in float64; the subclass says what its two phases are."""
        raise NotImplementedError

    def set_timesteps(self, num_inference_steps: int = None, device=None, num_train_timesteps=None, timesteps=None):
        name = type(self).__name__
        if timesteps is not None:
            raise NotImplementedError(f"custom timesteps are not supported by the HIP {name}")
        if num_inference_steps is None or int(num_inference_steps) < 1:
            raise ValueError("`num_inference_steps` must be a positive number of steps.")
        n = int(num_inference_steps)
        sig, ts = self._ladder(n)
        if not (np.diff(sig) < 0).all():
            raise ValueError(f"{name}: the sigmas of a {n}-step schedule do not decrease strictly (more steps than training "
                             "timesteps?)")
        ent = np.asarray(self._entries(sig, ts), dtype=np.float64)           # [2n - 1][5]
        s = ent[:, 0]
        rows = np.zeros((len(ent), 8), dtype=np.float64)
        rows[:, 0], rows[:, 1], rows[:, 2] = s, ent[:, 1], ent[:, 2]
        rows[:, 3], rows[:, 4], rows[:, 5] = np.sqrt(s * s + 1.0), -s / np.sqrt(s * s + 1.0), s * s + 1.0
        rows[:, 6], rows[:, 7] = ent[:, 3], ent[:, 4]
        rows = rows.astype(np.float32)
        if not np.isfinite(rows).all():
            raise ValueError(f"{name}: non-finite step coefficients")
        self.phases = [int(p) for p in ent[:, 3]]
        self.sigmas = torch.from_numpy(np.concatenate([s, [0.0]]).astype(np.float32))    # per entry; kept on the CPU
        ts32 = ent[:, 4].astype(np.float32)
        self._set_schedule(n, torch.from_numpy(ts32).to(device=device), ts32, rows, device)

    # -- index bookkeeping -----------------------------------------------------------------------------------------------
    @property
    def state_in_first_order(self) -> bool:
        """True where the next entry is a predictor (or the final Euler entry), as the reference's ``dt is None``."""
        return self._step_index is None or self._step_index % 2 == 0

    def _refuse_corrector_start(self, index: int):
        if int(index) % 2:
            raise ValueError(f"{type(self).__name__}: a loop cannot begin at entry {index}, a corrector (it would read a history "
                             "no predictor wrote); begin indices are even")

    def set_begin_index(self, begin_index: int = 0):
        self._refuse_corrector_start(begin_index)
        super().set_begin_index(begin_index)

    def reset(self, index: int = 0):
        self._refuse_corrector_start(index)
        super().reset(index)

    def _before_step(self, timestep):
        self._require_schedule()
        if self._step_index is None:
            self._init_step_index(timestep)
        if not 0 <= self._step_index < len(self._timesteps_host):
            raise IndexError(f"{type(self).__name__}: entry {self._step_index} of a schedule of {len(self._timesteps_host)} "
                             "entries (call set_timesteps() or reset() before another loop)")

    def history(self, sample):
        """The fp32 history buffer for samples of this size (allocated once: captured graphs hold its address).  A corrector reads
        what the predictor in front of it wrote and a loop begins on a predictor, so it is not cleared between loops."""
        if self._hist is None or self._hist.shape != sample.shape or self._hist.device != sample.device:
            self._hist = torch.zeros(sample.shape, dtype=torch.float32, device=sample.device)
        return self._hist

    def graph_buffers(self, sample):
        return (self.history(sample).data_ptr(),)

    # -- the step --------------------------------------------------------------------------------------------------------
    def _run(self, model_output, sample, cfg, guidance_scale):
        """The one caller of these classes' fused step (ops.second_order_step_): ``sample`` is updated in place."""
        ops.second_order_step_(model_output, sample, self.history(sample), self._table, self._step_dev, self._step_dev, cfg=cfg,
                               guidance=float(guidance_scale), pred_type=self._pred)
        self._advance()
        return sample

    def step(self, model_output, timestep, sample, return_dict: bool = True):
        self._before_step(timestep)
        return self._result(self._run(model_output.contiguous(), sample.contiguous().clone(), False, 0.0), return_dict)

    def step_cfg(self, model_output_2b, sample, guidance_scale: float, out=None, cfg: bool = True):
        """Engine extension: CFG combine (``cfg=False``: a plain model output) + the entry, written over ``sample`` (graph replay)."""
        if out is not None and out.data_ptr() != sample.data_ptr():
            raise ValueError(f"{type(self).__name__}.step_cfg updates `sample` in place")
        self._before_step(self.timesteps[0])
        return self._run(model_output_2b, sample, cfg, guidance_scale)

    def step_inplace(self, model_output, sample):
        self._before_step(self.timesteps[0])
        return self._run(model_output, sample, False, 0.0)


class HeunDiscreteScheduler(_SecondOrderBase):
    """schedulers/scheduling_heun_discrete.py ("Heun"): Karras et al. 2022, Alg. 1 without churn.  Step i < n - 1, dt = sigma_{i+1} -
    sigma_i: the predictor entry evaluates the model at sigma_i and moves x by dt d, the corrector entry evaluates it at sigma_{i+1}
    and leaves x_i + dt (d + d') / 2 = (x_i + (dt/2) d) + (dt/2) d' -- the bracket is the one history tensor.  ``timesteps`` =
    [t0, t1, t1, t2, t2, ...]."""

    _defaults = dict(_SecondOrderBase._common_defaults, clip_sample=False, clip_sample_range=1.0)

    def _entries(self, sig, ts):
        n = len(ts)
        ent = []
        for i in range(n - 1):
            dt = sig[i + 1] - sig[i]
            ent.append((sig[i], dt / 2, dt, 1, ts[i]))
            ent.append((sig[i + 1], 0.0, dt / 2, 2, ts[i + 1]))
        ent.append((sig[n - 1], 0.0, sig[n] - sig[n - 1], 0, ts[n - 1]))
        return ent


class KDPM2DiscreteScheduler(_SecondOrderBase):
    """schedulers/scheduling_k_dpm_2_discrete.py ("DPM2"): k-diffusion's sample_dpm_2, the midpoint method in log sigma.  Step i <
    n - 1, sigma_mid = exp((ln sigma_i + ln sigma_{i+1}) / 2): the predictor entry evaluates the model at sigma_i and moves x to
    sigma_mid, the corrector entry evaluates it there -- at the fractional timestep whose training sigma is sigma_mid -- and leaves
    x_i + (sigma_{i+1} - sigma_i) d_mid; the history tensor is x_i.  ``timesteps`` = [t0, t_mid01, t1, t_mid12, ..., t_{n-1}]."""

    _defaults = dict(_SecondOrderBase._common_defaults)

    def _entries(self, sig, ts):
        n = len(ts)
        log_base = np.log(self._sig_all)
        ent = []
        for i in range(n - 1):
            mid = np.exp((np.log(sig[i]) + np.log(sig[i + 1])) / 2)
            ent.append((sig[i], 0.0, mid - sig[i], 1, ts[i]))
            ent.append((mid, 0.0, sig[i + 1] - sig[i], 2, float(_sigma_to_t(mid, log_base))))
        ent.append((sig[n - 1], 0.0, sig[n] - sig[n - 1], 0, ts[n - 1]))
        return ent
