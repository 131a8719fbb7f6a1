"""The case table of tests/test_scheduler_paths_cpu.py and tools/record_scheduler_paths.py: what the seven schedulers of
diffusers_amd/schedulers.py compute on the host and what they hand to their fused-step kernels.

Everything runs with ``device="cpu"`` over stand-ins of the eight sampler functions of ``ops`` (and of ``ops.add_noise``) that do NO
arithmetic: they log the call and return ``out`` or the sample; ``advance_step`` adds one to the counter.  A logged call holds the op
name, every scalar argument, and per tensor argument which known buffer it IS (the sample, the model output, the table, the step
counter, the begin counter, the noise table, a history buffer, or "fresh"), its shape, dtype and contiguity, the bits of a fresh
tensor (a generator draw or a copy), and the values of the device step counter and of DPM's begin counter at the call.  The one
exception to the CPU is ``set_timesteps/devices``: ``device="meta"`` (no data, no GPU) shows which tensors follow the device that
was asked for -- on the CPU a ``sigmas.to(device)`` and no move at all look the same.

Results are compared with tests/golden/scheduler_paths.npz (valid cases) and scheduler_paths.json (refusals), which
tools/record_scheduler_paths.py wrote from this table BEFORE the schedulers' shared code was folded: bit for bit wherever the
host's fp32 libm is the recording host's (``libm_probe``), and otherwise as the test's docstring says.

  CASES     ``{name: thunk}``; ``record(name)`` returns ``(arrays, meta)``: tensors as numpy arrays (bf16 as its int16 bits) and
            everything else as JSON
  ERRORS    ``{name: thunk}`` of calls that are refused; ``record_error(name)`` returns the exception's type name and message
"""
import hashlib
import json
import warnings

import numpy as np
import torch

from diffusers_amd import _lib as L
from diffusers_amd import ops
from diffusers_amd import schedulers as S

bf16 = torch.bfloat16
B1, B2 = (1, 4, 2, 3), (2, 4, 2, 3)      # latents: tiny (the golden file holds every fresh tensor), batch 1 and 2

_UNIPC = dict(prediction_type="flow_prediction", use_flow_sigmas=True, flow_shift=3.0)
_BETAS10 = (0.01, 0.02, 0.03, 0.05, 0.08, 0.1, 0.12, 0.15, 0.2, 0.25)
_TRAINED = dict(trained_betas=_BETAS10, num_train_timesteps=10)
# kind -> (class, the config every case of the kind starts from, the fused-step entry points it has)
KINDS = {
    "euler": (S.EulerDiscreteScheduler, {}, ("step", "step_cfg")),
    "euler_a": (S.EulerAncestralDiscreteScheduler, {}, ("step", "step_cfg")),
    "ddim": (S.DDIMScheduler, {}, ("step", "step_cfg")),
    "ddpm": (S.DDPMScheduler, {}, ("step", "step_inplace")),
    "flow": (S.FlowMatchEulerDiscreteScheduler, {}, ("step", "step_cfg", "step_inplace")),
    "unipc": (S.UniPCMultistepScheduler, _UNIPC, ("step", "step_cfg", "step_inplace")),
    "dpm": (S.DPMSolverMultistepScheduler, {}, ("step", "step_cfg", "step_inplace")),
}
_TAKES_CFG_FLAG = ("euler", "euler_a", "ddim", "dpm")       # step_cfg(cfg=False)


def make(kind, **cfg):
    cls, base, _ = KINDS[kind]
    return cls(**dict(base, **cfg))


def _rand(shape, seed, dtype=bf16):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)).to(dtype)


def _gen(seed=7):
    return torch.Generator("cpu").manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------------
# one recording
# ----------------------------------------------------------------------------------------------------------------------
class Run:
    """The scheduler of one case, the tensors the case hands to it, and what has been recorded so far."""

    def __init__(self, sch):
        global _RUN
        self.sch, self.named, self.arrays, self.meta, self.held = sch, {}, {}, {"log": []}, []
        _RUN = self         # the stand-ins log into the newest Run

    def put(self, key, t):
        """Tensor ``t`` under ``key``: its bits go to the arrays, [dtype, shape, device] to the meta.  Of a long tensor (the
        training ladders of 1000 entries: exact fp32 products, the same on every CPU) the meta holds the SHA-256 of the bits
        instead, and its two ends; of the 1001 training sigmas, every eighth and the last are kept."""
        if t is None:
            self.meta[key] = None
            return
        t = torch.as_tensor(t).detach()
        self.meta[key] = [str(t.dtype), list(t.shape), str(t.device)]
        t = t.cpu().contiguous()
        a = (t.view(torch.int16) if t.dtype == bf16 else t).numpy().copy()
        if a.size > 256 and "sigmas" in key:        # (sigmas come out of a libm ``pow``: numbers, not a digest -- see the test)
            self.arrays[key] = np.concatenate([a[::8], a[-1:]])
        elif a.size > 256:
            self.meta[key] += [hashlib.sha256(a.tobytes()).hexdigest(), a.reshape(-1)[[0, -1]].tolist()]
        else:
            self.arrays[key] = a

    def which(self, t):
        sch = self.sch
        known = dict(self.named)
        known.update(table=sch._table, step=sch._step_dev, begin=getattr(sch, "_begin_dev", None), coef=getattr(sch, "_coef", None),
                     noise_coef=getattr(sch, "_noise_coef", None))
        hist = getattr(sch, "_hist", None)
        for i, h in enumerate(hist if isinstance(hist, tuple) else (hist,)):
            known[f"hist{i}"] = h
        for name, c in known.items():
            if c is not None and (c is t or (c.data_ptr() == t.data_ptr() and c.shape == t.shape and c.dtype == t.dtype)):
                return name
        return "fresh"

    def counters(self):
        sch = self.sch
        begin = getattr(sch, "_begin_dev", None)
        return [None if sch._step_dev is None else int(sch._step_dev), None if begin is None else int(begin)]

    def log_call(self, op, tensors, scalars):
        entry = {"op": op, "scalars": {k: [type(v).__name__, v] for k, v in scalars.items()}, "counters": self.counters(),
                 "tensors": {}}
        n = len(self.meta["log"])
        for k, t in tensors.items():
            if t is None:
                entry["tensors"][k] = None
                continue
            name = self.which(t)
            entry["tensors"][k] = [name, list(t.shape), str(t.dtype), t.is_contiguous()]
            if name == "fresh":
                self.put(f"op{n}.{k}", t)
        self.meta["log"].append(entry)

    def note(self, what, value=None):
        self.meta["log"].append({"note": what, "value": value, "index": [self.sch.step_index, self.sch.begin_index],
                                 "counters": self.counters()})


_RUN = None


def install(monkeypatch, ops_module=ops):
    """The stand-ins: the eight sampler functions of ``ops`` and ``add_noise``, with the real functions' defaults."""
    def euler_scale_model_input(x, table, step_idx, rep=1):
        _RUN.log_call("euler_scale_model_input", dict(x=x, table=table, step_idx=step_idx), dict(rep=rep))
        return x

    def euler_step(eps, x, table, step_idx, *, cfg, guidance, out=None, pred_type=L.PRED_EPSILON):
        _RUN.log_call("euler_step", dict(eps=eps, x=x, table=table, step_idx=step_idx, out=out),
                      dict(cfg=cfg, guidance=guidance, pred_type=pred_type))
        return x if out is None else out

    def euler_ancestral_step(eps, x, noise, table, step_idx, *, cfg, guidance, out=None, pred_type=L.PRED_EPSILON,
                             noise_step_stride=0):
        _RUN.log_call("euler_ancestral_step", dict(eps=eps, x=x, noise=noise, table=table, step_idx=step_idx, out=out),
                      dict(cfg=cfg, guidance=guidance, pred_type=pred_type, noise_step_stride=noise_step_stride))
        return x if out is None else out

    def x0_linear_step(eps, x, noise, table, step_idx, *, cfg, guidance, out=None, noise_step_stride=0, pred_type=L.PRED_EPSILON):
        _RUN.log_call("x0_linear_step", dict(eps=eps, x=x, noise=noise, table=table, step_idx=step_idx, out=out),
                      dict(cfg=cfg, guidance=guidance, pred_type=pred_type, noise_step_stride=noise_step_stride))
        return x if out is None else out

    def flowmatch_step(v, x, table, step_idx, *, cfg=False, guidance=0.0, out=None):
        _RUN.log_call("flowmatch_step", dict(v=v, x=x, table=table, step_idx=step_idx, out=out), dict(cfg=cfg, guidance=guidance))
        return x if out is None else out

    def unipc_flow_step_(v, x, last, m1, m2, coef, step_idx, *, cfg=False, guidance=0.0):
        _RUN.log_call("unipc_flow_step_", dict(v=v, x=x, last=last, m1=m1, m2=m2, coef=coef, step_idx=step_idx),
                      dict(cfg=cfg, guidance=guidance))
        return x

    def dpmpp_2m_step_(eps, x, m1, table, step_idx, begin_idx, *, cfg=False, guidance=0.0, pred_type=L.PRED_EPSILON):
        _RUN.log_call("dpmpp_2m_step_", dict(eps=eps, x=x, m1=m1, table=table, step_idx=step_idx, begin_idx=begin_idx),
                      dict(cfg=cfg, guidance=guidance, pred_type=pred_type))
        return x

    def advance_step(step_idx):
        _RUN.log_call("advance_step", dict(step_idx=step_idx), {})
        step_idx.add_(1)

    def add_noise(x, noise, a, b):
        _RUN.log_call("add_noise", dict(x=x, noise=noise), dict(a=a, b=b))
        return x

    for f in (euler_scale_model_input, euler_step, euler_ancestral_step, x0_linear_step, flowmatch_step, unipc_flow_step_,
              dpmpp_2m_step_, advance_step, add_noise):
        monkeypatch.setattr(ops_module, f.__name__, f)


# ----------------------------------------------------------------------------------------------------------------------
# construction and set_timesteps
# ----------------------------------------------------------------------------------------------------------------------
def _plain(v):
    if torch.is_tensor(v):
        return {"tensor": v.detach().double().reshape(-1).tolist(), "dtype": str(v.dtype), "shape": list(v.shape)}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, float) and not np.isfinite(v):
        return repr(v)
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return repr(v)


def _schedule_state(run, tag):
    """The host side of a schedule: timesteps, sigmas (and where they live), indices."""
    sch = run.sch
    run.put(f"{tag}.timesteps", sch.timesteps)
    host = np.asarray(sch._timesteps_host)     # (the lookup table of index_for_timestep: its dtype, and that it mirrors `timesteps`)
    run.meta[f"{tag}.timesteps_host"] = [str(host.dtype), bool(np.array_equal(host, sch.timesteps.cpu().numpy()))]
    run.put(f"{tag}.sigmas", getattr(sch, "sigmas", None))
    run.meta[f"{tag}.state"] = dict(num_inference_steps=sch.num_inference_steps, step_index=sch.step_index,
                                    begin_index=sch.begin_index, init_noise_sigma=_plain(sch.init_noise_sigma),
                                    init_noise_sigma_type=type(sch.init_noise_sigma).__name__)


def _construct(kind, **cfg):
    def thunk():
        run = Run(make(kind, **cfg))
        sch, cls = run.sch, KINDS[kind][0]
        _schedule_state(run, "new")
        for name in ("betas", "alphas", "alphas_cumprod", "final_alpha_cumprod", "one"):
            run.put(name, getattr(sch, name, None))
        token, other = sch.graph_token(), make(kind, **cfg).graph_token()
        again = cls.from_config(sch.config)
        foreign = cls.from_config(dict(sch.config, _class_name="Other", no_such_option=3, trained_betas=list(_BETAS10)),
                                  num_train_timesteps=10)
        run.put("from_config.timesteps", again.timesteps)
        run.meta.update(
            config={k: _plain(v) for k, v in dict(sch.config).items()}, order=sch.order, no_table_yet=sch._table is None,
            token=[token[0], token[2]], tokens_differ=token != other and token[1] != other[1],
            from_config_same=dict(again.config) == dict(sch.config) and type(again) is cls,
            from_config_foreign={k: _plain(v) for k, v in dict(foreign.config).items()},
            needs_step_noise=getattr(sch, "needs_step_noise", False),       # (as the pipelines read it)
            attributes={k: _plain(getattr(sch, k, "absent")) for k in (
                "step_noise_dtype", "is_scale_input_called", "custom_timesteps", "variance_type", "sigma_min",
                "sigma_max", "shift", "second_order_rows", "_pred", "_eta")})
        return run
    return thunk


def _device_state(run, tag, prev):
    """The device side after a ``set_timesteps``: the table (for DDIM this builds it for eta 0), the counters, UniPC's and DPM's
    extras, the add_noise table -- and whether each buffer kept the address it had after the previous call."""
    sch = run.sch
    now = {"table": sch.device_table, "step": sch.device_step, "coef": getattr(sch, "_coef", None),
           "begin": getattr(sch, "device_begin", None)}
    try:
        now["noise_coef"] = sch.add_noise_table(bf16)
    except NotImplementedError as exc:
        now["noise_coef"] = None
        run.meta[f"{tag}.add_noise_table"] = str(exc)
    for k, t in now.items():
        run.put(f"{tag}.{k}", t)
    run.meta[f"{tag}.second_order_rows"] = getattr(sch, "second_order_rows", None)
    run.meta[f"{tag}.kept"] = {k: None if prev.get(k) is None or t is None else prev[k].data_ptr() == t.data_ptr()
                               for k, t in now.items()}
    run.meta[f"{tag}.after_tables"] = [sch.step_index, sch.begin_index, run.counters()]
    run.held.append(now)        # (kept alive: a reallocated buffer never lands on the old address)
    return now


def _set_timesteps(kind, calls, prepare=None, **cfg):
    """``calls``: the keyword sets of consecutive ``set_timesteps`` calls.  Between two calls the scheduler is given a begin index
    and rewound to step 1, which the next ``set_timesteps`` has to clear."""
    def thunk():
        run = Run(make(kind, **cfg))
        sch, prev = run.sch, {}
        if prepare is not None:
            prepare(sch)
        for i, kw in enumerate(calls):
            sch.set_timesteps(device="cpu", **kw)
            _schedule_state(run, f"call{i}")
            prev = _device_state(run, f"call{i}", prev)
            sch.set_begin_index(1)
            sch.reset(1)
        return run
    return thunk


def _devices(kind):
    """Where each tensor of a schedule lives when a device other than the CPU is asked for.  "meta" holds no data and needs no GPU:
    only the devices are recorded.  (Not UniPC, which reads its timesteps back from the device.)"""
    def thunk():
        run = Run(make(kind))
        sch = run.sch
        sch.set_timesteps(4, device="meta")
        tensors = dict(timesteps=sch.timesteps, sigmas=getattr(sch, "sigmas", None), table=sch.device_table, step=sch.device_step,
                       begin=getattr(sch, "device_begin", None))
        run.meta["devices"] = {k: None if t is None else str(t.device) for k, t in tensors.items()}
        return run
    return thunk


def _refused_state(kind, bad, first=4, **cfg):
    """What a refused ``set_timesteps(**bad)`` leaves behind -- after a good ``set_timesteps(first)`` and a begin index, or on the
    new object (``first=None``: the configuration itself is what is refused)."""
    def thunk():
        run = Run(make(kind, **cfg))
        sch = run.sch
        if first is not None:
            sch.set_timesteps(first, device="cpu")
            sch.set_begin_index(1)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sch.set_timesteps(device="cpu", **bad)
            run.meta["refused"] = None
        except Exception as exc:        # noqa: BLE001
            run.meta["refused"] = [type(exc).__name__, str(exc)]
        _schedule_state(run, "after")
        run.put("after.table", sch._table)
        run.meta["after.counters"] = run.counters()
        return run
    return thunk


def _counts(*ns):
    return [dict(num_inference_steps=n) for n in ns]


# ----------------------------------------------------------------------------------------------------------------------
# add_noise / scale_noise
# ----------------------------------------------------------------------------------------------------------------------
def _noising(kind):
    def thunk():
        run = Run(make(kind))
        sch = run.sch
        sch.set_timesteps(5, device="cpu")
        x1, n1, x2, n2 = _rand(B1, 1), _rand(B1, 2), _rand(B2, 3), _rand(B2, 4)
        run.named.update(x1=x1, n1=n1, x2=x2, n2=n2)

        def both(state):
            run.note(state)
            for x, n, ts in ((x1, n1, sch.timesteps[1:2]), (x2, n2, sch.timesteps[[1, 3]]), (x2, n2, sch.timesteps[3])):
                try:
                    out = sch.scale_noise(x, ts, n) if kind == "flow" else sch.add_noise(x, n, ts)
                    run.note("returned", [run.which(out), list(out.shape)])
                except NotImplementedError as exc:
                    run.note("NotImplementedError", str(exc))

        both("no begin index")
        sch.set_begin_index(2)
        both("begin index 2, before the first step")
        _drive(run, "step_cfg" if "step_cfg" in KINDS[kind][2] else "step_inplace", 2, B1)
        both("mid-loop")
        return run
    return thunk


# ----------------------------------------------------------------------------------------------------------------------
# step scripts
# ----------------------------------------------------------------------------------------------------------------------
def _tensors(run, kind, shape, n):
    sample = _rand(shape, 11, torch.float32 if kind == "unipc" else bf16)
    run.named.update(sample=sample, model_output=_rand(shape, 12), model_output_2b=_rand((2 * shape[0],) + shape[1:], 13),
                     noise_table=_rand((n,) + shape, 14))


def _after(run, entry, out):
    if isinstance(out, tuple):
        ret = ["tuple", len(out), [None if o is None else run.which(o) for o in out]]
    elif isinstance(out, S.SchedulerOutput):
        ret = ["SchedulerOutput", None, [run.which(out.prev_sample), out.pred_original_sample is None]]
    else:
        ret = [type(out).__name__, None, run.which(out)]
    run.note(f"{entry} returned", ret)


def _call(run, kind, entry, i, **extra):
    sch, t = run.sch, run.named
    if entry == "step":
        if kind in ("euler_a", "ddpm") and "noise" not in extra:
            extra.setdefault("generator", run.generator)
        out = sch.step(t["model_output"], sch.timesteps[i], t["sample"], **extra)
    elif entry == "step_cfg":
        if kind == "euler_a" or extra.get("eta", 0.0) > 0:
            extra.setdefault("noise_table", t["noise_table"])
        mo = t["model_output"] if extra.get("cfg") is False else t["model_output_2b"]
        out = sch.step_cfg(mo, t["sample"], 5.0, out=t["sample"], **extra)
    else:
        out = sch.step_inplace(t["model_output"], t["sample"], *((t["noise_table"],) if kind == "ddpm" else ()))
    _after(run, entry, out)


def _drive(run, entry, steps, shape=None, first=None, **extra):
    """``steps`` calls of ``entry`` from schedule entry ``first`` (default: where the scheduler stands)."""
    sch = run.sch
    kind = next(k for k, v in KINDS.items() if type(sch) is v[0])
    if shape is not None:
        _tensors(run, kind, shape, len(sch.timesteps))
        run.generator = _gen()
    if first is None:
        first = sch.step_index if sch.step_index is not None else (sch.begin_index or 0)
    for i in range(first, first + steps):
        _call(run, kind, entry, i, **extra)


def _loops(kind, entry, **cfg):
    """A full loop, a loop after ``set_begin_index(2)``, and ``reset(1)`` then two steps, on one scheduler object."""
    def thunk():
        run = Run(make(kind, **cfg))
        sch = run.sch
        sch.set_timesteps(4, device="cpu")
        run.note("full loop")
        _drive(run, entry, 4, B1)
        sch.set_timesteps(5, device="cpu")
        sch.set_begin_index(2)
        run.note("begin index 2")
        _drive(run, entry, 3, B2)
        run.note("reset(1)")
        sch.reset(1)
        _drive(run, entry, 2)
        run.put("table", sch._table)
        run.meta["is_scale_input_called"] = getattr(sch, "is_scale_input_called", None)
        return run
    return thunk


def _script(kind, body, n=4, shape=B1, **cfg):
    """``body(run)`` on a new scheduler after ``set_timesteps(n)``, with the step tensors of ``shape`` made."""
    def thunk():
        run = Run(make(kind, **cfg))
        run.sch.set_timesteps(n, device="cpu")
        _tensors(run, kind, shape, n)
        run.generator = _gen()
        body(run)
        run.put("table", run.sch._table)
        return run
    return thunk


def _tuple_out(run):
    _drive(run, "step", 2, return_dict=False)


def _cfg_off(run):
    _drive(run, "step_cfg", 2, cfg=False)


def _out_of_order(run):
    for i in (2, 0, 3, 3):
        _drive(run, "step", 1, first=i)


def _euler_scale(run):
    sch, t = run.sch, run.named
    run.note("is_scale_input_called", sch.is_scale_input_called)
    for rep in (2, 1):
        out = sch.scale_model_input(t["sample"], sch.timesteps[0], rep=rep)
        run.note("scale_model_input returned", [run.which(out), sch.is_scale_input_called])
        _drive(run, "step_cfg", 1)


def _identity_scale(run):
    out = run.sch.scale_model_input(run.named["sample"], run.sch.timesteps[0])
    run.note("scale_model_input returned", run.which(out))


def _ddim_eta_generator(run):
    _drive(run, "step", 2, eta=0.5, generator=run.generator)
    torch.manual_seed(5)
    _drive(run, "step", 1, eta=0.5)             # no generator: a draw from the global one


def _ddim_variance_noise(run):
    run.named["variance_noise"] = _rand(B1, 15)
    _drive(run, "step", 2, eta=0.5, variance_noise=run.named["variance_noise"])


def _ddim_eta_changes(run):
    sch = run.sch
    _drive(run, "step_cfg", 2)
    run.put("table.eta0", sch._table)
    _drive(run, "step_cfg", 2, eta=0.5)         # mid-loop: the rebuild keeps step 2
    run.put("table.eta0.5", sch._table)
    sch.set_timesteps(4, device="cpu")
    sch.set_begin_index(1)
    _drive(run, "step_cfg", 3, eta=1.0)         # a new loop from entry 1 with another eta: the rebuild keeps the begin index
    run.put("table.eta1", sch._table)


def _ddim_lazy_table(run):
    sch = run.sch
    sch.set_begin_index(2)
    run.note("before the table is read", sch._table is None)
    run.put("lazy.table", sch.device_table)
    run.note("after device_table")
    sch.set_timesteps(4, device="cpu")
    sch.set_begin_index(2)
    run.put("lazy.step", sch.device_step)
    run.note("after device_step")
    _drive(run, "step_cfg", 2)


def _ddpm_noise_argument(run):
    run.named["variance_noise"] = _rand(B1, 15)
    _drive(run, "step", 4, noise=run.named["variance_noise"])


def _model_timesteps(run):
    sch = run.sch
    sch.device_table        # (DDIM builds its table here)
    sch.set_model_timesteps([float(i) + 0.5 for i in range(len(sch.timesteps))])
    run.put("table.model_timesteps", sch._table)
    sch.set_model_timesteps(torch.arange(len(sch.timesteps)))


def _graph_buffers(run):
    sch = run.sch
    sch.device_table
    ptrs = sch.graph_buffers(run.named["sample"])
    known = {"coef": getattr(sch, "_coef", None), "begin": getattr(sch, "_begin_dev", None)}
    hist = getattr(sch, "_hist", None)
    known.update({f"hist{i}": h for i, h in enumerate(hist if isinstance(hist, tuple) else (hist,))})
    names = {t.data_ptr(): k for k, t in known.items() if t is not None}
    run.note("graph_buffers", [type(ptrs).__name__, [names.get(p, "unknown") for p in ptrs]])
    run.note("again", tuple(ptrs) == tuple(sch.graph_buffers(run.named["sample"])))
    other = _rand(B2, 16, run.named["sample"].dtype)
    run.note("another sample size", [a == b for a, b in zip(ptrs, sch.graph_buffers(other))])


def _index_for_timestep(run):
    sch = run.sch
    run.note("index_for_timestep", [sch.index_for_timestep(t) for t in sch.timesteps]
             + [sch.index_for_timestep(float(sch.timesteps[1])), sch.index_for_timestep(sch.timesteps[2], sch.timesteps)])


def _repeated_timesteps(run):
    """More steps than training timesteps: entries repeat, and a lookup takes the second match."""
    _index_for_timestep(run)
    _drive(run, "step", 2)


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
_SPACINGS = [dict(timestep_spacing="linspace"), dict(timestep_spacing="leading"), dict(timestep_spacing="leading", steps_offset=1),
             dict(timestep_spacing="trailing"), dict(timestep_spacing="trailing", steps_offset=1)]
_VP = [dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012), _TRAINED]
_CONFIGS = {
    "euler": _SPACINGS + _VP + [
        dict(prediction_type="v_prediction"), dict(prediction_type="sample"), dict(prediction_type="original_sample"),
        dict(use_karras_sigmas=True), dict(use_exponential_sigmas=True), dict(use_karras_sigmas=True, sigma_min=0.1, sigma_max=10.0),
        dict(final_sigmas_type="sigma_min"), dict(use_karras_sigmas=True, final_sigmas_type="sigma_min", timestep_spacing="leading")],
    "euler_a": _SPACINGS + _VP + [dict(prediction_type="v_prediction")],
    "ddim": _SPACINGS + _VP + [
        dict(prediction_type="v_prediction"), dict(prediction_type="sample"), dict(set_alpha_to_one=False),
        dict(clip_sample=False), dict(clip_sample_range=2.5), dict(set_alpha_to_one=False, timestep_spacing="trailing")],
    "ddpm": _SPACINGS + _VP + [
        dict(prediction_type="v_prediction"), dict(prediction_type="sample"), dict(variance_type="fixed_large"),
        dict(clip_sample=False), dict(clip_sample_range=2.5), dict(variance_type="fixed_large", timestep_spacing="linspace")],
    "flow": [dict(shift=3.0), dict(use_dynamic_shifting=True), dict(use_dynamic_shifting=True, time_shift_type="linear"),
             dict(num_train_timesteps=500, shift=2.0)],
    "unipc": [dict(flow_shift=1.0), dict(flow_shift=5.0), dict(solver_order=1), dict(solver_type="bh1"),
              dict(solver_type="bh1", solver_order=1, num_train_timesteps=500)],
    "dpm": _SPACINGS + _VP + [
        dict(prediction_type="v_prediction"), dict(prediction_type="sample"), dict(use_karras_sigmas=True),
        dict(use_exponential_sigmas=True), dict(solver_order=1), dict(solver_type="heun"), dict(euler_at_final=True),
        dict(lower_order_final=False), dict(final_sigmas_type="sigma_min"),
        dict(final_sigmas_type="sigma_min", use_karras_sigmas=True, solver_type="heun"),
        dict(final_sigmas_type="sigma_min", timestep_spacing="trailing"),
        dict(final_sigmas_type="sigma_min", timestep_spacing="trailing", lower_order_final=False),
        dict(final_sigmas_type="sigma_min", timestep_spacing="trailing", euler_at_final=True)],
}


def _name(cfg):
    return ",".join(f"{k}={'trained' if k == 'trained_betas' else v}" for k, v in cfg.items()) or "defaults"


def _cases():
    c = {}
    for kind, (_, _, entries) in KINDS.items():
        mu = dict(mu=0.8)
        for cfg in [{}] + _CONFIGS[kind]:
            c[f"{kind}/new/{_name(cfg)}"] = _construct(kind, **cfg)
            n_train = cfg.get("num_train_timesteps", 1000)
            calls = _counts(4, 7) if n_train >= 16 else _counts(4, 3)
            if cfg.get("final_sigmas_type") == "sigma_min" and kind == "dpm":
                calls = _counts(4, 14, 15)                    # lower_order_final: second order on the last row from 15 steps on
            if cfg.get("use_dynamic_shifting"):
                calls = [dict(k, **mu) for k in calls]
            c[f"{kind}/set_timesteps/{_name(cfg)}"] = _set_timesteps(kind, calls, **cfg)
        # same count twice (buffers refreshed in place), other counts (reallocated), one step, DPM's 15-step boundary
        c[f"{kind}/set_timesteps/counts"] = _set_timesteps(kind, _counts(4, 4, 6, 1, 15, 16, 16))
        c[f"{kind}/add_noise"] = _noising(kind)
        if kind != "unipc":
            c[f"{kind}/set_timesteps/devices"] = _devices(kind)
        for entry in entries:
            c[f"{kind}/loops/{entry}"] = _loops(kind, entry)
        c[f"{kind}/step/return_dict=False"] = _script(kind, _tuple_out)
        c[f"{kind}/step/batch_of_2"] = _script(kind, lambda run: _drive(run, "step", 2), shape=B2)
        c[f"{kind}/set_model_timesteps"] = _script(kind, _model_timesteps)
        c[f"{kind}/graph_buffers"] = _script(kind, _graph_buffers)
        c[f"{kind}/index_for_timestep"] = _script(kind, _index_for_timestep, n=6)
        if kind in _TAKES_CFG_FLAG:
            c[f"{kind}/step_cfg/cfg=False"] = _script(kind, _cfg_off)
        if kind not in ("euler", "euler_a"):
            c[f"{kind}/scale_model_input"] = _script(kind, _identity_scale)
    for kind in ("euler", "euler_a", "ddim", "ddpm", "dpm"):
        c[f"{kind}/loops/step/v_prediction"] = _loops(kind, "step", prediction_type="v_prediction")
        c[f"{kind}/loops/{KINDS[kind][2][1]}/sample"] = _loops(kind, KINDS[kind][2][1], **(
            dict(prediction_type="sample") if kind != "euler_a" else dict(prediction_type="v_prediction")))
    for kind in ("euler", "euler_a"):
        c[f"{kind}/scale_model_input"] = _script(kind, _euler_scale)
    c["euler/set_timesteps/custom_timesteps"] = _set_timesteps("euler", [dict(timesteps=[900, 600, 300, 100]),
                                                                         dict(timesteps=np.array([801.0, 401.5, 1.0]))])
    c["euler/set_timesteps/custom_sigmas"] = _set_timesteps("euler", [dict(sigmas=[10.0, 4.0, 1.5, 0.5, 0.0]),
                                                                      dict(sigmas=[14.6, 3.0, 0.03]), dict(num_inference_steps=4)])
    c["euler/set_timesteps/custom_timesteps_sigma_min"] = _set_timesteps("euler", [dict(timesteps=[900, 600, 300, 100])],
                                                                         final_sigmas_type="sigma_min")
    c["flow/set_timesteps/sigmas"] = _set_timesteps("flow", [dict(sigmas=[1.0, 0.75, 0.5, 0.25]),
                                                             dict(sigmas=[1.0, 0.6, 0.3, 0.1], num_inference_steps=4),
                                                             dict(sigmas=np.linspace(1.0, 0.2, 5), mu=0.3)], shift=3.0)
    c["flow/set_timesteps/sigmas_mu"] = _set_timesteps("flow", [dict(sigmas=[1.0, 0.75, 0.5, 0.25], mu=1.1),
                                                                dict(num_inference_steps=4, mu=0.5)], use_dynamic_shifting=True)
    c["flow/set_timesteps/set_shift"] = _set_timesteps("flow", _counts(4, 4), prepare=lambda sch: sch.set_shift(2.0))
    c["unipc/set_timesteps/mu"] = _set_timesteps("unipc", [dict(num_inference_steps=5, mu=0.7)])
    c["dpm/set_timesteps/mu"] = _set_timesteps("dpm", [dict(num_inference_steps=5, mu=0.7)])
    c["dpm/index_for_timestep/repeated"] = _script("dpm", _repeated_timesteps, n=16, solver_order=1, **_TRAINED)
    zero_beta = dict(trained_betas=(0.0,) + _BETAS10[1:], num_train_timesteps=10)
    even, n3 = dict(timestep_spacing="even"), dict(num_inference_steps=3)
    for name, kind, bad, first, cfg in (
            ("final_sigmas_type", "euler", n3, None, dict(final_sigmas_type="one")), ("spacing", "euler", n3, None, even),
            ("nothing", "euler", {}, 4, {}), ("count_and_timesteps", "euler", dict(n3, timesteps=[9, 6, 3]), 4, {}),
            ("spacing", "euler_a", n3, None, even), ("non_finite_rows", "euler_a", n3, None, zero_beta),
            ("too_many_steps", "ddim", dict(num_inference_steps=1001), 4, {}), ("spacing", "ddim", n3, None, even),
            ("too_many_steps", "ddpm", dict(num_inference_steps=1001), 4, {}), ("spacing", "ddpm", n3, None, even),
            ("custom_timesteps", "ddpm", dict(timesteps=[9, 6]), 4, {}),
            ("without_mu", "flow", n3, None, dict(use_dynamic_shifting=True)),
            ("custom_timesteps", "flow", dict(timesteps=[900.0, 600.0]), 4, {}),
            ("sigmas_count", "flow", dict(n3, sigmas=[1.0, 0.5]), 4, {}), ("custom_sigmas", "unipc", dict(sigmas=[1.0, 0.5]), 4, {}),
            ("custom_timesteps", "dpm", dict(timesteps=[9, 6]), 4, {}), ("nothing", "dpm", {}, 4, {}),
            ("spacing", "dpm", n3, None, even), ("non_finite_rows", "dpm", dict(num_inference_steps=16), 4, _TRAINED)):
        c[f"{kind}/refused_set_timesteps/{name}"] = _refused_state(kind, bad, first, **cfg)
    c["euler_a/step/generator_batch_of_2"] = _script("euler_a", lambda run: _drive(run, "step", 3), shape=B2)
    c["ddim/step/eta_generator"] = _script("ddim", _ddim_eta_generator)
    c["ddim/step/variance_noise"] = _script("ddim", _ddim_variance_noise)
    c["ddim/step_cfg/eta_changes"] = _script("ddim", _ddim_eta_changes)
    c["ddim/device_table/lazy"] = _script("ddim", _ddim_lazy_table)
    c["ddim/step/out_of_order"] = _script("ddim", _out_of_order)
    c["ddpm/step/out_of_order"] = _script("ddpm", _out_of_order)
    c["ddpm/step/noise_argument"] = _script("ddpm", _ddpm_noise_argument)
    return c


def _errors():
    zero_beta = dict(trained_betas=(0.0,) + _BETAS10[1:], num_train_timesteps=10)

    def ready(kind, n=4, **cfg):
        sch = make(kind, **cfg)
        sch.set_timesteps(n, device="cpu")
        return sch

    def step(kind, timestep=None, sch=None, entry="step", **extra):
        """One ``entry`` call on a 4-step scheduler (or ``sch``), through the case machinery."""
        def thunk():
            run = Run(sch() if sch is not None else ready(kind))
            _tensors(run, kind, B1, 4)
            run.generator = _gen()
            if timestep is not None:
                return run.sch.step(run.named["model_output"], timestep, run.named["sample"], **extra)
            return _call(run, kind, entry, 0, **extra)
        return thunk

    def past_the_end(kind):
        def thunk():
            run = Run(ready(kind))
            _drive(run, "step_cfg", 5, B1)
        return thunk

    def other_out(kind):
        def thunk():
            sch = ready(kind)
            x = _rand(B1, 1, torch.float32)
            sch.step_cfg(_rand(B2, 2), x, 5.0, out=x.clone())
        return thunk

    def add_noise(kind, x, n, ts):
        return lambda: ready(kind).add_noise(x, n, ts(ready(kind)) if callable(ts) else ts)

    e = {
        "base/unknown_config_key": lambda: make("euler", no_such_option=1),
        "base/beta_schedule": lambda: make("euler", beta_schedule="squaredcos_cap_v2"),
        "base/add_noise_not_implemented": add_noise("unipc", _rand(B1, 1), _rand(B1, 2), lambda s: s.timesteps[:1]),
        "base/add_noise_dtype": add_noise("euler", _rand(B1, 1, torch.float32), _rand(B1, 2, torch.float32), lambda s: s.timesteps[:1]),
        "base/add_noise_batch": add_noise("euler", _rand(B2, 1), _rand(B2, 2), lambda s: s.timesteps[:3]),
        "base/timestep_not_in_schedule": lambda: ready("euler").index_for_timestep(3.25),
        "base/set_model_timesteps_before_set_timesteps": lambda: make("euler").set_model_timesteps([1.0]),
        "base/set_model_timesteps_count": lambda: ready("flow").set_model_timesteps([1.0, 2.0]),
        "euler/beta_sigmas": lambda: make("euler", use_beta_sigmas=True),
        "euler/zero_snr": lambda: make("euler", rescale_betas_zero_snr=True),
        "euler/karras_and_exponential": lambda: make("euler", use_karras_sigmas=True, use_exponential_sigmas=True),
        "euler/timestep_type": lambda: make("euler", timestep_type="continuous"),
        "euler/interpolation_type": lambda: make("euler", interpolation_type="log_linear"),
        "euler/prediction_type": lambda: make("euler", prediction_type="flow"),
        "euler/spacing": lambda: ready("euler", timestep_spacing="even"),
        "euler/set_timesteps_nothing": lambda: make("euler").set_timesteps(),
        "euler/set_timesteps_count_and_timesteps": lambda: make("euler").set_timesteps(4, timesteps=[900, 600, 300, 100]),
        "euler/set_timesteps_count_and_sigmas": lambda: make("euler").set_timesteps(4, sigmas=[10.0, 4.0, 1.5, 0.5, 0.0]),
        "euler/set_timesteps_timesteps_and_sigmas": lambda: make("euler").set_timesteps(timesteps=[9, 6], sigmas=[2.0, 1.0, 0.0]),
        "euler/set_timesteps_timesteps_karras": lambda: make("euler", use_karras_sigmas=True).set_timesteps(timesteps=[9, 6]),
        "euler/set_timesteps_timesteps_exponential": lambda: make("euler", use_exponential_sigmas=True).set_timesteps(timesteps=[9, 6]),
        "euler/final_sigmas_type": lambda: ready("euler", final_sigmas_type="one"),
        "euler/step_int_timestep": step("euler", 3),
        "euler/step_int_tensor_timestep": step("euler", torch.tensor(3)),
        "euler/step_int32_tensor_timestep": step("euler", torch.tensor(3, dtype=torch.int32)),
        "euler/step_s_churn": step("euler", s_churn=0.5),
        "euler_a/zero_snr": lambda: make("euler_a", rescale_betas_zero_snr=True),
        "euler_a/prediction_type_sample": lambda: make("euler_a", prediction_type="sample"),
        "euler_a/prediction_type": lambda: make("euler_a", prediction_type="flow"),
        "euler_a/spacing": lambda: ready("euler_a", timestep_spacing="even"),
        "euler_a/non_finite_rows": lambda: ready("euler_a", **zero_beta),
        "euler_a/step_before_set_timesteps": step("euler_a", sch=lambda: make("euler_a")),
        "euler_a/step_cfg_before_set_timesteps": step("euler_a", sch=lambda: make("euler_a"), entry="step_cfg"),
        "euler_a/step_past_the_end": past_the_end("euler_a"),
        "euler_a/step_int_timestep": step("euler_a", 3),
        "euler_a/step_int_tensor_timestep": step("euler_a", torch.tensor(3)),
        "euler_a/step_cfg_without_noise_table": step("euler_a", entry="step_cfg", noise_table=None),
        "euler_a/step_cfg_noise_table_rows": step("euler_a", entry="step_cfg", noise_table=_rand((3,) + B1, 1)),
        "ddim/thresholding": lambda: make("ddim", thresholding=True),
        "ddim/zero_snr": lambda: make("ddim", rescale_betas_zero_snr=True),
        "ddim/prediction_type": lambda: make("ddim", prediction_type="flow"),
        "ddim/too_many_steps": lambda: ready("ddim", n=1001),
        "ddim/spacing": lambda: ready("ddim", timestep_spacing="even"),
        "ddim/step_before_set_timesteps": step("ddim", sch=lambda: make("ddim")),
        "ddim/step_use_clipped_model_output": step("ddim", use_clipped_model_output=True),
        "ddim/step_generator_and_variance_noise": step("ddim", eta=0.5, generator=_gen(), variance_noise=_rand(B1, 1)),
        "ddim/step_cfg_eta_without_noise_table": step("ddim", entry="step_cfg", eta=0.5, noise_table=None),
        "ddim/step_timestep_not_in_schedule": step("ddim", torch.tensor(5)),
        "ddpm/thresholding": lambda: make("ddpm", thresholding=True),
        "ddpm/zero_snr": lambda: make("ddpm", rescale_betas_zero_snr=True),
        "ddpm/prediction_type": lambda: make("ddpm", prediction_type="flow"),
        "ddpm/variance_type": lambda: make("ddpm", variance_type="learned"),
        "ddpm/custom_timesteps": lambda: make("ddpm").set_timesteps(timesteps=[9, 6]),
        "ddpm/too_many_steps": lambda: ready("ddpm", n=1001),
        "ddpm/spacing": lambda: ready("ddpm", timestep_spacing="even"),
        "ddpm/step_timestep_not_in_schedule": step("ddpm", torch.tensor(5)),
        "flow/karras": lambda: make("flow", use_karras_sigmas=True),
        "flow/shift_terminal": lambda: make("flow", shift_terminal=0.1),
        "flow/stochastic_sampling": lambda: make("flow", stochastic_sampling=True),
        "flow/time_shift_type": lambda: make("flow", time_shift_type="cubic"),
        "flow/dynamic_shifting_without_mu": lambda: ready("flow", use_dynamic_shifting=True),
        "flow/custom_timesteps": lambda: make("flow").set_timesteps(timesteps=[900.0, 600.0]),
        "flow/sigmas_count": lambda: make("flow").set_timesteps(3, sigmas=[1.0, 0.5]),
        "flow/scale_noise_without_noise": lambda: ready("flow").scale_noise(_rand(B1, 1), torch.tensor([500.0])),
        "flow/step_int_timestep": step("flow", 3),
        "flow/step_int_tensor_timestep": step("flow", torch.tensor(3)),
        "flow/step_per_token_timesteps": step("flow", per_token_timesteps=torch.zeros(1)),
        "unipc/default_config": lambda: S.UniPCMultistepScheduler(),
        "unipc/flow_prediction_without_flow_sigmas": lambda: S.UniPCMultistepScheduler(prediction_type="flow_prediction"),
        "unipc/solver_order": lambda: make("unipc", solver_order=3),
        "unipc/solver_type": lambda: make("unipc", solver_type="logrho"),
        "unipc/predict_x0": lambda: make("unipc", predict_x0=False),
        "unipc/lower_order_final": lambda: make("unipc", lower_order_final=False),
        "unipc/final_sigmas_type": lambda: make("unipc", final_sigmas_type="sigma_min"),
        "unipc/custom_sigmas": lambda: make("unipc").set_timesteps(sigmas=[1.0, 0.5]),
        "unipc/step_before_set_timesteps": step("unipc", sch=lambda: make("unipc")),
        "unipc/step_cfg_other_out": other_out("unipc"),
        "dpm/algorithm_type": lambda: make("dpm", algorithm_type="sde-dpmsolver++"),
        "dpm/solver_order": lambda: make("dpm", solver_order=3),
        "dpm/solver_type": lambda: make("dpm", solver_type="bh2"),
        "dpm/prediction_type": lambda: make("dpm", prediction_type="flow_prediction"),
        "dpm/lambda_min_clipped": lambda: make("dpm", lambda_min_clipped=-5.1),
        "dpm/lambda_min_clipped_inf": lambda: make("dpm", lambda_min_clipped=float("inf")),
        "dpm/variance_type": lambda: make("dpm", variance_type="learned"),
        "dpm/karras_and_exponential": lambda: make("dpm", use_karras_sigmas=True, use_exponential_sigmas=True),
        "dpm/final_sigmas_type": lambda: make("dpm", final_sigmas_type="one"),
        "dpm/beta_schedule": lambda: make("dpm", beta_schedule="squaredcos_cap_v2"),
        "dpm/custom_timesteps": lambda: make("dpm").set_timesteps(timesteps=[9, 6]),
        "dpm/set_timesteps_nothing": lambda: make("dpm").set_timesteps(),
        "dpm/spacing": lambda: ready("dpm", timestep_spacing="even"),
        "dpm/non_finite_rows": lambda: ready("dpm", n=16, **_TRAINED),       # repeated sigmas: r0 = 0
        "dpm/step_before_set_timesteps": step("dpm", sch=lambda: make("dpm")),
        "dpm/step_inplace_before_set_timesteps": step("dpm", sch=lambda: make("dpm"), entry="step_inplace"),
        "dpm/step_past_the_end": past_the_end("dpm"),
        "dpm/step_cfg_other_out": other_out("dpm"),
    }
    for flag in ("thresholding", "use_beta_sigmas", "use_lu_lambdas", "use_flow_sigmas", "rescale_betas_zero_snr",
                 "use_dynamic_shifting"):
        e[f"dpm/{flag}"] = lambda flag=flag: make("dpm", **{flag: True})
    return e


CASES, ERRORS = _cases(), _errors()
PROBE = "libm_probe"        # the golden file's entries of ``libm_probe()``


def libm_probe():
    """fp32 results of the libm functions the schedulers' host math calls -- ``pow``, ``log``, ``expm1``, as 1000-element tensor ops
    and as 0-d ones -- on fixed inputs, computed here without diffusers_amd/schedulers.py.  They are not correctly rounded, so a
    host whose torch picks another implementation gives other last bits: the golden file holds the recording host's, and where a
    host reproduces them every case has to match bit for bit.  Inputs: k / 1024 (exact), and the sigma(t) of the two beta schedules
    -- the very ``pow`` every fp32 ladder starts with."""
    x = torch.arange(1, 1001, dtype=torch.float32) / 1024
    out = {"pow": x ** 0.5, "log": torch.log(x), "expm1": torch.expm1(-4 * x), "pow_of_ratio": ((1 - x) / x) ** 0.5,
           "pow_int": torch.pow(x[:16], 3)}
    for fn in ("pow", "log", "expm1"):
        f = {"pow": lambda v: v ** 0.5, "log": torch.log, "expm1": lambda v: torch.expm1(-4 * v)}[fn]
        out[f"{fn}_0d"] = torch.stack([f(v) for v in x[::5]])
    for name, betas in (("linear", torch.linspace(0.0001, 0.02, 1000, dtype=torch.float32)),
                        ("scaled_linear", torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2)):
        ac = torch.cumprod(1.0 - betas, dim=0)
        out[f"sigma_{name}"] = ((1 - ac) / ac) ** 0.5
    return {k: v.numpy().copy() for k, v in out.items()}


def record(name):
    """One valid case: ``(arrays, meta)``."""
    with torch.random.fork_rng():
        run = CASES[name]()
    return run.arrays, json.loads(json.dumps(run.meta))


def record_error(name):
    """One refused call: the exception's type name and message ("no error" when the call goes through)."""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (numpy's divide-by-zero warnings on the way to the non-finite-rows refusals)
            ERRORS[name]()
    except Exception as exc:        # noqa: BLE001  (whatever the call raises is what is recorded)
        return {"type": type(exc).__name__, "message": str(exc)}
    return {"type": None, "message": "no error"}
