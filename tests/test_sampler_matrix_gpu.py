"""GPU: every instantiation csrc/sampler.hip's entry points can launch, through ``ops`` (one C entry point directly).

The entry points pick a kernel instantiation from (dtype[, second dtype], cfg, pred_type) and the two 4-wide kernels pick a vector /
scalar split from the operands' addresses.  A wrong pick launches a kernel that runs and returns plausible numbers, so every accepted
combination is run here and held to three kinds of equality; none has a tolerance of its own.

a. Fused equals unfused: the ``cfg=True`` result on ``[uncond; cond]`` is ``torch.equal`` to the ``cfg=False`` result on
   ``oracle.samplers.cfg_combine(uncond, cond, g)`` for g in {5.0, 7.5} (both exact in bf16: torch's CPU handling of the scalar
   cannot differ from the device's).
b. Vector path equals scalar path (DPM-Solver++ 2M, Euler ancestral): the result on 16-byte aligned operands is ``torch.equal`` to the
   result with one operand starting one element into its allocation, which makes the launch all-scalar.  Every operand sits in a
   ``footprint.guarded`` buffer, so the bands around it are checked as well.
c. One anchor per kernel: each ``cfg=False`` result equals the bit-exact reference the project has -- oracle/samplers.py with
   ``device_scalars=True`` (Euler, DDIM, DDPM, FlowMatch, UniPC), ``lcm_emulation.ref_step_row`` (LCM),
   ``test_euler_ancestral_cpu.ref_step_row`` (Euler ancestral).  DPM-Solver++ is pinned bit for bit nowhere: it gets the float64
   comparison and the gate of ``test_dpmsolver_gpu.test_one_step_against_float64``, unchanged.

Sizes: n in {1, 3, 4, 1027, 1028}: below one vector, one vector, one full 256-thread workgroup of vectors plus a three-element tail
(1027 = 4 * 256 + 3), and the multiple of 4 the CFG vector path needs.  A bf16 Euler-ancestral launch with CFG needs a multiple of 8
(the cond half 16-byte aligned), so the 4-wide kernels also run 1032.  ``ew_grid`` caps a launch at 2048 workgroups of 256 threads;
one size per loop form lies past the cap so that the grid stride is taken: cap + 261 elements for the scalar kernels, 4 * cap + 23 for
the 4-wide ones (and 4 * cap + 24 so that the CFG vector loop strides too), for one bf16 / epsilon case per kernel and both ``cfg``."""
import pytest
import torch

import footprint as FP
import lcm_emulation
from test_dpmsolver_cpu import SD_BETAS
from test_dpmsolver_gpu import _check_step as dpm_check_step, _combine as dpm_combine
from test_euler_ancestral_cpu import ref_step_row as euler_a_ref_step_row

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
bf16, f32 = torch.bfloat16, torch.float32
DT = {"bf16": bf16, "f32": f32}
PREDS = ("epsilon", "v_prediction", "sample")

GRID_CAP = 2048 * 256                       # ew_grid: at most 2048 workgroups of 256 threads
SMALL = (1, 3, 4, 1027, 1028)
SMALL_WIDE = SMALL + (1032,)
BIG_SCALAR = GRID_CAP + 261
BIG_WIDE = (4 * GRID_CAP + 23, 4 * GRID_CAP + 24)
GUIDANCE = (5.0, 7.5)
BAND = 1024                                 # guard band of the path tests, elements (a multiple of 8: 16-byte aligned views)


def _ops():
    from diffusers_amd import _lib as L, ops
    return ops, L


def _randn(n, seed, rows=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n,) if rows is None else (rows, n), generator=g)


def _step(r):
    return torch.full((), r, dtype=torch.int32, device=DEV)


def _model_output(u, c, cfg, g):
    """(what the fused launch gets, what the unfused launch gets)."""
    from oracle import samplers as OS
    return torch.cat([u, c]).contiguous(), OS.cfg_combine(u, c, g)


def _sizes(small, big, dt_name, pred):
    """The small sizes for every case, the sizes past the grid cap for the one bf16 / epsilon case of a kernel."""
    big = big if isinstance(big, tuple) else (big,)
    return small + (big if dt_name in ("bf16", "bf16-bf16") and pred in (None, "epsilon") else ())


# ----------------------------------------------------------------------------------------------------------------------
# da_euler_step: 2 dtypes x 2 cfg x 3 prediction types
# ----------------------------------------------------------------------------------------------------------------------
EULER_KW = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1, timestep_spacing="leading")


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_euler_step(dt_name, pred):
    from diffusers_amd import schedulers as S
    from oracle import samplers as OS
    ops, L = _ops()
    dt, r = DT[dt_name], 2
    e = S.EulerDiscreteScheduler(prediction_type=pred, **EULER_KW)
    e.set_timesteps(5, device=DEV)
    o = OS.EulerOracle(device_scalars=True, prediction_type=pred, **EULER_KW)
    o.set_timesteps(5)
    assert torch.equal(e.sigmas, o.sigmas)
    table, step = e.device_table, _step(r)
    for n in _sizes(SMALL, BIG_SCALAR, dt_name, pred):
        x = (_randn(n, 1) * float(o.sigmas[r])).to(dt)
        u, c = _randn(n, 2).to(dt), _randn(n, 3).to(dt)
        run = lambda eps, cfg, g=0.0: ops.euler_step(eps.to(DEV), x.to(DEV), table, step, cfg=cfg, guidance=g,  # noqa: E731
                                                     pred_type=L.PRED_TYPES[pred]).cpu()
        o.step_index = r
        assert torch.equal(run(c, False), o.step(c, x)), (n, "anchor")
        for g in GUIDANCE:
            fused, plain = _model_output(u, c, True, g)
            assert torch.equal(run(fused, True, g), run(plain, False)), (n, g)


# ----------------------------------------------------------------------------------------------------------------------
# da_euler_scale_model_input, da_mul_scalar, da_cast_f32_bf16: the three replicate-store kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [1, 2, 3])
def test_replicate_store_kernels(rep):
    from diffusers_amd import schedulers as S
    from oracle import samplers as OS
    ops, L = _ops()
    e = S.EulerDiscreteScheduler(**EULER_KW)
    e.set_timesteps(5, device=DEV)
    o = OS.EulerOracle(device_scalars=True, **EULER_KW)
    o.set_timesteps(5)
    o.step_index = 2
    step = _step(2)
    for dt_name, dt in DT.items():
        for n in _sizes(SMALL, BIG_SCALAR, dt_name, None):
            x = (_randn(n, 4) * 3.0).to(dt).reshape(1, n)
            want = torch.cat([o.scale_model_input(x)] * rep)
            assert torch.equal(ops.euler_scale_model_input(x.to(DEV), e.device_table, step, rep=rep).cpu(), want), (dt_name, n, "scale")
            want = torch.cat([x * 13.75] * rep)                            # 13.75 is exact in bf16
            assert torch.equal(ops.mul_scalar(x.to(DEV), 13.75, rep=rep).cpu(), want), (dt_name, n, "mul_scalar")
    for n in SMALL + (BIG_SCALAR,):
        x = (_randn(n, 5) * 3.0).reshape(1, n)
        assert torch.equal(ops.cast_f32_bf16(x.to(DEV), rep=rep).cpu(), torch.cat([x.to(bf16)] * rep)), (n, "cast")


# ----------------------------------------------------------------------------------------------------------------------
# da_x0_linear_step: 2 dtypes x 2 cfg x 6 pred_type (DDIM / DDPM 0-2, the consistency update 4-6)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_x0_linear_step_ddim_and_ddpm(dt_name, pred):
    """DDIM (eta = 0: no noise operand) and DDPM (ancestral noise) rows through the same instantiations."""
    from diffusers_amd import schedulers as S
    from oracle import samplers as OS
    ops, L = _ops()
    dt, r = DT[dt_name], 2
    dk = dict(clip_sample=False, set_alpha_to_one=False, steps_offset=1, prediction_type=pred, **SD_BETAS)
    d, od = S.DDIMScheduler(**dk), OS.DDIMOracle(device_scalars=True, **dk)
    d.set_timesteps(5, device=DEV), od.set_timesteps(5)
    d.ensure_table(0.0)
    pk = dict(prediction_type=pred, clip_sample=True)
    p, op_ = S.DDPMScheduler(**pk), OS.DDPMOracle(device_scalars=True, **pk)
    p.set_timesteps(5, device=DEV), op_.set_timesteps(5)
    step = _step(r)
    for n in _sizes(SMALL, BIG_SCALAR, dt_name, pred):
        x, u, c, nz = (_randn(n, s).to(dt) for s in (6, 7, 8, 9))
        for name, table, use_noise, ref in (
                ("ddim", d.device_table, False, lambda e: od.step(e, od.timesteps[r], x)),
                ("ddpm", p.device_table, True, lambda e: op_.step(e, op_.timesteps[r], x, noise=nz))):
            run = lambda eps, cfg, g=0.0: ops.x0_linear_step(eps.to(DEV), x.to(DEV), nz.to(DEV) if use_noise else None,  # noqa: E731
                                                             table, step, cfg=cfg, guidance=g, pred_type=L.PRED_TYPES[pred]).cpu()
            assert torch.equal(run(c, False), ref(c)), (name, n, "anchor")
            for g in GUIDANCE:
                fused, plain = _model_output(u, c, True, g)
                assert torch.equal(run(fused, True, g), run(plain, False)), (name, n, g)


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_x0_linear_step_consistency_update(dt_name, pred):
    """pred_type 4-6 on a row that adds noise (1) and on the last row of the schedule, which does not read it."""
    from diffusers_amd import schedulers as S
    ops, L = _ops()
    dt = DT[dt_name]
    s = S.LCMScheduler()
    s.set_timesteps(4, device=DEV)
    table = s.device_table
    rows = table.cpu()
    pt = L.PRED_LCM + L.PRED_TYPES[pred]
    assert float(rows[1, 5]) != 0.0 and float(rows[3, 5]) == 0.0
    for r in (1, 3):
        step = _step(r)
        for n in _sizes(SMALL, BIG_SCALAR, dt_name, pred if r == 1 else "skip"):
            x, u, c, nz = (_randn(n, s_).to(dt) for s_ in (10, 11, 12, 13))
            run = lambda eps, cfg, g=0.0: ops.x0_linear_step(eps.to(DEV), x.to(DEV), nz.to(DEV), table, step, cfg=cfg,  # noqa: E731
                                                             guidance=g, pred_type=pt).cpu()
            assert torch.equal(run(c, False), lcm_emulation.ref_step_row(c, x, nz, rows[r], pred_type=pt)), (r, n, "anchor")
            for g in GUIDANCE:
                fused, plain = _model_output(u, c, True, g)
                assert torch.equal(run(fused, True, g), run(plain, False)), (r, n, g)


# ----------------------------------------------------------------------------------------------------------------------
# da_flowmatch_step, da_unipc_flow_step: 3 (sample, model output) dtype pairs x 2 cfg
# ----------------------------------------------------------------------------------------------------------------------
FLOW_PAIRS = [("bf16-bf16", bf16, bf16), ("f32-f32", f32, f32), ("f32-bf16", f32, bf16)]


@pytest.mark.parametrize("name,xd,vd", FLOW_PAIRS)
def test_flowmatch_step(name, xd, vd):
    from diffusers_amd import schedulers as S
    from oracle import samplers as OS
    ops, L = _ops()
    r = 2
    f = S.FlowMatchEulerDiscreteScheduler(shift=3.0)
    f.set_timesteps(6, device=DEV)
    of = OS.FlowMatchOracle(shift=3.0, device_scalars=True)
    of.set_timesteps(6)
    assert torch.equal(f.sigmas.cpu(), of.sigmas)
    table, step = f.device_table, _step(r)
    for n in _sizes(SMALL, BIG_SCALAR, name, None):
        x, u, c = _randn(n, 14).to(xd), _randn(n, 15).to(vd), _randn(n, 16).to(vd)
        run = lambda v, cfg, g=0.0: ops.flowmatch_step(v.to(DEV), x.to(DEV), table, step, cfg=cfg, guidance=g).cpu()  # noqa: E731
        of.step_index = r
        got = run(c, False)
        assert got.dtype == vd and torch.equal(got, of.step(c, x)), (n, "anchor")
        for g in GUIDANCE:
            fused, plain = _model_output(u, c, True, g)
            assert torch.equal(run(fused, True, g), run(plain, False)), (n, g)


@pytest.mark.parametrize("name,xd,vd", FLOW_PAIRS)
def test_unipc_flow_step(name, xd, vd):
    """Three consecutive steps, so that the first-order row, the corrector and both second-order branches run; the sample and the
    three history tensors are updated in place and all four are compared."""
    from diffusers_amd import schedulers as S
    from oracle import samplers as OS
    ops, L = _ops()
    sch = S.UniPCMultistepScheduler(prediction_type="flow_prediction", use_flow_sigmas=True, flow_shift=3.0)
    sch.set_timesteps(7, device=DEV)
    coef = sch._coef
    for n in _sizes(SMALL, BIG_SCALAR, name, None):
        orc = OS.UniPCFlowOracle(flow_shift=3.0, device_scalars=True)
        orc.set_timesteps(7)
        x0 = _randn(n, 17, rows=1).to(xd)                                   # [1][n]: the oracle's einsum wants a batch dim
        states = {k: [x0.to(DEV)] + [torch.zeros((1, n), dtype=xd, device=DEV) for _ in range(3)] for k in ("anchor",) + GUIDANCE}
        xo = x0.clone()
        for i in range(3):
            u, c = _randn(n, 18 + 2 * i, rows=1).to(vd), _randn(n, 19 + 2 * i, rows=1).to(vd)
            step = _step(i)
            ops.unipc_flow_step_(c.to(DEV), *states["anchor"], coef, step)
            xo = orc.step(c, xo)
            assert torch.equal(states["anchor"][0].cpu(), xo), (n, i, "anchor")
            for g in GUIDANCE:
                fused, plain = _model_output(u, c, True, g)
                unfused = [t.clone() for t in states[g]]
                ops.unipc_flow_step_(fused.to(DEV), *states[g], coef, step, cfg=True, guidance=g)
                ops.unipc_flow_step_(plain.to(DEV), *unfused, coef, step)
                for a, b, what in zip(states[g], unfused, ("x", "last", "m1", "m2")):
                    assert torch.equal(a, b), (n, i, g, what)


# ----------------------------------------------------------------------------------------------------------------------
# The two 4-wide kernels.  Operands live in guarded buffers; `shift` names the one that starts an element late (None: all aligned).
# ----------------------------------------------------------------------------------------------------------------------
def _boxed(values, dtype, late):
    b = FP.guarded((values.numel(),), dtype=dtype, lead=BAND + int(late), trail=BAND)
    b.set(values.reshape(-1))
    assert (b.ptr() % 16 != 0) == bool(late)
    return b


DPM_PAIRS = [("bf16-bf16", bf16, bf16), ("bf16-f32", bf16, f32), ("f32-bf16", f32, bf16), ("f32-f32", f32, f32)]


def _dpm_run(table, step, begin, x, eps, m1, xd, ed, cfg, g, pred, shift=None):
    """One da_dpmpp_2m_step on guarded operands -> (next sample, history), both on the host, guards checked."""
    ops, L = _ops()
    xb, eb, mb = _boxed(x, xd, shift == "x"), _boxed(eps, ed, shift == "eps"), _boxed(m1, f32, shift == "m1")
    ops.dpmpp_2m_step_(eb.view, xb.view, mb.view, table, step, begin, cfg=cfg, guidance=g, pred_type=L.PRED_TYPES[pred])
    torch.cuda.synchronize()
    for b, what in ((xb, "sample"), (eb, "model output"), (mb, "history")):
        b.check(f"dpmpp_2m {what} (shift={shift})")
    assert torch.equal(eb.view.cpu(), eps.reshape(-1).to(ed)), "the model output is read only"
    return xb.view.cpu(), mb.view.cpu()


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("name,xd,ed", DPM_PAIRS)
def test_dpmpp_2m_step(name, xd, ed, pred):
    """4 dtype pairs x 2 cfg x 3 prediction types, on a second-order row (the history is read) -- a, b and the float64 gate."""
    from test_dpmsolver_gpu import _sched
    ops, L = _ops()
    table = _sched(20, use_karras_sigmas=True).device_table
    rows = table.cpu().numpy()
    r = 10
    step, begin = _step(r), _step(0)
    assert rows[r, 6] != 0
    for n in _sizes(SMALL_WIDE, BIG_WIDE, name, pred):
        x = (_randn(n, 24) * float(rows[r, 1] / rows[r, 0] + 1.0)).to(xd)
        m1 = _randn(n, 25)
        u, c = _randn(n, 26).to(ed), _randn(n, 27).to(ed)
        run = lambda eps, cfg, g=0.0, shift=None: _dpm_run(table, step, begin, x, eps, m1, xd, ed, cfg, g, pred, shift)  # noqa: E731
        got_x, got_m1 = run(c, False)
        dpm_check_step(got_x, got_m1, x, dpm_combine(c, False, 0.0, (n,)), m1, rows[r], True, L.PRED_TYPES[pred], xd, (name, pred, n))
        for shift in ("x", "eps", "m1"):
            sx, sm = run(c, False, shift=shift)
            assert torch.equal(sx, got_x) and torch.equal(sm, got_m1), (n, "scalar path", shift)
        for g in GUIDANCE:
            fused, plain = _model_output(u, c, True, g)
            fx, fm = run(fused, True, g)
            px, pm = run(plain, False)
            assert torch.equal(fx, px) and torch.equal(fm, pm), (n, g)
            for shift in ("x", "eps", "m1") if g == GUIDANCE[0] else ():
                sx, sm = run(fused, True, g, shift=shift)
                assert torch.equal(sx, fx) and torch.equal(sm, fm), (n, g, "scalar path", shift)


def _euler_a_run(table, step, x, eps, nz, dt, cfg, g, pred, shift=None):
    ops, L = _ops()
    xb, eb, nb = _boxed(x, dt, shift == "x"), _boxed(eps, dt, shift == "eps"), _boxed(nz, dt, shift == "noise")
    ob = FP.guarded((x.numel(),), dtype=dt, lead=BAND + int(shift == "out"), trail=BAND)
    y = ops.euler_ancestral_step(eb.view, xb.view, nb.view, table, step, cfg=cfg, guidance=g, out=ob.view,
                                 pred_type=L.PRED_TYPES[pred])
    torch.cuda.synchronize()
    assert y.data_ptr() == ob.ptr()
    for b, what in ((xb, "sample"), (eb, "model output"), (nb, "noise"), (ob, "out")):
        b.check(f"euler_ancestral {what} (shift={shift})")
    for b, v in ((xb, x), (eb, eps), (nb, nz)):
        assert torch.equal(b.view.cpu(), v.reshape(-1).to(dt)), "inputs are read only"
    return ob.view.cpu()


@pytest.mark.parametrize("pred", PREDS[:2])
@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_euler_ancestral_step(dt_name, pred):
    """2 dtypes x 2 cfg x 2 prediction types on a row that adds noise -- a, b and the anchor."""
    from diffusers_amd import schedulers as S
    ops, L = _ops()
    dt, r = DT[dt_name], 2
    s = S.EulerAncestralDiscreteScheduler(prediction_type=pred, **SD_BETAS)
    s.set_timesteps(5, device=DEV)
    table = s.device_table
    rows = table.cpu()
    assert float(rows[r, 6]) != 0.0
    step = _step(r)
    for n in _sizes(SMALL_WIDE, BIG_WIDE, dt_name, pred):
        x = (_randn(n, 28) * float(rows[r, 0])).to(dt)
        u, c, nz = (_randn(n, s_).to(dt) for s_ in (29, 30, 31))
        run = lambda eps, cfg, g=0.0, shift=None: _euler_a_run(table, step, x, eps, nz, dt, cfg, g, pred, shift)  # noqa: E731
        got = run(c, False)
        assert torch.equal(got, euler_a_ref_step_row(c, x, nz, rows[r], pred_type=L.PRED_TYPES[pred])), (n, "anchor")
        for shift in ("x", "eps", "noise", "out"):
            assert torch.equal(run(c, False, shift=shift), got), (n, "scalar path", shift)
        for g in GUIDANCE:
            fused, plain = _model_output(u, c, True, g)
            fo = run(fused, True, g)
            assert torch.equal(fo, run(plain, False)), (n, g)
            for shift in ("x", "eps", "noise", "out") if g == GUIDANCE[0] else ():
                assert torch.equal(run(fused, True, g, shift=shift), fo), (n, g, "scalar path", shift)


# ----------------------------------------------------------------------------------------------------------------------
# da_cfg_rescale: guidance_rescale (statistics + apply) and DA_CFG_IMAGE_GUIDANCE (three-way combine)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_cfg_rescale_apply(dt_name):
    """The apply pass against the formula in torch ops on the device, fed the per-sample ratio the statistics pass stored (that pass
    is a reduction, pinned by test_kernels_gpu.test_cfg_rescale_matches_the_reference_bit_for_bit): every product and sum is
    rounded in the tensor dtype and the scalars stay fp32 on both sides, so the comparison is for equality."""
    ops, L = _ops()
    dt, gr = DT[dt_name], 0.75                                          # exact in bf16, and so is 1 - 0.75
    for B, n_per in [(2, n) for n in SMALL[1:]] + ([(1, BIG_SCALAR)] if dt == bf16 else []):
        eps = _randn(n_per, 32, rows=2 * B).to(dt).to(DEV)
        for g in GUIDANCE:
            out = torch.empty((B, n_per), dtype=dt, device=DEV)
            ws = torch.zeros((B,), dtype=f32, device=DEV)
            L.check(L.load().da_cfg_rescale(eps.data_ptr(), out.data_ptr(), ws.data_ptr(), B, n_per, g, gr, L.DTYPE_BF16 if dt == bf16 else L.DTYPE_F32,
                                            torch.cuda.current_stream().cuda_stream), "da_cfg_rescale")
            u, c = eps[:B], eps[B:]
            cv = u + g * (c - u)
            want = gr * (cv * ws.to(dt)[:, None]) + (1 - gr) * cv
            assert torch.equal(out, want), (B, n_per, g)
            assert torch.equal(ops.cfg_rescale(eps, g, gr), out), (B, n_per, g, "ops")


@pytest.mark.parametrize("dt_name", ["bf16", "f32"])
def test_cfg_image_guidance(dt_name):
    ops, L = _ops()
    dt = DT[dt_name]
    for n in _sizes(SMALL, BIG_SCALAR, dt_name, None):
        eps = _randn(n, 33, rows=3).to(dt).to(DEV)
        t, i, u = eps.chunk(3)
        for g in GUIDANCE:
            assert torch.equal(ops.cfg_combine3(eps, g, 1.5), u + g * (t - i) + 1.5 * (i - u)), (n, g)
