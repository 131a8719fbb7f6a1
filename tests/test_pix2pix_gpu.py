"""GPU: the two InstructPix2Pix kernel forms to the bit against the compositions they replace (the 8-channel conv_in from two
sources = ops.conv_thin_in on the reference's concatenation; the three-way guidance = the live torch expression), their refusals,
memory footprint and launch-plan replay, the SD1.5 / SDXL InstructPix2Pix pipelines against a hand-written loop over the same
engine components (eager = HIP graph = launch plan, no re-capture for another image), their accuracy against an fp32 oracle loop
restated here, and -- where the reference archive shipped -- against the reference's own pipelines."""
import numpy as np
import pytest
import torch

import value_domain as vd
from oracle import ref_runtime as RR
from oracle import reference_math as R
from oracle.samplers import DDIMOracle, EulerOracle
from test_kernel_footprint_gpu import _check, _p, _stream, run_both
from test_vae_encode_gpu import encoder_ref
from footprint import guarded, poisoned

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16
f32 = torch.float32
DA_ERR_INVALID, DA_ERR_UNSUPPORTED = 1, 3      # include/diffusers_amd.h


def _euler(steps=6):
    from diffusers_amd import factory
    from diffusers_amd.schedulers import EulerDiscreteScheduler
    sch = EulerDiscreteScheduler(**factory.SDXL_SCHEDULER)
    sch.set_timesteps(steps, device=DEV)
    return sch


def _concat(xs, img, rep):
    """The reference's conv_in input: cat([cat([s(x)] * rep), cat([img, img, zeros_like(img)][:rep])], dim=1)."""
    B = xs.shape[0] // rep
    im = img.expand(B, -1, -1, -1)
    return torch.cat([xs, torch.cat([im, im, torch.zeros_like(im)][:rep])], dim=1).contiguous()


# ---- K1: conv_in from two sources ----------------------------------------------------------------------------------------
_K1_CASES = [(rep, sc, co, hw, 1, 1) for rep in (1, 3) for sc in (True, False) for co in (8, 64, 320)
             for hw in ((1, 1), (9, 13), (17, 30), (64, 64))] + [(rep, True, 64, (9, 13), 2, Bm) for rep in (1, 3) for Bm in (1, 2)]


@pytest.mark.parametrize("rep,scaled,cout,hw,B,Bm", _K1_CASES)
def test_conv_in_pix2pix_is_conv_thin_in_on_the_concatenation_to_the_bit(rep, scaled, cout, hw, B, Bm):
    from diffusers_amd import ops
    g = torch.Generator().manual_seed(13)
    H, W_ = hw
    x = torch.randn(B, 4, H, W_, generator=g).to(bf16).to(DEV)
    img = torch.randn(Bm, 4, H, W_, generator=g).to(bf16).to(DEV)
    w4 = (torch.randn(cout, 8, 3, 3, generator=g) * 0.2).to(bf16).to(DEV)
    w = ops.pack_conv_weight(w4)
    bias = torch.randn(cout, generator=g).to(bf16).to(DEV)
    sch = _euler()
    step = sch.device_step
    step.fill_(3)
    tab = dict(table=sch.device_table, step_idx=step) if scaled else {}
    got = ops.conv_in_pix2pix(x, img, w, bias, rep=rep, **tab)
    xs = ops.euler_scale_model_input(x, sch.device_table, step, rep=rep) if scaled else torch.cat([x] * rep)
    cat = _concat(xs, img, rep)
    want = ops.conv_thin_in(cat, w, bias, ksize=3, in_nchw=True)
    assert tuple(got.shape) == (rep * B, H, W_, cout) and torch.equal(got, want)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "equal values but other bits: the sign of a zero"
    # without bias
    got_nb = ops.conv_in_pix2pix(x, img, w, None, rep=rep, **tab)
    assert torch.equal(got_nb.view(torch.int16), ops.conv_thin_in(cat, w, None, ksize=3, in_nchw=True).view(torch.int16))
    if rep == 3:
        assert torch.equal(got[:B], got[B:2 * B]), "the text and image rows have identical inputs"
        wz = w4.clone()
        wz[:, 4:] = 0
        only4 = ops.conv_thin_in(_concat(xs[:B], img, 1), ops.pack_conv_weight(wz), bias, ksize=3, in_nchw=True)
        assert torch.equal(got[2 * B:], only4), "the unconditional row is the conv of the latents alone"
        assert not torch.equal(got[2 * B:], got[:B])


# ---- K2: three-way guidance ----------------------------------------------------------------------------------------------
def _same_bits_or_both_nan(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    a, b = a.masked_fill(na, 0), b.masked_fill(nb, 0)
    return torch.equal(a.view(torch.int16 if a.dtype == bf16 else torch.int32), b.view(torch.int16 if b.dtype == bf16 else torch.int32))


def _torch_combine(eps, g, ig):
    t, i, u = eps.chunk(3)
    return u + g * (t - i) + ig * (i - u)


@pytest.mark.parametrize("scales", [(7.5, 1.5), (1.0, 1.0), (3.3, 2.7)])
@pytest.mark.parametrize("dt", [bf16, f32])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n_per", [1, 7, 256, 16384, 2048 * 256 + 3])
def test_cfg_combine3_is_the_torch_expression_to_the_bit(n_per, B, dt, scales):
    """n_per = 2048 * 256 + 3 is more than one sweep of the capped grid (2048 blocks of 256): the stride loop runs."""
    from diffusers_amd import ops
    g, ig = scales
    eps = torch.randn(3 * B, n_per, generator=torch.Generator().manual_seed(17)).to(dt).to(DEV)
    got = ops.cfg_combine3(eps, g, ig)
    want = _torch_combine(eps, g, ig)
    assert got.dtype == want.dtype == dt and tuple(got.shape) == (B, n_per)
    assert torch.equal(got.view(torch.int16 if dt == bf16 else torch.int32), want.view(torch.int16 if dt == bf16 else torch.int32))
    out = torch.empty_like(got)
    assert ops.cfg_combine3(eps, g, ig, out=out).data_ptr() == out.data_ptr() and torch.equal(out, got)


@pytest.mark.parametrize("scales", [(7.5, 1.5), (3.3, 2.7)])
def test_cfg_combine3_over_every_finite_bf16_value(scales):
    """Each of the three rows runs over every finite bf16 value (two of them in a seeded permutation): differences that cancel,
    overflow to infinity and inf - inf = NaN included, where the kernel and torch have to agree as well."""
    from diffusers_amd import ops
    v = vd.all_finite_bf16()
    gp = torch.Generator().manual_seed(5)
    rows = torch.stack([v, v[torch.randperm(v.numel(), generator=gp)], v[torch.randperm(v.numel(), generator=gp)]])
    for order in ((0, 1, 2), (1, 0, 2), (2, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 0)):
        eps = rows[list(order)].contiguous().to(DEV)
        got, want = ops.cfg_combine3(eps, *scales), _torch_combine(eps, *scales)
        assert _same_bits_or_both_nan(got, want), order


def test_cfg_combine3_reduces_for_zero_scales():
    from diffusers_amd import ops
    eps = torch.randn(6, 4, 9, 13, generator=torch.Generator().manual_seed(19)).to(bf16).to(DEV)
    t, i, u = eps.chunk(3)
    # ig = 0: uncond + g (text - image), the second term an exact zero
    assert torch.equal(ops.cfg_combine3(eps, 7.5, 0.0), u + 7.5 * (t - i))
    # g = 0: uncond + ig (image - uncond), the two-way combine of the image row over the unconditional one
    assert torch.equal(ops.cfg_combine3(eps, 0.0, 1.5), u + 1.5 * (i - u))
    assert torch.equal(ops.cfg_combine3(eps, 0.0, 0.0), u)


# ---- refusals through the C ABI ------------------------------------------------------------------------------------------
def test_entry_points_refuse_the_undefined_combinations():
    from diffusers_amd import _lib as L, ops
    lib = L.load()
    B, H, W_, Cout = 2, 5, 6, 8
    x, img = (torch.zeros(B, 4, H, W_, dtype=bf16, device=DEV) for _ in range(2))
    mask = torch.zeros(B, 1, H, W_, dtype=bf16, device=DEV)
    w8, w9 = torch.zeros(Cout, 72, dtype=bf16, device=DEV), torch.zeros(Cout, 81, dtype=bf16, device=DEV)
    y = torch.zeros(3 * B, H, W_, Cout, dtype=bf16, device=DEV)

    def conv(mask_, w_, rep, Bm=B, masked=img):
        return lib.da_conv_in_inpaint(x.data_ptr(), _p(mask_), _p(masked), w_.data_ptr(), None, y.data_ptr(), None, None, B, H, W_, Cout,
                                      rep, Bm, _stream())
    assert conv(mask, w9, 3) == DA_ERR_INVALID           # three rows belong to the NULL-mask form
    assert conv(None, w8, 2) == DA_ERR_INVALID           # two rows belong to the inpainting form
    assert conv(None, w8, 0) == DA_ERR_INVALID and conv(None, w8, 4) == DA_ERR_INVALID
    assert conv(None, w8, 3, Bm=3) == DA_ERR_INVALID and conv(None, w8, 3, masked=None) == DA_ERR_INVALID
    assert conv(None, w8, 3) == L.DA_OK and conv(None, w8, 1) == L.DA_OK and conv(mask, w9, 2) == L.DA_OK
    eps = torch.zeros(3, 8, dtype=bf16, device=DEV)
    out = torch.zeros(1, 8, dtype=bf16, device=DEV)
    flag = L.CFG_IMAGE_GUIDANCE

    def comb(e, o, Bc, n, code):
        return lib.da_cfg_rescale(_p(e), _p(o), None, Bc, n, 7.5, 1.5, code, _stream())
    assert comb(eps, out, 1, 8, flag | L.DTYPE_BF16) == L.DA_OK
    assert comb(eps, out, 1, 8, L.DTYPE_BF16) == DA_ERR_INVALID      # without the flag a NULL ratio_ws stays refused
    assert comb(None, out, 1, 8, flag) == DA_ERR_INVALID and comb(eps, None, 1, 8, flag) == DA_ERR_INVALID
    assert comb(eps, out, 0, 8, flag) == DA_ERR_INVALID and comb(eps, out, 1, 0, flag) == DA_ERR_INVALID
    assert comb(eps, out, 1, 8, flag | 2) == DA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="rep must be 1 or 3"):
        ops.conv_in_pix2pix(x, img, w8, None, rep=2)
    with pytest.raises(ValueError, match=r"\[Cout\]\[72\]"):
        ops.conv_in_pix2pix(x, img, w9, None)
    with pytest.raises(ValueError, match="image_latents"):
        ops.conv_in_pix2pix(x, img[:, :3].contiguous(), w8, None)
    with pytest.raises(ValueError, match="3 B rows"):
        ops.cfg_combine3(torch.zeros(4, 8, dtype=bf16, device=DEV), 7.5, 1.5)
    with pytest.raises(ValueError, match="out must be"):
        ops.cfg_combine3(eps, 7.5, 1.5, out=torch.zeros(2, 8, dtype=bf16, device=DEV))


# ---- footprint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [1, 3])
def test_conv_in_pix2pix_footprint(rep):
    """17 x 30 runs the W tail of the four-pixel form; NULL mask, sources and weight between poisoned bands, guarded output."""
    import torch.nn.functional as F
    from conftest import assert_close_bf16
    from diffusers_amd import _lib as L, ops
    lib, B, H, W_, Cout = L.load(), 2, 17, 30, 64

    def rnd(shape, seed, scale=1.0):
        return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(bf16).to(DEV)
    x, img = rnd((B, 4, H, W_), 700), rnd((B, 4, H, W_), 701)
    w8, b = rnd((Cout, 8, 3, 3), 702, 72 ** -0.5), rnd((Cout,), 703, 0.1)
    y = run_both("conv_in_pix2pix", lambda i, o: _check(L, lib.da_conv_in_inpaint(_p(i["x"]), None, _p(i["img"]), _p(i["w"]), _p(i["b"]), _p(o["y"]),
                                                                                  None, None, B, H, W_, Cout, rep, B, _stream()), "pix2pix_in"),
                 dict(x=poisoned(x), img=poisoned(img), w=poisoned(ops.pack_conv_weight(w8)), b=poisoned(b)),
                 lambda: dict(y=guarded((rep * B, H, W_, Cout))))["y"]
    ref = F.conv2d(_concat(torch.cat([x] * rep), img, rep).float(), w8.float(), b.float(), padding=1).permute(0, 2, 3, 1)
    assert_close_bf16(y, ref, f"conv_in_pix2pix rep {rep}", rtol=8e-3, atol_rms=4e-3)


@pytest.mark.parametrize("dt", [bf16, f32])
@pytest.mark.parametrize("n", [1, 7, 4097])
def test_cfg_combine3_footprint(n, dt):
    from conftest import assert_close_bf16
    from diffusers_amd import _lib as L
    B, g, ig = 2, 7.5, 1.5
    eps = torch.randn(3, B, n, generator=torch.Generator().manual_seed(150)).to(dt).to(DEV)
    code = (L.DTYPE_F32 if dt == f32 else L.DTYPE_BF16) | L.CFG_IMAGE_GUIDANCE
    r = run_both(f"cfg_combine3 n{n}", lambda i, o: _check(L, L.load().da_cfg_rescale(_p(i["eps"]), _p(o["y"]), None, B, n, g, ig, code, _stream()), "combine3"),
                 dict(eps=poisoned(eps)), lambda: dict(y=guarded((B, n), dtype=dt)))["y"]
    t, i, u = (e.float() for e in eps)
    assert_close_bf16(r, u + g * (t - i) + ig * (i - u), f"cfg_combine3 n{n} {dt}", rtol=1.6e-2, atol_rms=1.6e-2)


# ---- launch plans --------------------------------------------------------------------------------------------------------
def _plan_conv_in_pix2pix():
    import test_plan_entry_points_gpu as T
    from diffusers_amd import ops
    b = dict(x=T.rnd((2, 4, 9, 11), 1), img=T.rnd((2, 4, 9, 11), 3), w=T.rnd((16, 72), 4, 0.2), bias=T.rnd((16,), 5), table=T.euler_table(),
             step=T.step_counter())
    return b, lambda b: [ops.conv_in_pix2pix(b["x"], b["img"], b["w"], b["bias"], table=b["table"], step_idx=b["step"], rep=3)]


def _plan_cfg_combine3():
    import test_plan_entry_points_gpu as T
    from diffusers_amd import ops
    b = dict(eps=T.rnd((3 * T.SAMPLE[0],) + T.SAMPLE[1:], 2), out=T.blank(T.SAMPLE))
    return b, lambda b: [ops.cfg_combine3(b["eps"], 5.5, 1.7, out=b["out"])]


@pytest.mark.parametrize("name,builder,entry", [("pix2pix_conv_in", _plan_conv_in_pix2pix, "da_conv_in_inpaint"),
                                                ("pix2pix_cfg_combine3", _plan_cfg_combine3, "da_cfg_rescale")])
def test_new_forms_replay_and_relocate_bit_identically(name, builder, entry, tmp_path, monkeypatch):
    """Each form recorded into a launch plan of its own, replayed twice and replayed relocated from the saved file, with the stages of
    tests/test_plan_entry_points_gpu.py; the NULL pointers (mask, ratio_ws) stay NULL through the relocation."""
    import test_plan_entry_points_gpu as T
    monkeypatch.setitem(T.CASES, name, builder)
    names, _ = T.run_case(name, str(tmp_path))
    assert names == (entry,)


# ---- pipelines -----------------------------------------------------------------------------------------------------------
SAMPLERS = ("euler", "ddim", "euler_a", "lcm")
STEPS, HW = 6, 64


def _sampler(name):
    from diffusers_amd import factory
    from diffusers_amd.schedulers import DDIMScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, LCMScheduler
    return {"euler": lambda: EulerDiscreteScheduler(**factory.SDXL_SCHEDULER), "ddim": lambda: DDIMScheduler(**factory.SD15_SCHEDULER),
            "euler_a": lambda: EulerAncestralDiscreteScheduler(**factory.SDXL_SCHEDULER),
            "lcm": lambda: LCMScheduler(**factory.LCM_SCHEDULER)}[name]()


def _build(kind, sampler=None, cosxl=False):
    from diffusers_amd import factory
    build = factory.build_sdxl_pipeline if kind == "sdxl" else factory.build_sd15_pipeline
    pipe = build(device=DEV, tiny=True, seed=0, pix2pix=True)
    if sampler is not None:
        pipe.scheduler = _sampler(sampler)
    if cosxl:
        pipe = type(pipe)(vae=pipe.vae, unet=pipe.unet, scheduler=pipe.scheduler, is_cosxl_edit=True)
    return pipe


def _embeds(kind, B=1):
    g = torch.Generator().manual_seed(3)
    pe, npe = (torch.randn(B, 7, 64, generator=g).to(bf16) for _ in range(2))
    te, nte = (torch.randn(B, 64, generator=g).to(bf16) for _ in range(2)) if kind == "sdxl" else (None, None)
    return pe, npe, te, nte


def _call_kw(kind, gs=7.5, igs=1.5, output_type="latent", steps=STEPS):
    pe, npe, te, nte = _embeds(kind)
    kw = dict(num_inference_steps=steps, guidance_scale=gs, image_guidance_scale=igs, prompt_embeds=pe.to(DEV),
              negative_prompt_embeds=npe.to(DEV), output_type=output_type)
    if kind == "sdxl":
        kw.update(pooled_prompt_embeds=te.to(DEV), negative_pooled_prompt_embeds=nte.to(DEV))
    return kw


def _image(seed=4, hw=HW):
    return torch.rand(1, 3, hw, hw, generator=torch.Generator().manual_seed(seed))


def _gen(seed=21):
    return torch.Generator().manual_seed(seed)


def _hand_loop(pipe, kind, gs, igs, noise_table, seed=21, image=None, steps=STEPS):
    """The reference's loop over the engine's own components, concatenating: cat([latents] * 3), scale_model_input, cat with
    [img, img, 0] on the channels, the ordinary 8-channel conv_in, the combine as torch ops, the scheduler step without CFG."""
    from diffusers_amd import ops
    sch = pipe.scheduler
    do_cfg = gs > 1.0 and igs >= 1.0
    rep = 3 if do_cfg else 1
    pe, npe, te, nte = (t if t is None else t.to(DEV) for t in _embeds(kind))
    sch.set_timesteps(steps, device=DEV)
    lat = ops.mul_scalar(torch.randn(1, 4, HW // 2, HW // 2, generator=_gen(seed), dtype=bf16).to(DEV), float(sch.init_noise_sigma))
    img = pipe.vae.encode_image((_image() if image is None else image).to(DEV).contiguous(), nchw=True, normalize=True).mode()
    if kind == "sdxl":
        ids = torch.tensor([[HW, HW, 0, 0, HW, HW]], dtype=torch.float32)
        cond = pipe._conditioning(pe, npe, te, nte, ids, ids, do_cfg)
    else:
        cond = pipe._conditioning(pe, npe, do_cfg)
    assert cond["batch"] == rep
    kw = {} if noise_table is None else {"noise_table": noise_table}
    sch.reset(0)
    for _ in range(steps):
        xs = sch.scale_model_input(lat, sch.timesteps[0], rep=rep) if sch.scales_model_input else torch.cat([lat] * rep)
        eps = pipe.unet(_concat(xs, img, rep), None, None, conditioning=cond, sampler_table=sch.device_table, step_idx=sch.device_step,
                        return_dict=False)[0]
        if do_cfg:
            t, i, u = eps.chunk(3)
            eps = (u + gs * (t - i) + igs * (i - u)).contiguous()
        sch.step_cfg(eps, lat, gs, out=lat, cfg=False, **kw)
    return lat


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
def test_latents_equal_the_concatenating_loop_and_graph_plan_eager_agree(kind, sampler):
    kw = _call_kw(kind)
    outs, table = {}, None
    for mode in (False, True, "plan"):
        pipe = _build(kind, sampler)
        outs[mode] = pipe(image=_image(), generator=_gen(), use_graph=mode, **kw).images.clone()
        if mode is False:
            table = None if pipe._noise_table is None else pipe._noise_table.clone()
    torch.cuda.synchronize()
    assert (table is not None) == (sampler in ("euler_a", "lcm"))
    want = _hand_loop(_build(kind, sampler), kind, 7.5, 1.5, table)
    assert torch.isfinite(outs[False].float()).all() and tuple(outs[False].shape) == (1, 4, HW // 2, HW // 2)
    assert torch.equal(outs[False], want), "the two-source conv_in + one-launch combine differ from the concatenating loop"
    assert torch.equal(outs[True], outs[False]), "graph replay and eager launches differ"
    assert torch.equal(outs["plan"], outs[False]), "plan replay and eager launches differ"


@pytest.mark.parametrize("kind,sampler", [("sd15", "ddim"), ("sdxl", "euler")])
@pytest.mark.parametrize("gs,igs", [(1.0, 1.5), (7.5, 0.9)])
def test_without_guidance_the_batch_is_not_tripled(kind, sampler, gs, igs):
    pipe = _build(kind, sampler)
    out = pipe(image=_image(), generator=_gen(), **_call_kw(kind, gs, igs)).images.clone()
    want = _hand_loop(_build(kind, sampler), kind, gs, igs, None)
    assert torch.isfinite(out.float()).all() and torch.equal(out, want)


@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
def test_second_call_with_another_image_does_not_recapture_but_another_image_guidance_scale_does(kind):
    kw = _call_kw(kind)
    pipe = _build(kind)
    first = pipe(image=_image(4), generator=_gen(), **kw).images.clone()
    graph = pipe._graph
    second = pipe(image=_image(5), generator=_gen(7), **kw).images.clone()
    assert pipe._graph is graph, "same shapes: the captured step must be replayed, the image latents refreshed in place"
    fresh = _build(kind)(image=_image(5), generator=_gen(7), **kw).images
    assert torch.equal(second, fresh) and not torch.equal(first, second)
    kw2 = _call_kw(kind, igs=1.25)
    third = pipe(image=_image(5), generator=_gen(7), **kw2).images.clone()
    assert pipe._graph is not graph, "image_guidance_scale is an argument of the captured combine"
    assert torch.equal(third, _build(kind)(image=_image(5), generator=_gen(7), **kw2).images) and not torch.equal(third, second)


def test_cosxl_edit_scales_the_image_latents_once():
    kw = _call_kw("sdxl")
    cos = _build("sdxl", cosxl=True)
    out = cos(image=_image(), generator=_gen(), **kw).images.clone()
    plain = _build("sdxl")
    mode = plain.vae.encode_image(_image().to(DEV).contiguous(), nchw=True, normalize=True).mode()
    sf = float(plain.vae.config.scaling_factor)
    assert torch.equal(cos._pix2pix["image_latents"], mode * sf)
    # the plain pipeline handed those latents as `image` runs the same loop; handed the pixels it does not
    assert torch.equal(out, plain(image=mode * sf, generator=_gen(), **kw).images)
    assert not torch.equal(out, _build("sdxl")(image=_image(), generator=_gen(), **kw).images)


@pytest.mark.parametrize("kind", ["sd15", "sdxl"])
def test_step_callback_count(kind):
    from diffusers_amd.pipelines import denoising_end_steps
    n = [0]

    def cb(p, i, t, d):
        assert i == n[0] and tuple(d["latents"].shape) == (1, 4, HW // 2, HW // 2)
        n[0] += 1
        return {}
    pipe = _build(kind)
    pipe(image=_image(), generator=_gen(), callback_on_step_end=cb, **_call_kw(kind))
    assert n[0] == STEPS
    if kind == "sdxl":
        n[0] = 0
        pipe(image=_image(), generator=_gen(), callback_on_step_end=cb, denoising_end=0.5, **_call_kw(kind))
        assert 0 < n[0] == denoising_end_steps(pipe.scheduler, 0.5) < STEPS


# ---- accuracy ------------------------------------------------------------------------------------------------------------
def _psnr01(a, b):
    mse = float((a.float().cpu() - b.float().cpu()).pow(2).mean())
    return 10 * np.log10(1.0 / max(mse, 1e-12))


def _oracle_pix2pix(kind, pipe, img, steps, gs, igs, seed, hw):
    """The reference loop in fp32: encoder, posterior MODE (unscaled), latents = noise * init_noise_sigma, the U-Net on
    [scale(latents) | image latents] for the rows (text, image, uncond) -- the last with a zero image --, the three-way guidance, the
    sampler step, decode."""
    from diffusers_amd import factory, init as dinit
    from diffusers_amd.unet_2d_condition import _DEFAULTS as UD
    tiny = dict(dinit.TINY_SDXL_UNET if kind == "sdxl" else dinit.TINY_SD15_UNET, in_channels=8)
    ucfg = dict(UD)
    ucfg.update(tiny)
    vcfg = dict(pipe.vae.config)
    sf = vcfg["scaling_factor"]
    usd = {k: v.float() for k, v in factory.build_unet(tiny, seed=0, device="cpu")[1].items()}
    _, vsd = factory.build_vae(dinit.TINY_VAE, seed=1, device="cpu", with_encoder=True)
    vsd = {k: v.float() for k, v in vsd.items()}
    pe, npe, te, nte = _embeds(kind)
    zi = encoder_ref(vsd, vcfg, img * 2 - 1)[:, :4]
    sch = EulerOracle(**factory.SDXL_SCHEDULER) if kind == "sdxl" else DDIMOracle(**factory.SD15_SCHEDULER)
    sch.set_timesteps(steps)
    x = torch.randn((1, 4, hw // 2, hw // 2), generator=torch.Generator().manual_seed(seed), dtype=bf16).float() * sch.init_noise_sigma
    if kind == "sdxl":
        ids = torch.tensor([[hw, hw, 0, 0, hw, hw]], dtype=torch.float32)
        added = {"text_embeds": torch.cat([te, nte, nte]).float(), "time_ids": ids.repeat(3, 1)}
    else:
        added = None
    ehs = torch.cat([pe, npe, npe]).float()
    img3 = torch.cat([zi, zi, torch.zeros_like(zi)])
    for t in sch.timesteps:
        xin = sch.scale_model_input(x) if kind == "sdxl" else x
        eps = R.unet_forward(usd, ucfg, torch.cat([torch.cat([xin] * 3), img3], dim=1), float(t), ehs, added)
        et, ei, eu = eps.chunk(3)
        e = eu + gs * (et - ei) + igs * (ei - eu)
        x = sch.step(e, x) if kind == "sdxl" else sch.step(e, int(t), x)
    return (R.vae_decode(vsd, vcfg, x / sf) * 0.5 + 0.5).clamp(0, 1)


@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_tiny_pix2pix_vs_fp32_oracle(kind):
    """Gate: image PSNR >= 30 dB, the gate test_tiny_img2img_vs_fp32_oracle / test_tiny_inpaint_vs_fp32_oracle apply to the same tiny
    models and the same kind of oracle (SDXL: Euler, SD1.5: DDIM; 10 steps, guidance 7.5 / 1.5).  Measured on one MI355X: SDXL
    50.3 dB, SD1.5 49.7 dB.  The test is deterministic: no run-to-run spread."""
    steps, gs, igs = 10, 7.5, 1.5
    img = _image()
    pipe = _build(kind)
    out = pipe(image=img, generator=_gen(), **_call_kw(kind, gs, igs, "pt", steps)).images
    torch.cuda.synchronize()
    ref = _oracle_pix2pix(kind, pipe, img, steps, gs, igs, 21, HW)
    ps = _psnr01(out, ref)
    print(f"tiny {kind} InstructPix2Pix, {steps} steps, guidance {gs} / {igs}: PSNR vs fp32 oracle {ps:.1f} dB")
    assert tuple(out.shape) == (1, 3, HW, HW) and ps >= 30.0


@pytest.mark.skipif(not RR.available(), reason="reference archive oracle/_ref/diffusers_ref.zip did not ship")
@pytest.mark.parametrize("kind", ["sdxl", "sd15"])
def test_tiny_pix2pix_vs_reference_pipeline(kind):
    """The engine's pipelines against the REAL reference StableDiffusion(XL)InstructPix2PixPipeline in fp32 on the same weights,
    image, embeddings and GPU generator (same premise and gate as test_tiny_inpaint_vs_reference_pipeline)."""
    from diffusers_amd import factory, init as dinit
    ref = RR.load_reference()
    ga, gb = torch.Generator(DEV).manual_seed(5), torch.Generator(DEV).manual_seed(5)
    assert torch.equal(torch.randn(4, 999, generator=ga, device=DEV, dtype=bf16),
                       torch.randn(4, 999, generator=gb, device=DEV, dtype=f32).to(bf16)), "premise of this comparison"
    pipe = _build(kind)
    tiny = dict(dinit.TINY_SDXL_UNET if kind == "sdxl" else dinit.TINY_SD15_UNET, in_channels=8)
    _, usd = factory.build_unet(tiny, seed=0, device="cpu")
    _, vsd = factory.build_vae(dinit.TINY_VAE, seed=1, device="cpu", with_encoder=True)
    runet, rvae = RR.build_unet(ref, tiny, usd, DEV, f32), RR.build_vae(ref, dinit.TINY_VAE, vsd, DEV, f32)
    if kind == "sdxl":
        rpipe = ref.StableDiffusionXLInstructPix2PixPipeline(vae=rvae, text_encoder=None, text_encoder_2=None, tokenizer=None,
                                                             tokenizer_2=None, unet=runet,
                                                             scheduler=ref.EulerDiscreteScheduler(**factory.SDXL_SCHEDULER))
    else:
        rpipe = ref.StableDiffusionInstructPix2PixPipeline(vae=rvae, text_encoder=None, tokenizer=None, unet=runet,
                                                           scheduler=ref.DDIMScheduler(**factory.SD15_SCHEDULER), safety_checker=None,
                                                           feature_extractor=None, requires_safety_checker=False)
    rpipe.set_progress_bar_config(disable=True)
    pe, npe, te, nte = _embeds(kind)
    image = _image().to(DEV)
    kw = dict(num_inference_steps=10, guidance_scale=7.5, image_guidance_scale=1.5, output_type="pt")
    if kind == "sdxl":
        kw.update(height=HW, width=HW)

    def run(p, dtype):
        n = [0]

        def cb(pp, i, t, d):
            n[0] += 1
            return {}
        emb = dict(prompt_embeds=pe.to(DEV, dtype), negative_prompt_embeds=npe.to(DEV, dtype))
        if kind == "sdxl":
            emb.update(pooled_prompt_embeds=te.to(DEV, dtype), negative_pooled_prompt_embeds=nte.to(DEV, dtype))
        with torch.no_grad():
            out = p(image=image, generator=torch.Generator(DEV).manual_seed(21), callback_on_step_end=cb, **emb, **kw).images
        return out, n[0]
    want, n_ref = run(rpipe, f32)
    got, n_eng = run(pipe, bf16)
    ps = _psnr01(got, want)
    print(f"tiny {kind} InstructPix2Pix vs the reference pipeline (fp32): {n_eng} steps, PSNR {ps:.1f} dB")
    assert n_eng == n_ref and got.shape == want.shape
    assert ps >= 40.0
