"""Wan and FLUX with fp8 attention (enable_fp8_attention): transformers with heads of 128 built from the tiny configs, against the
reference forward restated in float64 with the same quantise -> dequantise of q, k, v and exact softmax, and the pipeline identities.
The floor of the 1.5 x rule is the contract's own error: the restatement in bf16 with P rounded to e4m3 against the row's true maximum,
the row sum taken from the rounded P and the output rounded once -- computed in torch, never by the kernel."""
import sys
from pathlib import Path

import pytest
import torch

import attention_domain as ad
import footprint as FP

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oracle import reference_math as R  # noqa: E402

pytestmark = pytest.mark.gpu

bf16, f8, f64 = torch.bfloat16, torch.float8_e4m3fn, torch.float64
DEV = "cuda"


def _cfg(kind):
    from diffusers_amd import init as dinit
    if kind == "wan":
        return dict(dinit.TINY_WAN, attention_head_dim=128, num_attention_heads=2, num_layers=2)
    return dict(dinit.TINY_FLUX, attention_head_dim=128, num_attention_heads=2, axes_dims_rope=(16, 56, 56), num_layers=1,
                num_single_layers=1)


def _fake_quant(t, dim):
    """csrc/attention_fp8.hip's prepare arithmetic over ``dim``, dequantised in float64."""
    x = t.float()
    amax = x.abs().amax(dim=dim, keepdim=True)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    return (x * (1.0 / scale)).clamp(-448.0, 448.0).to(f8).to(f64) * scale.to(f64)


def _sdpa_fp8(round_p):
    plain = R._sdpa

    def sdpa(q, k, v):                                            # (B, H, S, D)
        if q.shape[-2] != k.shape[-2]:                            # Wan's cross-attention over the text keys stays as it is
            return plain(q, k, v)
        x = (_fake_quant(q, -1) @ _fake_quant(k, -1).transpose(-1, -2)) * q.shape[-1] ** -0.5
        vd = _fake_quant(v, -2)                                   # one scale per (batch, channel), over the keys
        if not round_p:
            return (torch.softmax(x, dim=-1) @ vd).to(q.dtype)
        p = torch.exp2((x - x.amax(dim=-1, keepdim=True)) * 1.4426950408889634 + 8).float().to(f8).to(f64)
        return ((p @ vd) / p.sum(dim=-1, keepdim=True)).to(q.dtype)
    return sdpa


def _restated(kind, sd, cfg, inputs, dt, round_p, monkeypatch):
    monkeypatch.setattr(R, "_sdpa", _sdpa_fp8(round_p))
    try:
        args = [t.to(dt) if i < 4 else t for i, t in enumerate(inputs)]        # (FLUX: the id grids stay fp32)
        return (R.wan_forward if kind == "wan" else R.flux_forward)({k: v.to(dt) for k, v in sd.items()}, cfg, *args)
    finally:
        monkeypatch.undo()


@pytest.mark.parametrize("kind", ["wan", "flux"])
def test_transformer_against_float64_restatement(kind, monkeypatch):
    from diffusers_amd import factory
    from diffusers_amd.pipelines import FluxPipeline
    cfg, g = _cfg(kind), torch.Generator().manual_seed(3)
    if kind == "wan":
        tr, sd = factory.build_wan_transformer(cfg, seed=9, device=DEV)
        x, pe, t = torch.randn((1, 16, 3, 8, 8), generator=g).to(bf16), torch.randn((1, 16, 64), generator=g).to(bf16), torch.tensor([500.0])
        inputs = (x, t, pe)
        run = lambda: tr(x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=pe.to(DEV), return_dict=False)[0].cpu()  # noqa: E731
    else:
        tr, sd = factory.build_flux_transformer(cfg, seed=5, device=DEV)
        x, pe, pp = (torch.randn(s, generator=g).to(bf16) for s in ((1, 64, 64), (1, 16, 64), (1, 64)))
        t = torch.tensor([0.5])
        inputs = (x, pe, pp, t, FluxPipeline._prepare_latent_image_ids(8, 8), torch.zeros(16, 3))
        run = lambda: tr(x.to(DEV), encoder_hidden_states=pe.to(DEV), pooled_projections=pp.to(DEV), timestep=t.to(DEV),  # noqa: E731
                         img_ids=inputs[4], txt_ids=inputs[5], return_dict=False)[0].cpu()
    tr.enable_fp8_attention()
    got = run()
    ref = _restated(kind, sd, cfg, inputs, f64, False, monkeypatch)
    err, floor = ad.rel_rms64(got, ref), ad.rel_rms64(_restated(kind, sd, cfg, inputs, bf16, True, monkeypatch), ref)
    print(f"[{kind} fp8 attention] engine {err:.3e}, bf16 restatement with e4m3 P (floor) {floor:.3e}")
    assert got.shape == ref.shape and err <= ad.FLOOR_FACTOR * floor, (err, floor)


def _pipe(kind):
    from diffusers_amd import FlowMatchEulerDiscreteScheduler, factory
    from diffusers_amd.pipelines import FluxPipeline, WanPipeline
    if kind == "wan":
        return WanPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=3.0, use_dynamic_shifting=False),
                           transformer=factory.build_wan_transformer(_cfg(kind), seed=9, device=DEV)[0])
    return FluxPipeline(scheduler=FlowMatchEulerDiscreteScheduler(shift=1.0, use_dynamic_shifting=False), vae=None,
                        transformer=factory.build_flux_transformer(_cfg(kind), seed=5, device=DEV)[0])


def _run(pipe, kind, seed=0, use_graph=True):
    g = torch.Generator().manual_seed(3)
    pe, ne, pp = (torch.randn(s, generator=g).to(bf16) for s in ((1, 16, 64), (1, 16, 64), (1, 64)))
    kw = dict(prompt_embeds=pe, num_inference_steps=2, output_type="latent", generator=torch.Generator().manual_seed(seed), use_graph=use_graph)
    if kind == "wan":
        return pipe(negative_prompt_embeds=ne, height=64, width=64, num_frames=9, guidance_scale=5.0, **kw).images.clone()
    return pipe(pooled_prompt_embeds=pp, height=128, width=128, **kw).images.clone()


@pytest.mark.parametrize("kind", ["wan", "flux"])
def test_pipeline_identities(kind):
    from diffusers_amd import factory
    pipe, never = _pipe(kind), _pipe(kind)
    off = _run(pipe, kind)
    g_off = pipe._graph
    pipe.enable_fp8_attention()
    on = _run(pipe, kind)
    g_on = pipe._graph
    assert g_on is not g_off and not FP.bits_equal(on, off), "enabling captures a new step that computes something else"
    assert FP.bits_equal(on, _run(pipe, kind, use_graph=False)), "captured graph == eager"
    second = _run(pipe, kind, seed=1)
    assert pipe._graph is g_on and FP.bits_equal(second, _run(pipe, kind, seed=1, use_graph=False)), "a second seed replays"
    with pytest.raises(NotImplementedError, match='use_graph="plan" with fp8 attention enabled: da_attention_fp8'):
        _run(pipe, kind, use_graph="plan")
    if kind == "flux":
        pipe.enable_fp8_linears()
        both = _run(pipe, kind)
        assert bool(torch.isfinite(both).all()) and not FP.bits_equal(both, on), "fp8 attention together with fp8 linears"
        pipe.disable_fp8_linears()
    pipe.disable_fp8_attention()
    back = _run(pipe, kind)
    assert pipe._graph is not g_on, "disabling captures again"
    assert FP.bits_equal(back, off) and FP.bits_equal(back, _run(never, kind)), "disable restores the bf16 path to the bit"
    tiny = (factory.build_wan_pipeline if kind == "wan" else factory.build_flux_pipeline)(device=DEV, tiny=True)      # heads of 64
    with pytest.raises(ValueError, match="enable_fp8_attention: .* heads of 128, this model has attention_head_dim = 64"):
        tiny.enable_fp8_attention()
