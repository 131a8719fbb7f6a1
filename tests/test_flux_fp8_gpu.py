"""FLUX with fp8 linears (enable_fp8_linears): the tiny transformer (2 heads of 64: every quantised width is a multiple of 128) against
the reference forward restated in float64 with the same quantise -> dequantise on the same operands, and the pipeline identities."""
import sys
from pathlib import Path

import pytest
import torch

import attention_domain as ad
import footprint as FP

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oracle import reference_math as R  # noqa: E402

pytestmark = pytest.mark.gpu

bf16, f64 = torch.bfloat16, torch.float64
DEV = "cuda"
BLOCK_LINEARS = ("attn.to_q", "attn.to_k", "attn.to_v", "attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj", "attn.to_out.0",
                 "attn.to_add_out", "ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj", "ff_context.net.2", "proj_mlp", "proj_out")


def _fake_quant(t):
    """csrc/gemm_fp8.hip's row arithmetic, then back to t's dtype: amax / 448 scales, e4m3 round to nearest even."""
    x = t.float()
    amax = x.abs().amax(dim=-1, keepdim=True)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    q = (x * (1.0 / scale)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return (q.to(f64) * scale.to(f64)).to(t.dtype)


def _restated(sd, cfg, inputs, dt, monkeypatch):
    """oracle flux_forward in `dt` with every block linear reading fake-quantised activations and weights."""
    w = {k: v.to(dt) for k, v in sd.items()}
    quantised = {id(v) for k, v in w.items() if k.startswith(("transformer_blocks.", "single_transformer_blocks."))
                 and k.endswith(".weight") and k.rsplit(".", 1)[0].split(".", 2)[2] in BLOCK_LINEARS}
    plain = torch.nn.functional.linear

    def linear(x, weight, bias=None):
        if id(weight) in quantised:
            x, weight = _fake_quant(x), _fake_quant(weight)
        return plain(x, weight, bias)
    monkeypatch.setattr(R.F, "linear", linear)
    try:
        return R.flux_forward(w, cfg, *(t.to(dt) if t.is_floating_point() and i < 4 else t for i, t in enumerate(inputs)))
    finally:
        monkeypatch.undo()


def test_transformer_against_float64_restatement(monkeypatch):
    from diffusers_amd import factory, init as dinit
    cfg = dinit.TINY_FLUX
    tr, sd = factory.build_flux_transformer(cfg, seed=5, device=DEV)
    g = torch.Generator().manual_seed(3)
    x, pe, pp = (torch.randn(s, generator=g).to(bf16) for s in ((1, 64, 64), (1, 16, 64), (1, 64)))
    t = torch.tensor([0.5])
    ids = torch.zeros(8, 8, 3)
    ids[..., 1] += torch.arange(8)[:, None]
    ids[..., 2] += torch.arange(8)[None, :]
    img_ids, txt_ids = ids.reshape(-1, 3), torch.zeros(16, 3)
    tr.enable_fp8_linears()
    got = tr(x.to(DEV), encoder_hidden_states=pe.to(DEV), pooled_projections=pp.to(DEV), timestep=t.to(DEV), img_ids=img_ids,
             txt_ids=txt_ids, return_dict=False)[0].cpu()
    inputs = (x, pe, pp, t, img_ids, txt_ids)
    ref = _restated(sd, cfg, inputs, f64, monkeypatch)
    err, floor = ad.rel_rms64(got, ref), ad.rel_rms64(_restated(sd, cfg, inputs, bf16, monkeypatch), ref)
    print(f"[flux fp8] engine {err:.3e}, bf16 restatement (floor) {floor:.3e}")
    assert got.shape == ref.shape and err <= ad.FLOOR_FACTOR * floor, (err, floor)


def _embeds():
    g = torch.Generator().manual_seed(3)
    return torch.randn(1, 16, 64, generator=g).to(bf16), torch.randn(1, 64, generator=g).to(bf16)


def _run(pipe, seed=0, use_graph=True):
    pe, pp = _embeds()
    return pipe(prompt_embeds=pe, pooled_prompt_embeds=pp, height=64, width=64, num_inference_steps=2, output_type="latent",
                generator=torch.Generator().manual_seed(seed), use_graph=use_graph).images.clone()


def test_pipeline_identities():
    from diffusers_amd import factory
    pipe, never = (factory.build_flux_pipeline(device=DEV, tiny=True, seed=5) for _ in range(2))
    off = _run(pipe)
    g_off = pipe._graph
    pipe.enable_fp8_linears()
    on = _run(pipe)
    g_on = pipe._graph
    assert g_on is not g_off and not FP.bits_equal(on, off), "enabling captures a new step that computes something else"
    assert FP.bits_equal(on, _run(pipe, use_graph=False)), "captured graph == eager"
    second = _run(pipe, seed=1)
    assert pipe._graph is g_on and FP.bits_equal(second, _run(pipe, seed=1, use_graph=False)), "a second seed replays"
    with pytest.raises(NotImplementedError, match='use_graph="plan" with fp8 linears enabled'):
        _run(pipe, use_graph="plan")
    pipe.disable_fp8_linears()
    back = _run(pipe)
    assert pipe._graph is not g_on, "disabling captures again"
    assert FP.bits_equal(back, off) and FP.bits_equal(back, _run(never)), "disable restores the bf16 path to the bit"


def test_width_not_a_multiple_of_128_is_refused_by_name():
    from diffusers_amd import factory, init as dinit
    cfg = dict(dinit.TINY_FLUX, num_attention_heads=1)          # inner width 64
    tr, _ = factory.build_flux_transformer(cfg, seed=5, device=DEV)
    with pytest.raises(ValueError, match=r"transformer_blocks\.0\.attn\.to_q\|to_k has an input width of 64"):
        tr.enable_fp8_linears()
