"""The wide-head flash kernel (csrc/attention_wide.hip: D = 256 / 384 / 512, 64 queries per workgroup, 32-key tiles) against fp64, held to
the suite's element-wise attention bound and to 1.5 x the rel-rms of the three-launch path it replaces (fp32 scores GEMM -> row softmax
-> P.V GEMM) on the same inputs; its footprint, determinism, graph replay and refusals; the two call sites against ``force_gemm_path``."""
import functools

import pytest
import torch

import attention_domain as ad
import footprint as FP

pytestmark = pytest.mark.gpu

bf16, f64 = torch.bfloat16, torch.float64
DEV, B = "cuda", 2
QB, KT = 64, 32                                  # queries per workgroup, keys per tile
SQS, SKVS = (1, QB + 2), (8, KT + 13, 5 * KT + 13)
PARITY = [(D, 1, Sq, Skv) for D in (256, 384, 512) for Sq in SQS for Skv in SKVS] + [(256, 2, QB + 2, 5 * KT + 13)]
HOSTILE = [("offset", 300.0), ("offset", -300.0), ("ramp", 8.5), ("ramp", 40.0), ("late_low_to_high", 300.0), ("onehot", 0.0),
           ("vscale", 100.0)]


def _layout(q, k, v):
    """Q | K as column views of one [B * R][2 C] buffer (R = max(Sq, Skv_alloc)), V^T [C][B * Skv_alloc]; keys [Skv, Skv_alloc) of K
    and V^T hold +-bf16 max; the output is a column block of a wider buffer."""
    Bn, Sq, C = q.shape
    Skv = k.shape[1]
    sa = (Skv + 7) // 8 * 8
    R = max(Sq, sa)
    qk = torch.zeros((Bn, R, 2 * C), dtype=bf16, device=DEV)
    qk[:, :Sq, :C] = q.to(DEV)
    qk[:, :sa, C:] = FP.big_finite((Bn, sa, C), 1)
    qk[:, :Skv, C:] = k.to(DEV)
    vt = FP.big_finite((C, Bn, sa), 2)
    vt[:, :, :Skv] = v.to(DEV).permute(2, 0, 1)
    qk, vt = qk.view(Bn * R, 2 * C), vt.view(C, Bn * sa)
    kw = dict(B=Bn, Sq=Sq, Skv=Skv, Skv_alloc=sa, q_row_stride=2 * C, k_row_stride=2 * C, q_batch_stride=R * 2 * C,
              k_batch_stride=R * 2 * C, vt_ld=Bn * sa, vt_batch_stride=sa)
    out = torch.zeros((Bn * Sq, C + 64), dtype=bf16, device=DEV)[:, 32:32 + C]
    return qk, qk[:, C:], vt, kw, out


def _wide(q, k, v, H, scale, **pins):
    from diffusers_amd import ops
    qv, kv, vt, kw, out = _layout(q, k, v)
    return ops.attention(qv, kv, vt, H=H, D=q.shape[2] // H, scale=scale, out=out, **kw, **pins).view(q.shape)


def _three_launch(q, k, v, H, scale):
    """The GEMM route of VaeAttention / the Wan AttentionBlock per (batch, head), keys zero-padded to the GEMM's K granule of 64."""
    from diffusers_amd import ops
    Bn, Sq, C = q.shape
    Skv, D = k.shape[1], C // H
    Sp = (Skv + 63) // 64 * 64
    out = torch.empty((Bn, Sq, C), dtype=bf16, device=DEV)
    for b in range(Bn):
        for h in range(H):
            cols = slice(h * D, (h + 1) * D)
            kp, vtp = torch.zeros((Sp, D), dtype=bf16, device=DEV), torch.zeros((D, Sp), dtype=bf16, device=DEV)
            kp[:Skv], vtp[:, :Skv] = k[b, :, cols].to(DEV), v[b, :, cols].to(DEV).t()
            scores = ops.linear(q[b, :, cols].to(DEV).contiguous(), kp, alpha=scale, out_f32=True)
            probs = torch.zeros((Sq, Sp), dtype=bf16, device=DEV)
            ops.softmax_rows(scores[:, :Skv], out=probs)
            out[b, :, cols] = ops.linear(probs, vtp)
    return out


@functools.lru_cache(maxsize=None)
def _case(kind, level, D, H, Sq, Skv):
    """Inputs, the fp64 reference from the bf16-rounded inputs, and the three-launch path's rel-rms to it (computed once)."""
    scale = ad.default_scale(D)
    q, k, v = ad.family(kind, level, B, H, Sq, Skv, D, scale, seed=D + Sq + Skv)
    ref = ad.attention_ref64(q, k, v, H, scale)
    return q, k, v, scale, ref, ad.rel_rms64(_three_launch(q, k, v, H, scale).cpu(), ref)


@pytest.mark.parametrize("D,H,Sq,Skv", PARITY)
def test_wide_attention_parity(D, H, Sq, Skv):
    q, k, v, scale, ref, gemm_rr = _case("vscale", 0.0, D, H, Sq, Skv)          # (V * 2^0: plain N(0, 1) operands)
    fails = ad.check(_wide(q, k, v, H, scale), ref, gemm_rr, f"wide D{D} H{H} Sq{Sq} Skv{Skv}", ad.TOL_DEFAULT)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind,level", HOSTILE, ids=[ad.family_id(f) for f in HOSTILE])
def test_wide_attention_on_hostile_scores(kind, level):
    Sq, Skv = QB + 2, 5 * KT + 13
    q, k, v, scale, ref, gemm_rr = _case(kind, level, 512, 1, Sq, Skv)
    out = _wide(q, k, v, 1, scale)
    fails = ad.check(out, ref, gemm_rr, f"wide {ad.family_id((kind, level))} D512 Sq{Sq} Skv{Skv}", ad.TOL_DEFAULT)
    if kind == "onehot":
        fails += ad.check_onehot(out, v, Sq, "wide onehot")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("D", [256, 384, 512])
def test_wide_attention_footprint(D):
    """Poisoned operands, +-bf16 max in keys [Skv, Skv_alloc), guarded output (rows D + 4 apart: the 8-byte store path)."""
    from diffusers_amd import ops
    Sq, Skv, sa = QB + 2, KT + 13, KT + 16
    g = torch.Generator("cpu").manual_seed(D)
    q, k, v = (torch.randn((B, s, D), generator=g).to(bf16).to(DEV) for s in (Sq, Skv, Skv))
    kp, vt = FP.big_finite((B, sa, D), 3), FP.big_finite((D, B, sa), 4)
    kp[:, :Skv], vt[:, :, :Skv] = k, v.permute(2, 0, 1)
    ins = [FP.poisoned(q.view(B * Sq, D), ld=D + 8), FP.poisoned(kp.view(B * sa, D), ld=D + 8), FP.poisoned(vt.view(D, B * sa), ld=B * sa + 8)]
    outs = []
    for src in (ins, [i.clean() for i in ins]):
        o = FP.guarded((B * Sq, D), ld=D + 4)
        ops.attention(*(i.view for i in src), B=B, H=1, D=D, Sq=Sq, Skv=Skv, Skv_alloc=sa, q_row_stride=D + 8, k_row_stride=D + 8,
                      q_batch_stride=Sq * (D + 8), k_batch_stride=sa * (D + 8), vt_ld=B * sa + 8, vt_batch_stride=sa, out=o.view)
        torch.cuda.synchronize()
        for t in (o, *src):
            t.check(f"wide attention D{D}")
        outs.append(o.view.clone())
    assert bool(torch.isfinite(outs[0].float()).all()) and FP.bits_equal(outs[0], outs[1])
    fails = ad.check(outs[0], ad.attention_ref64(q.cpu(), k.cpu(), v.cpu(), 1, ad.default_scale(D)), None, f"footprint D{D}", ad.TOL_DEFAULT)
    assert not fails, "\n".join(fails)


def test_wide_attention_is_deterministic_and_replays_from_a_hip_graph():
    q, k, v, scale, _, _ = _case("vscale", 0.0, 512, 1, QB + 2, 5 * KT + 13)
    from diffusers_amd import ops
    qv, kv, vt, kw, out = _layout(q, k, v)
    run = lambda: ops.attention(qv, kv, vt, H=1, D=512, scale=scale, out=out, **kw)                    # noqa: E731
    eager = run().clone()
    assert FP.bits_equal(run(), eager)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
        s.synchronize()
        with torch.cuda.graph(g, stream=s):
            run()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert FP.bits_equal(out, eager), "graph replay differs from the eager launch"


@pytest.mark.parametrize("pin", [dict(causal=True), dict(bias=True), dict(algo=1), dict(q_block=128)], ids=lambda p: next(iter(p)))
def test_wide_attention_refuses_masks_and_pinned_variants(pin):
    q, k, v, scale, _, _ = _case("vscale", 0.0, 256, 1, QB + 2, KT + 13)
    if "bias" in pin:
        pin = dict(bias=torch.zeros((1, 1, QB + 2, 64), dtype=bf16, device=DEV))
    with pytest.raises(RuntimeError, match="DA_ERR_UNSUPPORTED"):
        _wide(q, k, v, 1, scale, **pin)


def _routes(block, x, ref):
    """The block's default route and its GEMM route against the fp64 evaluation `ref` of the block."""
    flash = block(x).float().cpu()
    block.force_gemm_path = True
    gemm = block(x).float().cpu()
    rr, floor = ad.rel_rms64(flash, gemm), ad.rel_rms64(gemm, ref.reshape(gemm.shape))
    print(f"[parity] routes: flash vs gemm rel_rms={rr:.3e}; gemm vs fp64 rel_rms={floor:.3e}")
    assert bool(torch.isfinite(flash).all()) and rr <= ad.FLOOR_FACTOR * floor


@pytest.mark.parametrize("side", [8, 5])
def test_vae_attention_routes_agree(side, monkeypatch):
    from diffusers_amd import autoencoder_kl, factory, init as dinit
    monkeypatch.setattr(autoencoder_kl, "wide_flash_pays", lambda B, S: True)     # (the default sends so few tokens to the GEMMs)
    vae, sd = factory.build_vae(dict(dinit.TINY_VAE, block_out_channels=(64, 256)), seed=5, device=DEV)
    x = (torch.randn((2, side, side, 256), generator=torch.Generator("cpu").manual_seed(side)) * 1.5).to(bf16)
    w = {n: sd["decoder.mid_block.attentions.0." + n].to(bf16).to(f64) for n in
         ("group_norm.weight", "group_norm.bias", "to_q.weight", "to_q.bias", "to_k.weight", "to_k.bias", "to_v.weight", "to_v.bias",
          "to_out.0.weight", "to_out.0.bias")}
    xs = x.to(f64).view(2, side * side, 256)
    h = torch.nn.functional.group_norm(xs.transpose(1, 2), 32, w["group_norm.weight"], w["group_norm.bias"], 1e-6).transpose(1, 2)
    qh, kh, vh = (h @ w[f"to_{n}.weight"].t() + w[f"to_{n}.bias"] for n in "qkv")
    att = torch.softmax(qh @ kh.transpose(1, 2) * 256 ** -0.5, -1) @ vh
    _routes(vae.mid_attn, x.to(DEV), att @ w["to_out.0.weight"].t() + w["to_out.0.bias"] + xs)


def test_wan_attention_block_routes_agree_in_one_launch():
    from diffusers_amd import plan as P
    from diffusers_amd.autoencoder_kl_wan import AttentionBlock
    from diffusers_amd.layers import Weights
    c, T, side = 256, 3, 8
    g = torch.Generator("cpu").manual_seed(7)
    sd = {"a.norm.gamma": 1 + 0.1 * torch.randn((c, 1, 1), generator=g), "a.to_qkv.weight": torch.randn((3 * c, c, 1, 1), generator=g) * c ** -0.5,
          "a.to_qkv.bias": 0.1 * torch.randn(3 * c, generator=g), "a.proj.weight": torch.randn((c, c, 1, 1), generator=g) * c ** -0.5,
          "a.proj.bias": 0.1 * torch.randn(c, generator=g)}
    sd = {n: t.to(bf16) for n, t in sd.items()}
    block = AttentionBlock(Weights(sd, DEV), "a")
    x = torch.randn((T, side, side, c), generator=g).to(bf16)
    xs = x.to(f64).view(T, side * side, c)
    h = torch.nn.functional.normalize(xs, dim=-1) * c ** 0.5 * sd["a.norm.gamma"].to(f64).view(c)
    qh, kh, vh = (h @ sd["a.to_qkv.weight"].to(f64).view(3 * c, c).t() + sd["a.to_qkv.bias"].to(f64)).chunk(3, -1)
    att = torch.softmax(qh @ kh.transpose(1, 2) * c ** -0.5, -1) @ vh
    _routes(block, x.to(DEV), att @ sd["a.proj.weight"].to(f64).view(c, c).t() + sd["a.proj.bias"].to(f64) + xs)
    block.force_gemm_path = False
    with P.recording(strict=False) as rec:
        block(x.to(DEV))
    assert rec.names.count("da_attention_bf16") == 1
