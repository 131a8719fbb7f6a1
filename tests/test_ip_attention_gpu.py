"""The IP-Adapter image-prompt kernel (csrc/attention_ip.hip, ops.ip_attention_accumulate, torch.ops.mi355x.ip_attn):
out += sum_a scale_a softmax(q K_a^T) V_a in place, against fp64 from the same bf16 `out`.

Bound.  The suite's element-wise attention bound (attention_domain.TOL_DEFAULT, the gate of test_temporal_attention_gpu.py) holds for
each adapter's attention output o_a; the kernel adds scale_a o_a, so the added term may be off by sum_a |scale_a| (tol rms(o_a) +
tol |o_a|), and the one final rounding adds half a bf16 step of the sum.  Everything comes from the fp64 reference.

Every call through _run has q as a column block of a wider buffer, `out` / k / v with row strides > their width, k | v stacked in one
buffer, NaN in the padding tokens [N, N_alloc) and in guard bands around every buffer."""
import ctypes as C

import pytest
import torch

import attention_domain as ad
import footprint as FP

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEV = "cuda"


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed))


def _inputs(B, H, D, Sq, Ns, seed):
    Cc = H * D
    return (_randn((B, Sq, Cc), seed).to(bf16), _randn((B, Sq, Cc), seed + 1).to(bf16),
            [(_randn((B, N, Cc), seed + 2 + 2 * a).to(bf16), _randn((B, N, Cc), seed + 3 + 2 * a).to(bf16)) for a, N in enumerate(Ns)])


def _run(out0, q, kvs, scales, H, sm_scale, clean=False):
    """One launch on footprint.Guarded buffers (`clean`: zeros around them in place of NaN), every guard band checked afterwards."""
    from diffusers_amd import ops
    B, Sq, Cc = q.shape
    pick = lambda g: g.clean() if clean else g  # noqa: E731
    wide = _randn((B * Sq, Cc + 16), 1).to(bf16)
    wide[:, 8:8 + Cc] = q.reshape(B * Sq, Cc)
    qg, og = pick(FP.poisoned(wide, ld=Cc + 24)), FP.guarded((B * Sq, Cc), ld=Cc + 8).set(out0.reshape(B * Sq, Cc))
    bufs, adapters = [qg, og], []
    for (k, v), s in zip(kvs, scales):
        N, na = k.shape[1], k.shape[1] + 3
        kv = torch.full((B, na, 2 * Cc), float("nan"), dtype=bf16)
        kv[:, :N, :Cc], kv[:, :N, Cc:] = k, v
        bufs.append(pick(FP.poisoned(kv.view(B * na, 2 * Cc), ld=2 * Cc + 8)))
        adapters.append((bufs[-1].view[:, :Cc], bufs[-1].view[:, Cc:], N, na, s))
    ops.ip_attention_accumulate(og.view, qg.view[:, 8:8 + Cc], adapters, B=B, H=H, D=Cc // H, Sq=Sq, scale=sm_scale)
    torch.cuda.synchronize()
    for g in bufs:
        g.check("ip attention")
    return og.view.cpu().view(B, Sq, Cc)


def _check(got, out0, q, kvs, scales, H, sm_scale, what):
    tol, f64 = ad.TOL_DEFAULT, torch.float64
    ref, slack = out0.to(f64), torch.zeros(out0.shape, dtype=f64)
    for (k, v), s in zip(kvs, scales):
        o = ad.attention_ref64(q, k, v, H, sm_scale)
        ref = ref + s * o
        slack += abs(s) * (tol * float(o.pow(2).mean().sqrt()) + tol * o.abs())
    err = (got.to(f64) - ref).abs()
    bad = int((~(err <= slack + 0.5 * ad.bf16_step(ref))).sum())
    print(f"[parity] {what}: max_abs={float(err.nan_to_num(float('inf')).max()):.3e} violations={bad}/{err.numel()}")
    assert bad == 0, f"{what}: {bad} elements outside the bound"


CASES = [(D, [N], [0.6], Sq, B, H) for D in (64, 96, 160) for N in (1, 4, 5, 16, 31, 32) for Sq in (1, 31, 32, 33, 129) for B, H in ((1, 1), (2, 3))]
CASES += [(D, [5, 32, 1, 16][:A], [0.7, -0.5, 1.0, 0.25][:A], 129, 2, 3) for D in (64, 96, 160) for A in (2, 4)]


@pytest.mark.parametrize("D,Ns,scales,Sq,B,H", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_against_fp64(D, Ns, scales, Sq, B, H):
    out0, q, kvs = _inputs(B, H, D, Sq, Ns, seed=D + sum(Ns) + Sq + B)
    sm = ad.default_scale(D)
    _check(_run(out0, q, kvs, scales, H, sm), out0, q, kvs, scales, H, sm, f"ip D{D} N{Ns} Sq{Sq} B{B} H{H}")


def test_bit_identities():
    B, H, D, Sq = 2, 3, 96, 33
    sm = ad.default_scale(D)
    out0, q, kvs = _inputs(B, H, D, Sq, [5, 1], seed=3)
    nan_q = torch.full_like(q, float("nan"))
    assert FP.bits_equal(_run(out0, nan_q, kvs, [0.0, 0.0], H, sm), out0), "all scales 0: out keeps its bits (nothing launched)"
    assert FP.bits_equal(_run(out0, q, kvs, [0.7, 0.0], H, sm), _run(out0, q, kvs[:1], [0.7], H, sm))
    assert FP.bits_equal(_run(out0, q, kvs, [0.0, -1.5], H, sm), _run(out0, q, kvs[1:], [-1.5], H, sm))
    # one key: P = l = 1, the result is out + scale v with ONE rounding (scale v is exact in fp32 for a three-bit scale)
    want = (out0.float() + -1.5 * kvs[1][1].float()).to(bf16)
    assert FP.bits_equal(_run(out0, q, kvs[1:], [-1.5], H, sm), want)


@pytest.mark.parametrize("kind,level", [("offset", 3000.0), ("offset", -3000.0), ("onehot", 0.0)])
def test_hostile_scores(kind, level):
    B, H, D, Sq, N = 1, 2, 64, 33, 32
    sm = ad.default_scale(D)
    q, k, v = ad.family(kind, level, B, H, Sq, N, D, sm, seed=7)
    out0 = torch.zeros_like(q)
    got = _run(out0, q, [(k, v)], [1.0], H, sm)
    _check(got, out0, q, [(k, v)], [1.0], H, sm, f"ip {ad.family_id((kind, level))}")
    assert kind != "onehot" or not ad.check_onehot(got, v, Sq, "ip onehot")


@pytest.mark.parametrize("D", [64, 96, 160])
def test_footprint(D):
    """NaN against zeros in every byte around q, k and v (the guard bands themselves are checked in every _run): the same bits, twice."""
    out0, q, kvs = _inputs(2, 3, D, 129, [5, 17], seed=D)
    runs = [_run(out0, q, kvs, [0.5, 0.5], 3, ad.default_scale(D), clean=c) for c in (False, True, False)]
    assert bool(torch.isfinite(runs[0].float()).all()) and FP.bits_equal(runs[0], runs[1]) and FP.bits_equal(runs[0], runs[2])


@pytest.mark.parametrize("bad,status", [(dict(n=0), 3), (dict(n=33), 3), (dict(D=40), 3), (dict(A=5), 3), (dict(out=8), 3), (dict(v=None), 1)],
                         ids=lambda b: str(b))
def test_refusals_never_launch(bad, status):
    """Refused by return value (3 = DA_ERR_UNSUPPORTED, 1 = DA_ERR_INVALID) before any launch: `out` stays zero although every V is one."""
    from diffusers_amd import _lib as L
    B, H, D, Sq, N = 1, 2, 64, 40, 4
    out = torch.zeros((B * Sq + 1, H * D), dtype=bf16, device=DEV)
    q, kv = torch.zeros((B * Sq, H * D), dtype=bf16, device=DEV), torch.ones((B * 40, H * 160), dtype=bf16, device=DEV)
    p = L.AttentionIPParams()
    p.q, p.out, p.A, p.B, p.H, p.D, p.Sq, p.sm_scale = q.data_ptr(), out.data_ptr(), 1, B, H, D, Sq, D ** -0.5
    p.q_row_stride = p.o_row_stride = H * D
    for a in range(L.IP_MAX_ADAPTERS):
        p.k[a] = p.v[a] = kv.data_ptr()
        p.n[a], p.n_alloc[a], p.k_row_stride[a], p.v_row_stride[a], p.scale[a] = N, 40, H * 160, H * 160, 1.0
    for key, val in bad.items():
        if key in ("n", "v"):
            getattr(p, key)[0] = val
        else:
            setattr(p, key, p.out + val if key == "out" else val)
    assert L.load().da_attention_ip_bf16(C.byref(p), None) == status
    torch.cuda.synchronize()
    assert not bool(out.any())


def test_torch_op_at_batch_two_and_under_graph_replay():
    from diffusers_amd import torch_ops  # noqa: F401
    B, H, D, Sq, Ns, scales = 2, 3, 64, 33, [4, 16], [0.6, -0.25]
    sm = ad.default_scale(D)
    out0, q, kvs = _inputs(B, H, D, Sq, Ns, seed=11)
    dev = [[t.to(DEV) for t in kv] for kv in kvs]
    args = ([k for k, _ in dev], [v for _, v in dev], Ns, scales, H, None)
    o0, qd = out0.to(DEV), q.to(DEV)
    eager = o0.clone()
    assert torch.ops.mi355x.ip_attn(eager, qd, *args) is None and torch.ops.mi355x.ip_attn.default._schema.is_mutable
    _check(eager.cpu(), out0, q, kvs, scales, H, sm, "torch op B2")
    o = torch.empty_like(o0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o.copy_(o0)
        torch.ops.mi355x.ip_attn(o, qd, *args)
    for i in range(3):
        o.fill_(float(i))
        g.replay()
        torch.cuda.synchronize()
        assert FP.bits_equal(o, eager), f"replay {i}"


# ---- one cross-attention layer with two adapters against IPAdapterAttnProcessor2_0, restated ----------------------------------------
def _restated(x, ehs, imgs, scales, sd, dtype, heads):
    """IPAdapterAttnProcessor2_0 in `dtype`: text attention + scale * image attention of every adapter, to_out, the residual"""
    w = {k: t.to(dtype) for k, t in sd.items()}
    x, ehs = x.to(dtype), ehs.to(dtype)
    B, S, Cc = x.shape
    split = lambda t: t.view(B, -1, heads, Cc // heads).transpose(1, 2)  # noqa: E731
    attend = lambda q, k, v: (torch.softmax(q @ k.transpose(2, 3) * (Cc // heads) ** -0.5, -1) @ v)  # noqa: E731
    q = split(x @ w["a.to_q.weight"].t())
    o = attend(q, split(ehs @ w["a.to_k.weight"].t()), split(ehs @ w["a.to_v.weight"].t()))
    for a, (img, s) in enumerate(zip(imgs, scales)):
        img = img.to(dtype)
        o = o + s * attend(q, split(img @ w[f"ip{a}.k"].t()), split(img @ w[f"ip{a}.v"].t()))
    return o.transpose(1, 2).reshape(B, S, Cc) @ w["a.to_out.0.weight"].t() + w["a.to_out.0.bias"] + x


def test_cross_attention_layer_with_two_adapters_against_the_restated_reference():
    """C = 320, 8 heads of 40 (the 64-wide kernel head), 77 text tokens, image prompts of 4 and 16 tokens, B = 2, 8 x 8 queries.
    Gate: rel-rms to fp64 <= 1.5 x that of the same restatement run in bf16."""
    from diffusers_amd import init as dinit
    from diffusers_amd.layers import Attention, Weights, pad_encoder_states
    B, S, Cc, heads, cross, Ns, scales = 2, 64, 320, 8, 768, [4, 16], [0.6, -0.8]
    shapes = {"a.to_q.weight": (Cc, Cc), "a.to_k.weight": (Cc, cross), "a.to_v.weight": (Cc, cross), "a.to_out.0.weight": (Cc, Cc),
              "a.to_out.0.bias": (Cc,), **{f"ip{a}.{c}": (Cc, cross) for a in range(2) for c in "kv"}}
    sd = dinit.random_state_dict(shapes, seed=13)
    x, ehs = _randn((B, S, Cc), 1).to(bf16), _randn((B, 77, cross), 2).to(bf16)
    imgs = [_randn((B, N, cross), 3 + a).to(bf16) for a, N in enumerate(Ns)]
    attn = Attention(Weights({k: v for k, v in sd.items() if k.startswith("a.")}, DEV), "a", heads, cross=True)
    xd = x.to(DEV).view(B * S, Cc)
    kv = attn.precompute_kv(*pad_encoder_states(ehs.to(DEV))[:1], B, *pad_encoder_states(ehs.to(DEV))[1:])
    attn.attach_ip([(sd[f"ip{a}.k"], sd[f"ip{a}.v"]) for a in range(2)])
    kv.ip = attn.precompute_ip_kv([pad_encoder_states(i.to(DEV)) for i in imgs], B)
    attn.ip_scales = tuple(scales)
    got = attn(xd, B, S, residual=xd, kv=kv).cpu().view(B, S, Cc)
    ref = _restated(x, ehs, imgs, scales, sd, torch.float64, heads)
    err, floor = ad.rel_rms64(got, ref), ad.rel_rms64(_restated(x, ehs, imgs, scales, sd, bf16, heads), ref)
    print(f"[ip layer] engine {err:.3e}, bf16 restatement (floor) {floor:.3e}")
    assert err <= 1.5 * floor, (err, floor)
