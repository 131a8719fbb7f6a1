"""FP8 flash attention, csrc/attention_fp8.hip: the prepare kernel to the bit against the header's arithmetic restated in torch, the
attention kernel against float64 softmax attention on the dequantised operands under a bound derived from the numeric contract.

The bound (``_check``), per output element, with w_ij the exact softmax weights and ref the float64 result.  The kernel computes
o = sum_j p8_ij v_jd / sum_j p8_ij with p8_ij = e4m3(p_ij), p_ij = 2^8 w_ij / max_j w_ij (or larger: an earlier running maximum).
  1. p in e4m3's normal range: p8 = p (1 + d), |d| <= 2^-4 (3 mantissa bits, half an ulp).  o - ref = sum_j w_ij d_j (v_jd - ref) /
     (1 + sum_j w_ij d_j), so |o - ref| <= 2^-4 / (1 - 2^-4) sum_j w_ij |v_jd - ref_id|.
  2. p below 2^-6 (subnormal or flushed): |p8 - p| <= 2^-10, i.e. 2^-18 in units of w / max w, against a denominator of
     sum_j w_ij / max_j w_ij: 2^-18 sum_j |v_jd - ref_id| / (sum_j w_ij / max_j w_ij).
  3. one rounding to bf16: 2^-8 |ref|.
  4. fp32: the products q8 k8 are exact, the MFMA's 128-term sum is off by at most 127 x 2^-24 A_ij (A the same sum over |q8 k8|,
     scaled like x), the three scale multiplies and the subtraction of m by 4 x 2^-24 |x_ij|, exp2 by 2^-22 relative: a relative error
     e_i = ln 2 x 2^-24 max_j (127 A_ij + 4 |x_ij|) + 2^-22 on every weight, twice that after normalisation, in the shape of term 1;
     the P V sum, the rescales by exp2(m_old - m_new) (one per key tile) and the epilogue: (Skv + tiles + 8) 2^-24 sum_j w_ij |v_jd|."""
import ctypes as C
import math

import pytest
import torch

import footprint as FP

pytestmark = pytest.mark.gpu

bf16, f8, f32, f64, u8 = torch.bfloat16, torch.float8_e4m3fn, torch.float32, torch.float64, torch.uint8
DEV = "cuda"
SHAPES_BH = [(1, 1), (2, 3)]


def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def _inputs(B, H, S, seed):
    g = _gen(seed)
    return torch.randn((B * S, 256 * H), generator=g).to(bf16), (torch.randn((128 * H, B * S), generator=g) * 2).to(bf16)


def _quant(x):
    """The header's arithmetic over the last dim, one fp32 operation per step: (e4m3 bytes, scale)."""
    amax = x.abs().amax(dim=-1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    return (x * (1.0 / scale)[..., None]).clamp(-448.0, 448.0).to(f8).view(u8), scale


def prepare_ref(qk, vt, B, S, H):
    Cc, S8 = 128 * H, (S + 127) // 128 * 128
    q, s = _quant(qk.float().reshape(B * S, 2 * H, 128))
    v, sv = _quant(vt.float().reshape(Cc, B, S))
    vt8 = torch.zeros((Cc, B, S8), dtype=u8)
    vt8[:, :, :S] = v
    return (q[:, :H].reshape(B * S, Cc), q[:, H:].reshape(B * S, Cc), vt8.reshape(Cc, B * S8), s[:, :H].contiguous(), s[:, H:].contiguous(),
            sv.t().contiguous())


@pytest.mark.parametrize("B,H", SHAPES_BH)
@pytest.mark.parametrize("S", [1, 127, 128, 129, 300])
def test_prepare_to_the_bit(S, B, H):
    from diffusers_amd import ops
    Cc, S8 = 128 * H, (S + 127) // 128 * 128
    qk, vt = _inputs(B, H, S, 100 * S + H)
    qk[0, :128] = 0                                               # a zero row: scale 1, bytes 0
    qk[0, Cc:Cc + 128] = torch.where(torch.arange(128) % 2 == 0, 448.0, -448.0).to(bf16)
    if B * S > 1:
        qk[-1, 5] = FP.BF16_MAX                                   # a row whose amax is the largest finite bf16
    vt[0], vt[1] = 0, vt[1] * 448
    src_qk, src_vt = FP.poisoned(qk, ld=2 * Cc + 8), FP.poisoned(vt, ld=B * S + 3)       # V^T rows at odd addresses
    outs = [FP.guarded(s, dtype=d) for s, d in (((B * S, Cc), u8), ((B * S, Cc), u8), ((Cc, B * S8), u8), ((B * S, H), f32),
                                                ((B * S, H), f32), ((B, Cc), f32))]
    for o in outs:
        o.bits.view(-1)[o.lead:o.lead + o.span] = o.sentinel     # the outputs start as the sentinel too: every byte must be written
    ops.attention_fp8_prepare(src_qk.view, src_vt.view, B=B, S=S, H=H, out=tuple(o.view.view(f8) if o.dtype == u8 else o.view for o in outs))
    for o, ref, name in zip(outs, prepare_ref(qk, vt, B, S, H), ("q8", "k8", "vt8", "sq", "sk", "sv")):
        assert FP.bits_equal(o.view.cpu(), ref), (name, int((o.view.cpu() != ref).sum()))
        o.check(name)
    assert int(outs[2].view.reshape(Cc, B, S8)[:, :, S:].count_nonzero()) == 0, "bytes [S, S8) of every batch segment are zero"
    src_qk.check("qk"), src_vt.check("vt")


def _operands(B, H, S, seed):
    from diffusers_amd import ops
    qk, vt = _inputs(B, H, S, seed)
    return list(ops.attention_fp8_prepare(qk.to(DEV), vt.to(DEV), B=B, S=S, H=H))


def _run(opnd, B, H, S, Sq, Skv, scale):
    """q8 / k8 as views of ONE poisoned [B*S][2C] buffer (the model's layout), the prefixes Sq / Skv of every batch; guarded output."""
    from diffusers_amd import ops
    q8, k8, vt8, sq, sk, sv = opnd
    Cc = 128 * H
    both = FP.poisoned(torch.cat((q8.view(u8), k8.view(u8)), dim=1), ld=2 * Cc + 16)
    x = both.view.view(f8).unflatten(0, (B, S))
    out = FP.guarded((B * Sq, Cc), ld=Cc + 8)
    out.view.fill_(float("nan"))
    ops.attention_fp8(x[:, :Sq, :Cc], x[:, :Skv, Cc:], vt8, sq.unflatten(0, (B, S))[:, :Sq], sk.unflatten(0, (B, S))[:, :Skv], sv,
                      B=B, H=H, Sq=Sq, Skv=Skv, scale=scale, out=out.view)
    out.check("out"), both.check("q8 | k8")
    return out.view.clone()


def _check(out, opnd, B, H, S, Sq, Skv, scale, what):
    q8, k8, vt8, sq, sk, sv = opnd
    S8, LOG2E = vt8.shape[1] // B, 1.4426950408889634
    q = q8.float().to(f64).reshape(B, S, H, 128)[:, :Sq] * sq.to(f64).reshape(B, S, H, 1)[:, :Sq]
    k = k8.float().to(f64).reshape(B, S, H, 128)[:, :Skv] * sk.to(f64).reshape(B, S, H, 1)[:, :Skv]
    v = (vt8.float().to(f64).reshape(H, 128, B, S8)[..., :Skv] * sv.to(f64).t().reshape(H, 128, B, 1)).permute(2, 0, 3, 1)     # [B][H][Skv][128]
    got = out.to(f64).reshape(B, Sq, H, 128)
    worst = 0.0
    for b in range(B):
        for h in range(H):
            qq, kk, vv = q[b, :, h], k[b, :, h], v[b, h]
            s = scale * (qq @ kk.t())
            w = torch.softmax(s, dim=-1)
            ref = w @ vv
            dev_all = (vv[None] - ref[:, None]).abs()                                    # [Sq][Skv][128]
            dev = (w[..., None] * dev_all).sum(1)
            mass = (w / w.amax(dim=-1, keepdim=True)).sum(-1, keepdim=True)
            e = math.log(2) * 2.0 ** -24 * (127 * LOG2E * scale * (qq.abs() @ kk.abs().t()) + 4 * LOG2E * s.abs()).amax(-1, keepdim=True) \
                + 2.0 ** -22
            tol = (2.0 ** -4 / (1 - 2.0 ** -4) + 2 * e) * dev + 2.0 ** -18 * dev_all.sum(1) / mass + 2.0 ** -8 * ref.abs() \
                + (Skv + (Skv + 127) // 128 + 8) * 2.0 ** -24 * (w @ vv.abs())
            worst = max(worst, float(((got[b, :, h] - ref).abs() / tol).max()))
    print(f"[attention_fp8] {what}: max err / bound = {worst:.3f}")
    assert bool(torch.isfinite(out).all()) and worst <= 1.0, (what, worst)


@pytest.mark.parametrize("B,H", SHAPES_BH)
@pytest.mark.parametrize("Skv", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("Sq", [1, 127, 128, 129, 257])
def test_attention_against_float64(Sq, Skv, B, H):
    S, scale = max(Sq, Skv), 128 ** -0.5
    opnd = _operands(B, H, S, 1000 * Sq + Skv + H)
    _check(_run(opnd, B, H, S, Sq, Skv, scale), opnd, B, H, S, Sq, Skv, scale, f"Sq {Sq} Skv {Skv} B {B} H {H}")


def test_hostile_rows_and_bit_identities():
    """Rows 0-7 / 8-15: every score shifted by +3000 / -3000 (a key-constant product in channels 64 .. 127) over a spread of a few
    units from channels 0 .. 63; row 16: one one-hot key; row 17: a flat row over the 300 keys.  Then: a second call gives the same
    bits, and content in the k8 rows past Skv changes nothing.  The offset is spread over 64 channels on purpose: carried by ONE
    product (q8 = k8 = 448 in one channel, sq 64 times larger) the same rows miss the bound -- measured max err / bound 3.1, the
    contract restated in torch 0.42 -- because the 8-bit MFMA's sum of 128 products is then not the fp32 sum of term 4."""
    B, H, S, scale = 1, 2, 300, 128 ** -0.5
    opnd = _operands(B, H, S, 7)
    q8, k8, vt8, sq, sk, sv = opnd
    qv, kv = q8.view(u8).view(S, H, 128), k8.view(u8).view(S, H, 128)
    kv[:, :, 64:], kv[:, :, 1], kv[77, :, 1] = 0x7E, 0, 0x7E                              # 448 | 0 except key 77 | (0x7E = 448)
    sk.fill_(2.0 ** -8)
    qv[:18] = (torch.randn((18, H, 128), generator=_gen(9)) * 4).to(f8).view(u8).to(DEV)
    qv[:18, :, 1] = 0
    qv[:8, :, 64:], qv[8:16, :, 64:] = 0x7E, 0xFE                                         # +-448: +-3000 = 64 scale sq sk 448^2
    sq[:16] = 3000.0 / (scale * 2.0 ** -8 * 64 * 448 * 448)
    qv[16:18], qv[16, :, 1], sq[16:18] = 0, 0x7E, 1.0                                     # scores: 69.3 at key 77, 0 elsewhere | all 0
    out = _run(opnd, B, H, S, S, S, scale)
    _check(out, opnd, B, H, S, S, S, scale, "hostile rows")
    one_hot = (vt8.float()[:, 77] * sv[0]).to(f64)
    assert bool(((out[16].to(f64) - one_hot).abs() <= 2.0 ** -7 * one_hot.abs()).all()), "one-hot row: sv * v8 of key 77 within a bf16 step"
    assert FP.bits_equal(out, _run(opnd, B, H, S, S, S, scale)), "a second call gives the same bits"
    short = _run(opnd, B, H, S, 257, 129, scale)
    kv[129:] = 0x7E
    assert FP.bits_equal(short, _run(opnd, B, H, S, 257, 129, scale)), "k8 rows past Skv are not part of the result"


def test_refusals_by_name(monkeypatch):
    from diffusers_amd import _lib as L, ops
    q8, k8, vt8, sq, sk, sv = _operands(1, 1, 128, 1)
    kw = dict(B=1, H=1, Sq=128, Skv=128, scale=1.0)
    zeros = lambda *s, dt=bf16: torch.zeros(s, dtype=dt, device=DEV)  # noqa: E731
    attn = lambda q, k: ops.attention_fp8(q, k, vt8, sq, sk, sv, **kw)  # noqa: E731
    prep = lambda w: ops.attention_fp8_prepare(zeros(8, 2 * w), zeros(w, 8), B=1, S=8, H=1)  # noqa: E731
    for exc, match, call in ((ValueError, "attention_fp8: head size 64 .* only D = 128", lambda: attn(q8[:, :64], k8[:, :64])),
                             (ValueError, "attention_fp8_prepare: head size 64 .* only D = 128", lambda: prep(64)),
                             (ValueError, "q8 needs row and batch strides", lambda: attn(zeros(128, 144, dt=f8)[:, 8:136], k8)),   # base + 8
                             (ValueError, "k8 needs row and batch strides", lambda: attn(q8, zeros(128, 136, dt=f8)[:, :128]))):  # ld 136
        with pytest.raises(exc, match=match):
            call()
    p = L.AttentionFp8Params()
    p.q8 = p.k8 = p.vt8 = p.sq = p.sk = p.sv = p.out = q8.data_ptr()
    p.B, p.H, p.Sq, p.Skv, p.S8, p.D = 1, 1, 128, 128, 128, 64
    assert L.load().da_attention_fp8(C.byref(p), None) == 3                               # DA_ERR_UNSUPPORTED: D = 64, no launch
    assert L.load().da_attention_fp8(C.byref(L.AttentionFp8Params()), None) == 1          # DA_ERR_INVALID: NULL operands
    monkeypatch.setattr(L._tls, "recorder", object(), raising=False)
    for match, call in (("attention_fp8: not replayable by a launch plan", lambda: attn(q8, k8)),
                        ("attention_fp8_prepare: not replayable by a launch plan", lambda: prep(128))):
        with pytest.raises(RuntimeError, match=match):
            call()
