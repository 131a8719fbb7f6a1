"""The Resampler attention kernel (csrc/attention_resampler.hip, ops.resampler_attention): at most 16 queries over keys / values from
two token-major sources, against fp64 on the explicitly concatenated keys and values under the suite's element-wise attention bound
(attention_domain.TOL_DEFAULT).

Every call through _run has q as a column block of a wider buffer, `out` with a row stride > its width, k | v of each source stacked
in one buffer (the kernel's operands are its column halves), NaN in the padding rows [S, S_alloc) of every batch and in guard bands
around every buffer."""
import ctypes as C

import pytest
import torch

import attention_domain as ad
import footprint as FP

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEV = "cuda"
D = 64
SCALE = ad.default_scale(D)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)).to(bf16)


def _inputs(B, H, Nq, S0, S1, seed):
    Cc = H * D
    return (_randn((B, Nq, Cc), seed), _randn((B, S0, Cc), seed + 1), _randn((B, S0, Cc), seed + 2),
            _randn((B, S1, Cc), seed + 3), _randn((B, S1, Cc), seed + 4))


def _run(q, k0, v0, k1, v1, H, clean=False):
    """One launch on footprint.Guarded buffers (`clean`: zeros around them in place of NaN), every guard band checked afterwards."""
    from diffusers_amd import ops
    B, Nq, Cc = q.shape
    pick = lambda g: g.clean() if clean else g  # noqa: E731
    wide = _randn((B * Nq, Cc + 16), 1)
    wide[:, 8:8 + Cc] = q.reshape(B * Nq, Cc)
    qg, og = pick(FP.poisoned(wide, ld=Cc + 24)), FP.guarded((B * Nq, Cc), ld=Cc + 8)
    bufs, halves = [qg, og], []
    for k, v in ((k0, v0), (k1, v1)):
        S, sa = k.shape[1], k.shape[1] + 3
        if S == 0:
            halves += [None, None, 0, 0]
            continue
        kv = torch.full((B, sa, 2 * Cc), float("nan"), dtype=bf16)
        kv[:, :S, :Cc], kv[:, :S, Cc:] = k, v
        bufs.append(pick(FP.poisoned(kv.view(B * sa, 2 * Cc), ld=2 * Cc + 8)))
        halves += [bufs[-1].view[:, :Cc], bufs[-1].view[:, Cc:], S, sa]
    ops.resampler_attention(qg.view[:, 8:8 + Cc], halves[0], halves[1], halves[4], halves[5], B=B, H=H, Nq=Nq, S0=halves[2],
                            S0_alloc=halves[3], S1=halves[6], S1_alloc=halves[7], scale=SCALE, out=og.view)
    torch.cuda.synchronize()
    for g in bufs:
        g.check("resampler attention")
    return og.view.cpu().view(B, Nq, Cc)


def _ref(q, k0, v0, k1, v1, H):
    return ad.attention_ref64(q, torch.cat([k0, k1], 1), torch.cat([v0, v1], 1), H, SCALE)


@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("with_s1", [False, True], ids=["S1=0", "S1=Nq"])
@pytest.mark.parametrize("S0", [1, 31, 32, 33, 127, 128, 129, 257])
@pytest.mark.parametrize("Nq", [1, 8, 15, 16])
def test_against_fp64(Nq, S0, with_s1, B, H):
    t = _inputs(B, H, Nq, S0, Nq if with_s1 else 0, seed=Nq + S0 + B)
    assert not ad.check(_run(*t, H), _ref(*t, H), None, f"resampler Nq{Nq} S0{S0} S1{t[3].shape[1]} B{B} H{H}", ad.TOL_DEFAULT)


def test_identities():
    B, H, Nq = 2, 3, 15
    q, k0, v0, k1, v1 = _inputs(B, H, Nq, 1, 0, seed=5)
    assert FP.bits_equal(_run(q, k0, v0, k1, v1, H), v0.expand(B, Nq, H * D).contiguous()), "one valid key: that V row to the bit"
    # the latent keys as source 1, or as the tail of source 0: another block cut and nothing else -- both under the same bound
    q, k0, v0, k1, v1 = t = _inputs(B, H, Nq, 33, Nq, seed=6)
    ref, none = _ref(*t, H), k1[:, :0]
    assert not ad.check(_run(*t, H), ref, None, "two sources", ad.TOL_DEFAULT)
    assert not ad.check(_run(q, torch.cat([k0, k1], 1), torch.cat([v0, v1], 1), none, none, H), ref, None, "one source", ad.TOL_DEFAULT)


@pytest.mark.parametrize("kind,level,shift", [("offset", 3000.0, 0), ("offset", -3000.0, 0), ("onehot", 0.0, 32), ("onehot", 0.0, 48)],
                         ids=["offset+3000", "offset-3000", "onehot-src0-last-block", "onehot-src1"])
def test_hostile_scores(kind, level, shift):
    """S0 = 48 (a full block and a partial one of 16 keys), S1 = 16.  `onehot`: query i selects key i of the family; the keys are
    rolled by `shift`, so the selected ones are exactly source 0's partial last block (32) or source 1 (48)."""
    B, H, Nq, S0, S1 = 1, 2, 16, 48, 16
    q, k, v = ad.family(kind, level, B, H, Nq, S0 + S1, D, SCALE, seed=7)
    kr, vr = k.roll(shift, 1), v.roll(shift, 1)
    t = (q, kr[:, :S0], vr[:, :S0], kr[:, S0:], vr[:, S0:])
    got = _run(*t, H)
    assert not ad.check(got, _ref(*t, H), None, f"resampler {kind}{level:+g} shift {shift}", ad.TOL_DEFAULT)
    assert kind != "onehot" or not ad.check_onehot(got, v, Nq, "resampler onehot")


def test_footprint():
    """NaN against zeros in every byte around q, k and v (the guard bands themselves are checked in every _run): the same bits, twice."""
    t = _inputs(2, 3, 15, 129, 15, seed=8)
    runs = [_run(*t, 3, clean=c) for c in (False, True, False)]
    assert bool(torch.isfinite(runs[0].float()).all()) and FP.bits_equal(runs[0], runs[1]) and FP.bits_equal(runs[0], runs[2])


@pytest.mark.parametrize("bad,status", [(dict(D=40), 3), (dict(Nq=17), 3), (dict(S1=17), 3), (dict(S0=0), 3), (dict(k0_row_stride=2 * 64 + 4), 3),
                                        (dict(v0=None), 1)], ids=lambda b: str(b))
def test_refusals_never_launch(bad, status):
    """Refused by return value (3 = DA_ERR_UNSUPPORTED, 1 = DA_ERR_INVALID) before any launch: `out` stays zero although every V is one."""
    from diffusers_amd import _lib as L
    B, H, Nq, S0, S1 = 1, 2, 16, 40, 16
    out = torch.zeros((B * 32, H * D), dtype=bf16, device=DEV)
    q, kv = torch.zeros((B * 32, H * D), dtype=bf16, device=DEV), torch.ones((B * 64, 2 * H * D), dtype=bf16, device=DEV)
    p = L.AttentionResamplerParams()
    p.q, p.out, p.k0, p.v0, p.k1, p.v1 = q.data_ptr(), out.data_ptr(), kv.data_ptr(), kv.data_ptr(), kv.data_ptr(), kv.data_ptr()
    p.B, p.H, p.D, p.Nq, p.S0, p.S0_alloc, p.S1, p.S1_alloc, p.scale = B, H, D, Nq, S0, 64, S1, 64, SCALE
    p.q_row_stride = p.o_row_stride = H * D
    p.k0_row_stride = p.v0_row_stride = p.k1_row_stride = p.v1_row_stride = 2 * H * D
    for key, val in bad.items():
        setattr(p, key, val)
    assert L.load().da_attention_resampler_bf16(C.byref(p), None) == status
    torch.cuda.synchronize()
    assert not bool(out.any())
