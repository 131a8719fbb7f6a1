"""CPU leg of the value-domain tests: the conditions tests/test_value_domain_gpu.py asserts on the kernels are conditions the
formulas and a plain fp32 implementation can meet.  The activation bound is checked on a numpy fp32 restatement of
csrc/common.cuh over every finite bf16 input; the normalisation tolerances on the torch fp32 stand-ins of tests/ops_emulation.py
over the same hostile input families and shapes the GPU tests use."""
import numpy as np
import pytest
import torch

import ops_emulation as E
import value_domain as vd

bf16 = torch.bfloat16


def test_the_domain_and_the_rounding():
    v = vd.all_finite_bf16()
    assert v.numel() == vd.N_FINITE_BF16 == 255 * 256 and bool(torch.isfinite(v.float()).all())
    f = v.float().numpy()
    assert np.unique(f.view(np.uint32)).size == v.numel() and float(np.abs(f).max()) == vd.BF16_MAX
    assert np.array_equal(vd.round_bf16(f.astype(np.float64)), f.astype(np.float64)), "bf16 values must round to themselves"
    # against torch's fp32 -> bf16 cast (one rounding from fp32) on fp32 values of every magnitude, ties included
    g = torch.Generator().manual_seed(1)
    x = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-140, 127, (200000,), generator=g).float())
    x = torch.cat([x, v.float() * (1 + 2.0 ** -8), torch.tensor([3.3961775e38, 3.4e38, -3.4e38, 1e-45, -0.0])])
    want = x.to(bf16).double().numpy()
    got = vd.round_bf16(x.double().numpy())
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    # the double rounding a cast through fp32 commits: 1 + 2^-8 + 2^-30 lies above the tie, fp32 rounds it onto the tie
    assert vd.round_bf16(1 + 2.0 ** -8 + 2.0 ** -30) == 1 + 2.0 ** -7


@pytest.mark.parametrize("act", vd.ACTS)
def test_activation_formulas_meet_the_bound_over_the_whole_domain(act):
    """common.cuh's four activations in exact fp32 arithmetic, all 65 280 finite bf16 inputs: finite, and within
    2^-8 |ref| + 5e-7 of fp64 -- as computed (fp32) and as stored (bf16)."""
    v = vd.to_f64(vd.all_finite_bf16())
    out = vd.act_model_f32(act, v).astype(np.float64)
    vd.check_activation(out, v, act, f"fp32 model of {act}")
    vd.check_activation(vd.round_bf16(out), v, act, f"fp32 model of {act}, stored as bf16")


def test_constant_families_sum_exactly_in_fp32():
    """The constants of the `constant` family: fp32 running sums of c and c^2 over the largest normalised unit of the tests are exact,
    so mean = c and E[x^2] - mean^2 = 0 in any summation order, and x - mean = 0."""
    n = max(B_HW * (C // G) for (_, B_HW, C, G) in vd.GN_SHAPES + vd.GN_SHAPES_MULTI)
    n = max(n, max(C for _, C in vd.LN_SHAPES))
    for c in vd.CONSTANTS:
        x = np.full(n, c, dtype=np.float32)
        assert float(torch.tensor(c).to(bf16)) == c
        s1, s2 = np.cumsum(x, dtype=np.float32), np.cumsum(x * x, dtype=np.float32)
        k = np.arange(1, n + 1, dtype=np.float64)
        assert np.array_equal(s1.astype(np.float64), c * k) and np.array_equal(s2.astype(np.float64), c * c * k)
        mean = np.float32(s1[-1]) / np.float32(n)
        assert float(mean) == c and float(np.float32(s2[-1]) / np.float32(n) - mean * mean) == 0.0


def _gn_cases():
    for shp in vd.GN_SHAPES:
        yield shp + (0,)
    B, HW, C1, C2, G = vd.GN_TWO_SOURCE
    yield (B, HW, C1 + C2, G, C2)


@pytest.mark.parametrize("B,HW,C,G,C2", list(_gn_cases()))
def test_groupnorm_stand_in_meets_the_tolerance_on_every_family(B, HW, C, G, C2):
    gamma, beta = vd.affine(C)
    for i, (kind, level) in enumerate(vd.GN_FAMILIES):
        x = vd.family_groups(kind, level, B, HW, C, G, seed=i)
        x1, x2 = (x[..., :C - C2].contiguous(), x[..., C - C2:].contiguous()) if C2 else (x, None)
        for silu in (False, True):
            y = E.group_norm_nhwc(x1, gamma, beta, G, 1e-5, silu=silu, x2=x2)
            ref = vd.group_norm_ref64(x, gamma, beta, G, 1e-5, silu=silu)
            vd.assert_close64(y, ref, f"stand-in groupnorm {B}x{HW}x{C}/{G} {kind} {level:g} silu={silu}", **vd.TOL_GROUPNORM)
        if kind == "constant":                     # the expected output of a constant slab is beta (then SiLU)
            assert torch.equal(vd.group_norm_ref64(x, gamma, beta, G, 1e-5), beta.double().expand(B, HW, C))


def test_several_workgroup_shapes_reach_that_form():
    """Which of the GPU test's `several_workgroups` shapes the plan deals to more than one workgroup per slab."""
    parts = [vd.gn_multi_parts(*s) for s in vd.GN_SHAPES_MULTI]
    assert parts == [1, 4, 4], parts
    B, HW, C1, C2, G = vd.GN_TWO_SOURCE_MULTI
    assert vd.gn_multi_parts(B, HW, C1 + C2, G) == 4


def test_groupnorm_constant_slab_of_1024_is_outside_the_fp32_apply_form():
    """Why GN_FAMILIES leaves c = 1024 out: fp32 x * a + (beta - mean * a) returns beta to within half an ulp of mean * a = 3.2e5
    (1.6e-2) there; the same slab through (x - mean) * a + beta, LayerNorm's form, is exact."""
    B, HW, C, G = vd.GN_SHAPES[0]
    gamma, beta = vd.affine(C)
    x = vd.family_groups("constant", 1024.0, B, HW, C, G)
    err = (E.group_norm_nhwc(x, gamma, beta, G, 1e-5).double() - vd.group_norm_ref64(x, gamma, beta, G, 1e-5)).abs().max()
    print(f"[value-domain] fp32 GroupNorm on a constant slab of 1024: max |y - beta| = {float(err):.3e}")
    assert 1e-3 < float(err) <= 1024.0 * 1e-5 ** -0.5 * 1.25 * 2.0 ** -24 * 1.01     # |mean| * rstd * max gamma * half an fp32 ulp


@pytest.mark.parametrize("M,C", vd.LN_SHAPES)
def test_layernorm_stand_in_meets_the_tolerance_on_every_family(M, C):
    gamma, beta = vd.affine(C)
    rpb = (M + 1) // 2
    for i, (kind, level) in enumerate(vd.FAMILIES):
        x = vd.family_rows(kind, level, M, C, seed=i)
        what = f"stand-in layernorm {M}x{C} {kind} {level:g}"
        vd.assert_close64(E.layer_norm(x, gamma, beta, 1e-5), vd.layer_norm_ref64(x, gamma, beta, 1e-5), what, **vd.TOL_LAYERNORM)
        for dt in (torch.float32, bf16):
            sc, sh = (vd._randn((2, C), 50) * 0.3).to(dt), (vd._randn((2, C), 51) * 0.3).to(dt)
            y = E.layer_norm(x, None, None, 1e-6, mod_scale=sc, mod_shift=sh, rows_per_batch=rpb)
            ref = vd.layer_norm_ref64(x, None, None, 1e-6, mod_scale=sc, mod_shift=sh, rows_per_batch=rpb)
            vd.assert_close64(y, ref, f"{what} adaLN {dt}", **vd.TOL_ADALN)


def test_rms_stand_ins_meet_the_tolerance_on_every_family():
    for i, (kind, level) in enumerate(vd.RMS_FAMILIES):
        for C in vd.RMS_NORM_WIDTHS:
            x, gamma = vd.family_rows(kind, level, 5, C, seed=i), vd.affine(C)[0]
            vd.assert_close64(E.rms_norm(x, gamma, 1e-6), vd.rms_norm_ref64(x, gamma, 1e-6), f"stand-in rms_norm 5x{C} {kind} {level:g}",
                              **vd.TOL_LAYERNORM)
        for C in vd.RMS_CHANNELS_WIDTHS:
            x, gamma = vd.family_rows(kind, level, 37, C, seed=i), vd.affine(C)[0]
            for silu in (False, True):
                vd.assert_close64(E.rmsnorm_channels(x, gamma, real_channels=C, silu=silu), vd.rmsnorm_channels_ref64(x, gamma, C, silu),
                                  f"stand-in rmsnorm_channels 37x{C} {kind} {level:g} silu={silu}", **vd.TOL_GROUPNORM)
        for D, heads in vd.RMS_ROPE_SHAPES:
            C = D * heads
            x = vd.family_rows(kind, level, 9, C, seed=i)
            wh, wa = vd.affine(D)[0], vd.affine(C)[0]
            y = E.rmsnorm_rope_(x.clone(), heads=heads, head_dim=D, col_offsets=(0,), weights=(wh,), eps=1e-6)
            vd.assert_close64(y, vd.rms_norm_ref64(x, wh, 1e-6, unit=D), f"stand-in rmsnorm per head D{D}x{heads} {kind} {level:g}", **vd.TOL_RMS_ROPE)
            y = E.rmsnorm_rope_(x.clone(), heads=heads, head_dim=D, col_offsets=(0,), weights=(wa,), eps=1e-6, norm="across_heads")
            vd.assert_close64(y, vd.rms_norm_ref64(x, wa, 1e-6), f"stand-in rmsnorm across heads D{D}x{heads} {kind} {level:g}", **vd.TOL_RMS_ROPE)


@pytest.mark.parametrize("M,C,N", vd.FOLD_SHAPES)
def test_layernorm_fold_stand_in_meets_the_tolerance_on_every_family(M, C, N):
    """The fold's algebra with fp32 one-pass statistics (the stand-in of ops.linear(stats_out=) / (ln=)) against fp64
    LN(x) @ W^T + b, and next to the unfolded fp32 path."""
    from diffusers_amd import ops
    gamma, beta, w, b = vd.fold_problem(C, N)
    wl, fold = ops.fold_layernorm(w, gamma, beta, vd.LN_EPS)
    a, wprod = torch.zeros((M, 64), dtype=bf16), vd._randn((C, 64), 9).to(bf16)
    bounded = vd.fold_families(M, C)
    measured = {f"offset {lv:g}": vd.family_rows("offset", lv, M, C, seed=int(lv)) for lv in vd.FOLD_EXTREME_LEVELS}
    for name, rows in list(bounded.items()) + list(measured.items()):
        st = ops.RowStats(M, "cpu")
        x = E.linear(a, wprod, residual=rows, stats_out=st)
        assert torch.equal(x, rows)                                   # a = 0: the producer's output IS the family
        ref = vd.fold_ref64(x, gamma, beta, w, b)
        y = E.linear(x, wl, b, ln=(st, fold))
        plain = E.linear(E.layer_norm(x, gamma, beta, vd.LN_EPS), w, b)
        e_fold, e_plain = vd.rel_rms64(y, ref), vd.rel_rms64(plain, ref)
        print(f"[value-domain] stand-in fold {M}x{C}x{N} {name}: e_fold {e_fold:.3e} e_plain {e_plain:.3e}")
        if name in bounded:                                           # (the extreme levels are measured, not bounded, here)
            vd.assert_close64(y, ref, f"stand-in fold {M}x{C}x{N} {name}", **vd.TOL_FOLD)


@pytest.mark.parametrize("N", vd.SOFTMAX_NS)
def test_softmax_stand_in_meets_the_conditions_on_every_family(N):
    for name in vd.SOFTMAX_FAMILIES:
        s = vd.softmax_family(name, N)
        p = E.softmax_rows(s)
        vd.check_softmax(p, s, f"stand-in softmax {name} N{N}")
        if name == "all_equal":
            assert torch.equal(p, torch.full_like(p, 1.0 / N)), "all-equal rows must give exactly bf16(1 / N)"
