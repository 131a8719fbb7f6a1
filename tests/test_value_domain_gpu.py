"""The HIP kernels over the bf16 VALUE domain (tests/value_domain.py), not only N(0, 1) data:
  * every finite bf16 input through every activation site -- the epilogues of the three GEMM families, linear_small_m, the GroupNorm
    apply passes, rmsnorm_channels -- against fp64, to one bf16 step + 5e-7 (what csrc/common.cuh states for its approximations);
  * the normalisation kernels on rows / groups with a large common offset, no spread, one dominating element, a scale far from 1,
    against fp64 references with the tolerances tests/test_kernels_gpu.py uses for the same ops; the LayerNorm fold up to
    mean / sigma = 64 with its own bound, and next to the unfolded path at 128 and 256;
  * softmax_rows on all-equal, one-hot, offset, masked and tied rows.
tests/test_value_domain_cpu.py shows on the CPU that each condition is one a plain fp32 implementation meets."""
import numpy as np
import pytest
import torch

import value_domain as vd

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEV = "cuda"


def _ops():
    from diffusers_amd import _lib as L
    from diffusers_amd import ops
    return ops, L


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the exhaustive activation sweep
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def domain():
    """All 65 280 finite bf16 values: as a bf16 vector, as fp64, and routed for the GEMMs -- x [65280][64] with the value in column 0
    and 1.0 in column 1 (the GEGLU value half reads that one), zeros elsewhere."""
    v = vd.all_finite_bf16()
    x = torch.zeros((v.numel(), 64), dtype=bf16)
    x[:, 0], x[:, 1] = v, 1.0
    return {"v": v, "v64": vd.to_f64(v), "x": x.to(DEV)}


PLAIN_N = (132, 64, 80, 128, 160, 256, 320)     # 132 = an edge tile where the tile allows one, then the smallest N it admits
GEGLU_N2 = (128, 256, 640)                      # packed [value | gate] columns: whole 64-column groups, 640 for the 320-wide tiles
GEMM_ACTS = {"silu": ("silu", "ACT_SILU"), "gelu_tanh": ("gelu_tanh", "ACT_GELU_TANH"), "gelu_erf": ("gelu_erf", "ACT_GELU_ERF"),
             "quick_gelu": ("quick_gelu", "ACT_QUICK_GELU"), "geglu": ("gelu_erf", "ACT_GEGLU"), "geglu_tanh": ("gelu_tanh", "ACT_GEGLU_TANH")}


def _route_weight(ops, n: int, geglu: bool) -> torch.Tensor:
    if not geglu:                                    # every output column = x[:, 0]
        w = torch.zeros((n, 64), dtype=bf16, device=DEV)
        w[:, 0] = 1.0
        return w
    w = torch.zeros((n, 64), dtype=bf16, device=DEV)  # [value rows ; gate rows]: value = x[:, 1] = 1.0, gate = x[:, 0]
    w[: n // 2, 1] = 1.0
    w[n // 2:, 0] = 1.0
    return ops.pack_geglu(w, None)[0]


def _tile_family(L, tile: int) -> str:
    return "first" if tile < L.FIRST_K2_TILE else ("k3" if tile >= L.TILE_K3_256x256 else "k2")


@pytest.mark.parametrize("act", list(GEMM_ACTS))
def test_gemm_epilogue_activation_over_all_finite_bf16(domain, act):
    """x[m] = (v_m, 1, 0, ...), W = e_0 rows, no bias: the fp32 accumulator of row m is exactly v_m, so every output column of row m is
    act(v_m) -- for every pinned tile of the three kernel families (one admissible staging each)."""
    ops, L = _ops()
    name, act_const = GEMM_ACTS[act]
    A, geglu = getattr(L, act_const), act.startswith("geglu")
    x, first, first_tile, ran = domain["x"], None, None, {}
    weights = {}
    for tile in range(1, len(L.TILE_NAMES)):
        y = None
        for n in (GEGLU_N2 if geglu else PLAIN_N):
            for st in (L.STAGE_LDS_DIRECT, L.STAGE_PINGPONG, L.STAGE_REGISTER):
                if n not in weights:
                    weights[n] = _route_weight(ops, n, geglu)
                try:
                    y = ops.linear(x, weights[n], act=A, tile=tile, staging=st)
                except RuntimeError as e:
                    assert "DA_ERR_UNSUPPORTED" in str(e) or "DA_ERR_INVALID" in str(e), f"{L.TILE_NAMES[tile]}/{st} N{n}: {e}"
                    continue
                break
            if y is not None:
                break
        if y is None:
            continue
        what = f"{act} on {L.TILE_NAMES[tile]} (N {n}, staging {st})"
        assert y.shape == (x.shape[0], n // 2 if geglu else n)
        yb = _bits(y)
        assert bool((yb == yb[:, :1]).all()), f"{what}: the columns of a row differ"
        col = yb[:, 0].clone()
        if first is None:
            first, first_tile = col, tile
            vd.check_activation(vd.to_f64(y[:, 0]), domain["v64"], name, f"GEMM epilogue, {what}")
        else:
            nd = int((col != first).sum())
            assert nd == 0, f"{what}: {nd} of 65280 results differ from {L.TILE_NAMES[first_tile]}"
        ran.setdefault(_tile_family(L, tile), []).append(L.TILE_NAMES[tile])
    print(f"[value-domain] {act}: ran on {ran}")
    assert ran.get("first") and ran.get("k2"), f"{act}: a kernel family did not run ({ran})"
    assert ("k3:256x320" if geglu else "k3:256x256") in ran.get("k3", []), f"{act}: the eight-phase tile did not run ({ran})"


def test_linear_small_m_activations_over_all_finite_bf16(domain):
    """W = identity (K = N = 2048), 8 rows per call, four calls for the domain: act_in = SiLU on the input side, SiLU / tanh-GELU on
    the output side; the two-row instantiation on every 15th value."""
    ops, L = _ops()
    K = 2048
    eye = torch.eye(K, dtype=bf16, device=DEV)
    v = domain["v"]
    pad = torch.zeros(4 * 8 * K, dtype=bf16)
    pad[: v.numel()] = v
    xs = pad.view(4, 8, K).to(DEV)
    x2 = v[::15][: 2 * K].reshape(2, K).contiguous().to(DEV)
    for side, act_in, act_out, name in (("in", L.ACT_SILU, L.ACT_NONE, "silu"), ("out", L.ACT_NONE, L.ACT_SILU, "silu"),
                                        ("out", L.ACT_NONE, L.ACT_GELU_TANH, "gelu_tanh")):
        out = torch.cat([ops.linear_small_m(xs[i], eye, act_in=act_in, act_out=act_out) for i in range(4)]).reshape(-1)[: v.numel()]
        vd.check_activation(vd.to_f64(out), domain["v64"], name, f"linear_small_m act_{side} {name}")
        out2 = ops.linear_small_m(x2, eye, act_in=act_in, act_out=act_out)
        vd.check_activation(vd.to_f64(out2.reshape(-1)), vd.to_f64(x2.reshape(-1)), name, f"linear_small_m (2 rows) act_{side} {name}")


def _gn_form(monkeypatch, ops, form: str) -> None:
    """The env knobs of the GroupNorm form tests of test_kernels_gpu.py."""
    if form == "two_kernel":
        monkeypatch.setenv("DA_GN_FUSED", "0")
        monkeypatch.setenv("DA_GN_MULTI", "0")
    elif form == "one_launch":
        monkeypatch.setenv("DA_GN_MULTI", "0")
        monkeypatch.setenv("DA_GN_FUSED", "1")
        monkeypatch.setenv("DA_GN_FUSED_KB", "4096")
        monkeypatch.setenv("DA_GN_FUSED_MINWG", "1")
    else:
        monkeypatch.setattr(ops, "GN_MULTI", True)
        monkeypatch.setenv("DA_GN_MULTI", "1")
        monkeypatch.setenv("DA_GN_FUSED", "1")


def _positive_grid(domain, width: int):
    """The non-negative finite bf16 values (32 640, +0 and the denormals included), padded with 1.0 to whole chunks of `width`."""
    v = domain["v"]
    t = v[~torch.signbit(v.float())]
    assert t.numel() == vd.N_FINITE_BF16 // 2
    n = -(-t.numel() // width) * width
    return torch.cat([t, torch.ones(n - t.numel(), dtype=bf16)]).view(-1, width), t.numel()


@pytest.mark.parametrize("form", ["two_kernel", "one_launch"])
def test_groupnorm_silu_over_all_finite_bf16(domain, form, monkeypatch):
    """Groups of +1 (even pixels) and -1 (odd pixels): mean 0, var 1, so the normalised value is +-gamma_c / sqrt(1 + eps), which
    rounds to +-gamma_c in bf16 (5e-6 relative against half an ulp of 2^-9); gamma walks the non-negative bf16 grid, beta = 0.  The
    output is SiLU(+-t): the full op against fp64 with GroupNorm's tolerance, the SiLU factor with the tail condition."""
    ops, L = _ops()
    _gn_form(monkeypatch, ops, form)
    B, HW, C, G = 1, 16, 2560, 32
    grid, n_real = _positive_grid(domain, C)
    sign = torch.where(torch.arange(HW) % 2 == 0, 1.0, -1.0)
    x = sign[None, :, None].expand(B, HW, C).to(bf16).contiguous().to(DEV)
    beta = torch.zeros(C, dtype=bf16, device=DEV)
    outs, pres = [], []
    for gamma in grid:
        g = gamma.to(DEV)
        y = ops.group_norm_nhwc(x, g, beta, G, 1e-5, silu=True)
        vd.assert_close64(y, vd.group_norm_ref64(x, g, beta, G, 1e-5, silu=True), f"groupnorm + SiLU ({form}), gamma {float(gamma[0]):.3e}..",
                          **vd.TOL_GROUPNORM)
        outs.append(y[0, :2].cpu())                                     # one +1 pixel, one -1 pixel
        pres.append(torch.stack([gamma, -gamma]))
    out = torch.stack(outs, 1).reshape(2, -1)[:, :n_real].reshape(-1)
    pre = torch.stack(pres, 1).reshape(2, -1)[:, :n_real].reshape(-1)
    vd.check_activation(vd.to_f64(out), vd.to_f64(pre), "silu", f"GroupNorm apply + SiLU ({form})")


def test_rmsnorm_channels_silu_over_all_finite_bf16(domain):
    """Rows of +-1 over C = real_channels = 1024: x / ||x|| = +-1/32, * sqrt(1024) = +-1, * gamma_c = +-gamma_c, every step exact; gamma
    walks the non-negative bf16 grid.  The output is bf16(SiLU(+-t))."""
    ops, L = _ops()
    C = 1024
    grid, n_real = _positive_grid(domain, C)
    x = torch.stack([torch.ones(C), -torch.ones(C)]).to(bf16).to(DEV)
    outs, pres = [], []
    for gamma in grid:
        y = ops.rmsnorm_channels(x, gamma.to(DEV), real_channels=C, silu=True)
        outs.append(y.cpu())
        pres.append(torch.stack([gamma, -gamma]))
    out = torch.stack(outs, 1).reshape(2, -1)[:, :n_real].reshape(-1)
    pre = torch.stack(pres, 1).reshape(2, -1)[:, :n_real].reshape(-1)
    ref = torch.from_numpy(vd.act_ref64("silu", vd.to_f64(pre)))
    d = (out.double() - ref).abs()                                      # the op's own bound: one bf16 ulp of the reference chain
    assert int((d > ref.abs() * 2.0 ** -7 + 1e-6).sum()) == 0
    vd.check_activation(vd.to_f64(out), vd.to_f64(pre), "silu", "rmsnorm_channels + SiLU")


# ----------------------------------------------------------------------------------------------------------------------
# 2. normalisation kernels on hostile value families
# ----------------------------------------------------------------------------------------------------------------------
def _gn_cases():
    for form in ("two_kernel", "one_launch"):
        for shp in vd.GN_SHAPES:
            yield (form,) + shp + (0,)
        B, HW, C1, C2, G = vd.GN_TWO_SOURCE
        yield (form, B, HW, C1 + C2, G, C2)
    for shp in vd.GN_SHAPES_MULTI:
        yield ("several_workgroups",) + shp + (0,)
    B, HW, C1, C2, G = vd.GN_TWO_SOURCE_MULTI
    yield ("several_workgroups", B, HW, C1 + C2, G, C2)


@pytest.mark.parametrize("form,B,HW,C,G,C2", list(_gn_cases()))
def test_groupnorm_on_hostile_value_families(form, B, HW, C, G, C2, monkeypatch):
    ops, L = _ops()
    _gn_form(monkeypatch, ops, form)
    gamma, beta = (t.to(DEV) for t in vd.affine(C))
    for i, (kind, level) in enumerate(vd.GN_FAMILIES):
        x = vd.family_groups(kind, level, B, HW, C, G, seed=i).to(DEV)
        x1, x2 = (x[..., :C - C2].contiguous(), x[..., C - C2:].contiguous()) if C2 else (x, None)
        for silu in ((True,) if form == "several_workgroups" else (False, True)):
            y = ops.group_norm_nhwc(x1, gamma, beta, G, 1e-5, silu=silu, x2=x2)
            ref = vd.group_norm_ref64(x, gamma, beta, G, 1e-5, silu=silu)
            vd.assert_close64(y, ref, f"groupnorm ({form}) {B}x{HW}x{C - C2}+{C2}/{G} {kind} {level:g} silu={silu}", **vd.TOL_GROUPNORM)
    if form == "several_workgroups":
        torch.cuda.synchronize()
        assert not ops.gn_sync_error()


@pytest.mark.parametrize("M,C", vd.LN_SHAPES)
def test_layernorm_on_hostile_value_families(M, C):
    ops, L = _ops()
    gamma, beta = (t.to(DEV) for t in vd.affine(C))
    rpb = (M + 1) // 2
    for i, (kind, level) in enumerate(vd.FAMILIES):
        x = vd.family_rows(kind, level, M, C, seed=i).to(DEV)
        what = f"layernorm {M}x{C} {kind} {level:g}"
        vd.assert_close64(ops.layer_norm(x, gamma, beta, 1e-5), vd.layer_norm_ref64(x, gamma, beta, 1e-5), what, **vd.TOL_LAYERNORM)
        for dt in (torch.float32, bf16):
            sc, sh = (vd._randn((2, C), 50) * 0.3).to(dt).to(DEV), (vd._randn((2, C), 51) * 0.3).to(dt).to(DEV)
            y = ops.layer_norm(x, None, None, 1e-6, mod_scale=sc, mod_shift=sh, rows_per_batch=rpb)
            ref = vd.layer_norm_ref64(x, None, None, 1e-6, mod_scale=sc, mod_shift=sh, rows_per_batch=rpb)
            vd.assert_close64(y, ref, f"{what} adaLN {dt}", **vd.TOL_ADALN)


def test_rms_norms_on_hostile_value_families():
    """rmsnorm_rope_ per head / across heads with its own tolerance, one shape per kernel instantiation.  The bounds for rms_norm and
    rmsnorm_channels are CHOSEN HERE, not taken from the suite: the existing tests of these two ops compare against the reference's
    chain of bf16 roundings restated in fp32 (one ulp of it), which has no fp64 counterpart -- a chain rounded from fp64 values can
    land one step away at every link.  Against the unrounded fp64 value the error is bounded by the roundings the op performs, half a
    bf16 step (2^-8 relative at most) each: two for rms_norm, 2 * 2^-8 = 7.8e-3, for which LayerNorm's rtol 8e-3 / atol_rms 4e-3 is
    used; four for rmsnorm_channels (the last behind SiLU), 4 * 2^-8 = 1.56e-2, for which GroupNorm + SiLU's 1.6e-2 / 8e-3 is used."""
    ops, L = _ops()
    for i, (kind, level) in enumerate(vd.RMS_FAMILIES):
        for C in vd.RMS_NORM_WIDTHS:
            x, gamma = vd.family_rows(kind, level, 5, C, seed=i).to(DEV), vd.affine(C)[0].to(DEV)
            vd.assert_close64(ops.rms_norm(x, gamma, 1e-6), vd.rms_norm_ref64(x, gamma, 1e-6), f"rms_norm 5x{C} {kind} {level:g}",
                              **vd.TOL_LAYERNORM)
        for C in vd.RMS_CHANNELS_WIDTHS:
            x, gamma = vd.family_rows(kind, level, 37, C, seed=i).to(DEV), vd.affine(C)[0].to(DEV)
            for silu in (False, True):
                vd.assert_close64(ops.rmsnorm_channels(x, gamma, real_channels=C, silu=silu), vd.rmsnorm_channels_ref64(x, gamma, C, silu),
                                  f"rmsnorm_channels 37x{C} {kind} {level:g} silu={silu}", **vd.TOL_GROUPNORM)
        for D, heads in vd.RMS_ROPE_SHAPES:
            C = D * heads
            x = vd.family_rows(kind, level, 9, C, seed=i).to(DEV)
            wh, wa = vd.affine(D)[0].to(DEV), vd.affine(C)[0].to(DEV)
            y = ops.rmsnorm_rope_(x.clone(), heads=heads, head_dim=D, col_offsets=(0,), weights=(wh,), eps=1e-6)
            vd.assert_close64(y, vd.rms_norm_ref64(x, wh, 1e-6, unit=D), f"rmsnorm per head D{D}x{heads} {kind} {level:g}", **vd.TOL_RMS_ROPE)
            y = ops.rmsnorm_rope_(x.clone(), heads=heads, head_dim=D, col_offsets=(0,), weights=(wa,), eps=1e-6, norm="across_heads")
            vd.assert_close64(y, vd.rms_norm_ref64(x, wa, 1e-6), f"rmsnorm across heads D{D}x{heads} {kind} {level:g}", **vd.TOL_RMS_ROPE)


def _fold_producers(L):
    return [(L.TILE_128x128, L.STAGE_LDS_DIRECT), (L.TILE_K2_128x80, L.STAGE_PINGPONG)]


def _produce(ops, rows: torch.Tensor, wprod: torch.Tensor, tile: int, staging: int):
    """rows [M][C] through a producing GEMM: a = 0, so the launch's output IS `rows` and its statistics are theirs."""
    M = rows.shape[0]
    st = ops.RowStats(M, DEV)
    a = torch.zeros((M, 64), dtype=bf16, device=DEV)
    x = ops.linear(a, wprod, residual=rows, tile=tile, staging=staging, stats_out=st)
    assert torch.equal(x, rows)
    return x, st


def _fold_consumers(ops, L, x, wl, b, st, fold, act=None):
    """(tile name, output) of every tile that accepts ln= for this problem."""
    act = L.ACT_NONE if act is None else act
    for tile in range(1, len(L.TILE_NAMES)):
        for stg in (L.STAGE_LDS_DIRECT, L.STAGE_PINGPONG):
            try:
                yield L.TILE_NAMES[tile], ops.linear(x, wl, b, act=act, tile=tile, staging=stg, ln=(st, fold))
            except RuntimeError as e:       # a refusal is skipped; anything else (a launch error) is a failure
                assert "DA_ERR_UNSUPPORTED" in str(e) or "DA_ERR_INVALID" in str(e), f"{L.TILE_NAMES[tile]}/{stg}: {e}"
                continue
            break


@pytest.mark.parametrize("M,C,N", vd.FOLD_SHAPES)
def test_layernorm_fold_on_hostile_value_families(M, C, N):
    """linear(x, W', ln=) against fp64 LN(x) @ W^T + b (rel_rms <= 6e-3, the fold test's bound) and next to the unfolded path
    (layer_norm, then linear) on the same rows: offsets up to mean / sigma = 64, constant rows, an outlier per row, both scales;
    statistics from a first-family and a K2 producer, every consumer tile that takes the fold."""
    ops, L = _ops()
    gamma, beta, w, b = (t.to(DEV) for t in vd.fold_problem(C, N))
    wl, fold = ops.fold_layernorm(w, gamma, beta, vd.LN_EPS)
    wprod = vd._randn((C, 64), 9).to(bf16).to(DEV)
    fams_ran = set()
    for name, rows in vd.fold_families(M, C).items():
        rows = rows.to(DEV)
        ref = vd.fold_ref64(rows, gamma, beta, w, b)
        plain = ops.linear(ops.layer_norm(rows, gamma, beta, vd.LN_EPS), w, b, tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
        e_plain = vd.assert_close64(plain, ref, f"unfolded {M}x{C}x{N} {name}", **vd.TOL_FOLD)
        e_fold, per_level = 0.0, [0.0] * len(vd.OFFSET_LEVELS)
        for ptile, pstg in _fold_producers(L):
            x, st = _produce(ops, rows, wprod, ptile, pstg)
            for tname, y in _fold_consumers(ops, L, x, wl, b, st, fold):
                e = vd.assert_close64(y, ref, f"fold {M}x{C}x{N} {name}: {L.TILE_NAMES[ptile]} -> {tname}", **vd.TOL_FOLD)
                e_fold = max(e_fold, e)
                fams_ran.add(tname[:2] if tname[:1] == "k" else "first")
                if name.startswith("offset"):                           # rows r, r + 4, ... are one level: the worst consumer of each
                    per_level = [max(pl, vd.rel_rms64(y[k::4], ref[k::4])) for k, pl in enumerate(per_level)]
        print(f"[value-domain] fold {M}x{C}x{N} {name}: e_fold {e_fold:.3e} e_plain {e_plain:.3e}")
        if name.startswith("offset"):
            for k, lv in enumerate(vd.OFFSET_LEVELS):
                print(f"[value-domain] fold {M}x{C}x{N} offset {lv:g}: e_fold {per_level[k]:.3e} "
                      f"e_plain {vd.rel_rms64(plain[k::4], ref[k::4]):.3e}")
    assert {"first", "k2"} <= fams_ran, f"consumers ran only on {fams_ran}"


@pytest.mark.parametrize("tanh", [False, True])
def test_layernorm_fold_geglu_consumer_on_hostile_value_families(tanh):
    """The GEGLU consumers (k3:256x320 among them) at a shape the eight-phase tile admits, with the fold + GEGLU bound of
    test_k3_geglu_tile_layernorm_fold_bit_identical_to_k1."""
    ops, L = _ops()
    M, C, N2 = vd.FOLD_GEGLU_SHAPE
    act = L.ACT_GEGLU_TANH if tanh else L.ACT_GEGLU
    gamma, beta, w1, b1 = (t.to(DEV) for t in vd.fold_problem(C, N2, seed=1))
    w1l, fold1 = ops.fold_layernorm(w1, gamma, beta, vd.LN_EPS)
    w1p, b1p = ops.pack_geglu(w1l, b1)
    n2 = N2 // 2
    idx = torch.arange(n2, device=DEV).view(n2 // 32, 32)
    order = torch.cat([idx, idx + n2], dim=1).reshape(-1)
    fold1p = ops.LNFold(fold1.s[order].contiguous(), fold1.c[order].contiguous(), fold1.eps)
    wprod = vd._randn((C, 64), 9).to(bf16).to(DEV)
    ran = set()
    for name, rows in vd.fold_families(M, C).items():
        rows = rows.to(DEV)
        ref = vd.geglu_ref64(vd.fold_ref64(rows, gamma, beta, w1, b1), tanh)
        for ptile, pstg in _fold_producers(L):
            x, st = _produce(ops, rows, wprod, ptile, pstg)
            for tname, y in _fold_consumers(ops, L, x, w1p, b1p, st, fold1p, act=act):
                vd.assert_close64(y, ref, f"fold + GEGLU{'-tanh' if tanh else ''} {name}: {L.TILE_NAMES[ptile]} -> {tname}", rtol=2.5e-2,
                                  atol_rms=2.5e-2, rel_rms_max=8e-3)
                ran.add(tname)
    assert "k3:256x320" in ran and "128x128" in ran, f"GEGLU consumers ran only on {ran}"


@pytest.mark.parametrize("M,C,N", vd.FOLD_SHAPES)
@pytest.mark.parametrize("level", vd.FOLD_EXTREME_LEVELS)
def test_layernorm_fold_at_extreme_offsets_is_no_worse_than_the_unfolded_path(level, M, C, N):
    """mean / sigma = 128 and 256 (bf16 keeps 2 and 1 bits of the spread there): e_fold <= max(6e-3, 1.5 e_plain), rel-rms against
    fp64 -- the fold skips one bf16 rounding, so it should not lose to the path it replaces; 1.5 allows for another summation order."""
    ops, L = _ops()
    gamma, beta, w, b = (t.to(DEV) for t in vd.fold_problem(C, N))
    wl, fold = ops.fold_layernorm(w, gamma, beta, vd.LN_EPS)
    wprod = vd._randn((C, 64), 9).to(bf16).to(DEV)
    rows = vd.family_rows("offset", level, M, C, seed=int(level)).to(DEV)
    ref = vd.fold_ref64(rows, gamma, beta, w, b)
    plain = ops.linear(ops.layer_norm(rows, gamma, beta, vd.LN_EPS), w, b, tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
    e_plain, e_fold = vd.rel_rms64(plain, ref), 0.0
    for ptile, pstg in _fold_producers(L):
        x, st = _produce(ops, rows, wprod, ptile, pstg)
        for tname, y in _fold_consumers(ops, L, x, wl, b, st, fold):
            assert bool(torch.isfinite(y.float()).all())
            e = vd.rel_rms64(y, ref)
            print(f"[value-domain] fold {M}x{C}x{N} offset {level:g}: {L.TILE_NAMES[ptile]} -> {tname}: e_fold {e:.3e}")
            e_fold = max(e_fold, e)
    print(f"[value-domain] fold {M}x{C}x{N} offset {level:g}: e_fold {e_fold:.3e} e_plain {e_plain:.3e}")
    assert e_fold > 0.0 and e_fold <= max(6e-3, 1.5 * e_plain), f"e_fold {e_fold:.3e} vs e_plain {e_plain:.3e}"


# ----------------------------------------------------------------------------------------------------------------------
# 3. softmax_rows on hostile rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", vd.SOFTMAX_NS)
def test_softmax_rows_on_hostile_rows(N):
    """Every family through rows of a [64][ceil4(N) + 4] buffer into an `out` of the same width that holds a sentinel: fp64 softmax
    with the op's tolerance (absolute term per family), finite, row sums, columns >= N untouched."""
    ops, L = _ops()
    M, ld = vd.SOFTMAX_M, (N + 3) // 4 * 4 + 4
    for name in vd.SOFTMAX_FAMILIES:
        s = vd.softmax_family(name, N)
        buf = torch.full((M, ld), float("nan"))
        buf[:, :N] = s
        buf = buf.to(DEV)
        out = torch.full((M, ld), -7.0, dtype=bf16, device=DEV)
        ops.softmax_rows(buf[:, :N], out=out)
        assert bool((out[:, N:] == -7.0).all()), f"softmax {name} N{N}: columns >= N were written"
        p = out[:, :N]
        vd.check_softmax(p, s.to(DEV), f"softmax {name} N{N}")
        if name == "all_equal":
            assert torch.equal(p, torch.full_like(p, 1.0 / N)), f"softmax all-equal N{N}: not exactly bf16(1 / N)"
        if N % 4 == 0:                                                   # the contiguous call, no `out`
            assert torch.equal(ops.softmax_rows(s.to(DEV)), p), f"softmax {name} N{N}: the strided and the contiguous call differ"
