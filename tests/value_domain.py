"""TEST INFRASTRUCTURE ONLY: input generators and fp64 references for the value-domain tests (test_value_domain_cpu.py /
test_value_domain_gpu.py).  The rest of the suite feeds the kernels N(0, 1) data; this module holds the values that data never
reaches -- every finite bf16 bit pattern for the activations, rows / groups with a large common offset, no spread at all, one
dominating element or a scale far from 1 for the normalisations, and degenerate rows for the row softmax -- together with plain
fp64 restatements of the operations.  Everything here runs on the CPU; inputs are rounded to bf16 FIRST and every reference is
computed from the rounded values."""
from __future__ import annotations

import math

import numpy as np
import torch

bf16 = torch.bfloat16
f64 = torch.float64

# ----------------------------------------------------------------------------------------------------------------------
# the bf16 value domain and exact rounding to it
# ----------------------------------------------------------------------------------------------------------------------
N_FINITE_BF16 = 65280          # 2 signs x 255 finite exponents x 128 significands = 255 * 256


def all_finite_bf16() -> torch.Tensor:
    """Every finite bf16 bit pattern (both zeros, the denormals, up to +- bf16 max), in bit-pattern order: [65280] bf16."""
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    assert bits.size == N_FINITE_BF16
    return torch.from_numpy((bits << 16).view(np.float32).copy()).to(bf16)


BF16_MAX = float(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0])


def round_bf16(x) -> np.ndarray:
    """fp64 -> the nearest bf16 value (ties to even), returned as fp64.  ONE rounding (torch's double -> bf16 cast goes through
    fp32 and rounds twice); denormals are kept, values past bf16 max become inf."""
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    _, e = np.frexp(a)                                      # a = m * 2^e, m in [0.5, 1)
    ulp = np.ldexp(1.0, np.maximum(e - 8, -133))            # 8 significant bits; the denormal spacing is 2^-133
    r = np.rint(a / ulp) * ulp                              # (a power-of-two scaling is exact; rint rounds ties to even)
    r = np.where(r > BF16_MAX, np.inf, r)
    return np.copysign(np.where(a == 0, 0.0, r), x)


def to_f64(t: torch.Tensor) -> np.ndarray:
    return t.detach().to("cpu").to(f64).numpy()


# ----------------------------------------------------------------------------------------------------------------------
# activations: fp64 references, the fp32 restatement of csrc/common.cuh, the bound
# ----------------------------------------------------------------------------------------------------------------------
ACTS = ("silu", "gelu_erf", "gelu_tanh", "quick_gelu")
ACT_RTOL, ACT_ATOL = 2.0 ** -8, 5e-7    # one bf16 step + the absolute bound common.cuh states (it also absorbs denormal flushing)


def _sigmoid64(z: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))                     # exp overflow -> inf -> 0: the right limit


def act_ref64(name: str, v: np.ndarray) -> np.ndarray:
    """The activation in fp64 (NOT rounded to bf16).  The tails are evaluated in forms that keep their relative accuracy:
    erfc for the erf-GELU, x * sigmoid(2u) for the tanh-GELU.  quick_gelu is the reference model's chain with its inner bf16
    roundings, x * bf16(sigmoid(bf16(1.702 x))); the outer product is left unrounded like the other references."""
    v = np.asarray(v, dtype=np.float64)
    if name == "silu":
        return v * _sigmoid64(v)
    if name == "gelu_erf":
        erfc = torch.special.erfc(torch.from_numpy(-v / math.sqrt(2.0))).numpy()
        return 0.5 * v * erfc
    if name == "gelu_tanh":
        u = math.sqrt(2.0 / math.pi) * (v + 0.044715 * v * v * v)
        return v * _sigmoid64(2.0 * u)
    if name == "quick_gelu":
        return v * round_bf16(_sigmoid64(round_bf16(1.702 * v)))
    raise KeyError(name)


def act_model_f32(name: str, v: np.ndarray) -> np.ndarray:
    """csrc/common.cuh restated in numpy fp32 with exactly rounded exp2 / reciprocal / division in place of v_exp_f32 / v_rcp_f32
    (1 ulp each on the device): what the formulas themselves give, before any hardware approximation."""
    f = np.float32
    x = np.asarray(v, dtype=f)
    log2e = f(1.4426950408889634)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        if name == "silu":                                  # x / (1 + __expf(-x))
            return x / (f(1) + np.exp2((-x) * log2e))
        if name == "gelu_erf":
            ax = np.abs(x)
            t = f(1) / (f(0.3275911) * f(0.70710678118654752440) * ax + f(1))
            poly = t * f(1.061405429) + f(-1.453152027)
            poly = t * poly + f(1.421413741)
            poly = t * poly + f(-0.284496736)
            poly = t * poly + f(0.254829592)
            e = (poly * t) * np.exp2((x * x) * (f(-0.5) * log2e))
            return (f(0.5) * x) * np.where(x >= 0, f(2) - e, e)
        if name == "gelu_tanh":
            u = f(0.7978845608028654) * (x + f(0.044715) * x * x * x)
            return x * (f(1) / (f(1) + np.exp2(u * (f(-2) * log2e))))
        if name == "quick_gelu":
            tv = round_bf16(f(1.702) * x).astype(f)
            sg = f(1) / (f(1) + np.exp2((-tv) * log2e))
            return x * round_bf16(sg).astype(f)
    raise KeyError(name)


def check_activation(out, v, name: str, what: str) -> int:
    """The conditions of one (site, activation) sweep: `out` (what the site produced for the inputs `v`, any float array) is finite
    wherever the fp64 reference is finite and inside the bf16 range, and |out - ref64| <= 2^-8 |ref64| + 5e-7.  Prints and returns
    the number of inputs whose bf16 result differs from the exactly rounded fp64 value."""
    out = np.asarray(out, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    ref = act_ref64(name, v)
    ok_ref = np.isfinite(ref) & (np.abs(ref) <= BF16_MAX)
    assert ok_ref.all(), f"{what}: the fp64 reference leaves the bf16 range on finite inputs"
    bad_fin = ~np.isfinite(out)
    assert not bad_fin.any(), f"{what}: {int(bad_fin.sum())} non-finite outputs, first at x = {v[bad_fin][0]!r}"
    err = np.abs(out - ref)
    excess = err - ACT_RTOL * np.abs(ref)
    worst = int(np.argmax(excess))
    mism = int((round_bf16(out) != round_bf16(ref)).sum())
    print(f"[value-domain] {what}: {v.size} inputs, max excess over 2^-8 |ref| = {float(excess[worst]):.3e} at x = {v[worst]!r}, "
          f"bf16 result != rounded fp64 on {mism}")
    bad = excess > ACT_ATOL
    assert not bad.any(), (f"{what}: {int(bad.sum())} inputs outside 2^-8 |ref| + 5e-7; worst x = {v[worst]!r}: got {out[worst]!r}, "
                           f"reference {ref[worst]!r}")
    return mism


# ----------------------------------------------------------------------------------------------------------------------
# the project's bf16 tolerance (conftest.assert_close_bf16) against an fp64 reference -- evaluated in fp64, so that
# tensors that hold 2^16-scaled or bf16-max-sized values do not overflow the rms
# ----------------------------------------------------------------------------------------------------------------------
def rel_rms64(a: torch.Tensor, ref: torch.Tensor) -> float:
    a, ref = a.to(f64), ref.to(device=a.device, dtype=f64)
    return float((a - ref).pow(2).mean().sqrt() / (ref.pow(2).mean().sqrt() + 1e-300))


def assert_close64(a: torch.Tensor, ref: torch.Tensor, what: str, rtol: float, atol_rms: float, rel_rms_max=None) -> float:
    """|a - ref| <= atol_rms * rms(ref) + rtol * |ref| elementwise (+ a bound on the relative rms), finite; on a's device."""
    assert a.shape == ref.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(ref.shape)}"
    a, ref = a.to(f64), ref.to(device=a.device, dtype=f64)
    rms = float(ref.pow(2).mean().sqrt())
    err = (a - ref).abs()
    bad = int((~(err <= atol_rms * rms + rtol * ref.abs())).sum())          # (a NaN counts as a violation)
    rr = rel_rms64(a, ref)
    print(f"[value-domain] {what}: rel_rms={rr:.3e} max_abs={float(err.max()):.3e} ref_rms={rms:.3e} violations={bad}/{err.numel()}")
    assert bool(torch.isfinite(a).all()), f"{what}: non-finite output"
    assert bad == 0, f"{what}: {bad} elements outside the tolerance (max err {float(err.max()):.4e}, rel_rms {rr:.3e})"
    if rel_rms_max is not None:
        assert rr <= rel_rms_max, f"{what}: rel_rms {rr:.3e} > {rel_rms_max}"
    return rr


# the tolerances tests/test_kernels_gpu.py uses for the same ops (rtol, atol_rms)
TOL_GROUPNORM = dict(rtol=1.6e-2, atol_rms=8e-3)
TOL_LAYERNORM = dict(rtol=8e-3, atol_rms=4e-3)
TOL_ADALN = dict(rtol=1.6e-2, atol_rms=8e-3)
TOL_RMS_ROPE = dict(rtol=1.6e-2, atol_rms=8e-3)          # test_rmsnorm_rope_per_head / test_rmsnorm_across_heads
TOL_FOLD = dict(rtol=1.6e-2, atol_rms=1.6e-2, rel_rms_max=6e-3)   # test_layernorm_fold_producer_and_consumers
TOL_SOFTMAX = dict(rtol=8e-3, atol_rms=1e-3)


# ----------------------------------------------------------------------------------------------------------------------
# hostile value families for the normalisations
# ----------------------------------------------------------------------------------------------------------------------
OFFSET_LEVELS = (0.0, 8.0, 32.0, 64.0)                  # mean / sigma
CONSTANTS = (0.0, 1.0, -3.5, 1024.0)                    # sum exactly in fp32: mean exact, x - mean = 0
FOLD_CONSTANTS = (0.0, 1.0, -3.5)
SCALES = (2.0 ** -20, 2.0 ** 16)                        # the small one puts var far below eps
OUTLIER = 2.0 ** 15
FAMILIES = ([("offset", m) for m in OFFSET_LEVELS] + [("constant", c) for c in CONSTANTS] + [("outlier", OUTLIER)]
            + [("scale", s) for s in SCALES])
# GroupNorm without c = 1024: the apply pass is y = x * a + (beta - mean * a) with a = rstd * gamma (one fma per element, in the
# kernels and in torch's own fp32 GroupNorm alike).  On a constant slab rstd = eps^-1/2 = 316, so mean * a = 3.2e5 and beta is
# recovered to half an fp32 ulp of that, 1.6e-2 -- the fp32 stand-in misses the tolerance there (test_value_domain_cpu.py keeps the
# figure), so the case is outside what the op supports: |mean| * rstd * 2^-24 must stay below the tolerance.
GN_FAMILIES = [f for f in FAMILIES if f != ("constant", 1024.0)]
# the rms-type norms: constant rows with c = 1 only (no mean is subtracted: a constant row is an ordinary input for them)
RMS_FAMILIES = [f for f in FAMILIES if f[0] != "constant" or f[1] == 1.0]


def _randn(shape, seed: int) -> torch.Tensor:
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed))


def family_rows(kind: str, level: float, M: int, C: int, seed: int = 0) -> torch.Tensor:
    """[M][C] bf16 rows of one family (every row is one normalised unit)."""
    z = _randn((M, C), 1000 + seed)
    if kind == "offset":
        x = z + level
    elif kind == "constant":
        x = torch.full((M, C), float(level))
    elif kind == "outlier":
        x = z
        pos = torch.randint(0, C, (M,), generator=torch.Generator("cpu").manual_seed(2000 + seed))
        x[torch.arange(M), pos] = float(level)
    elif kind == "scale":
        x = z * level
    else:
        raise KeyError(kind)
    return x.to(bf16)


def family_groups(kind: str, level: float, B: int, HW: int, C: int, G: int, seed: int = 0) -> torch.Tensor:
    """[B][HW][C] bf16 channels-last tensor of one family; the normalised unit is (batch, group of C / G channels)."""
    if kind != "outlier":
        return family_rows(kind, level, B * HW, C, seed).view(B, HW, C)
    cpg = C // G
    x = _randn((B, HW, G, cpg), 1000 + seed)
    g = torch.Generator("cpu").manual_seed(2000 + seed)
    pix, ch = torch.randint(0, HW, (B, G), generator=g), torch.randint(0, cpg, (B, G), generator=g)
    bi, gi = torch.meshgrid(torch.arange(B), torch.arange(G), indexing="ij")
    x[bi, pix, gi, ch] = float(level)
    return x.reshape(B, HW, C).to(bf16)


def offset_mix_rows(M: int, C: int, levels, seed: int = 0) -> torch.Tensor:
    """[M][C] bf16 rows, row r from offset level levels[r % len(levels)] (a quarter of the rows from each of four levels)."""
    z = _randn((M, C), 3000 + seed)
    lv = torch.tensor([float(levels[r % len(levels)]) for r in range(M)])
    return (z + lv[:, None]).to(bf16)


def affine(C: int, seed: int = 0):
    """(gamma, beta) bf16 [C]: the 1 + 0.1 N / 0.1 N the norm tests of test_kernels_gpu.py use."""
    return (_randn((C,), 4000 + seed) * 0.1 + 1.0).to(bf16), (_randn((C,), 5000 + seed) * 0.1).to(bf16)


# ----------------------------------------------------------------------------------------------------------------------
# fp64 references of the normalisations
# ----------------------------------------------------------------------------------------------------------------------
def _silu64(t: torch.Tensor) -> torch.Tensor:
    return t * torch.sigmoid(t)


def group_norm_ref64(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, G: int, eps: float, silu: bool = False,
                     x2=None) -> torch.Tensor:
    """GroupNorm (+ SiLU) on [B][HW][C] channels-last (x2: second channel-concat source) in fp64, two-pass statistics."""
    xx = x.to(f64) if x2 is None else torch.cat([x.to(f64), x2.to(f64)], -1)
    B, HW, C = xx.shape
    v = xx.view(B, HW, G, C // G)
    mean = v.mean(dim=(1, 3), keepdim=True)
    var = (v - mean).pow(2).mean(dim=(1, 3), keepdim=True)
    y = ((v - mean) / torch.sqrt(var + eps)).reshape(B, HW, C) * gamma.to(f64) + beta.to(f64)
    return _silu64(y) if silu else y


def layer_norm_ref64(x: torch.Tensor, gamma, beta, eps: float, mod_scale=None, mod_shift=None, rows_per_batch: int = 0) -> torch.Tensor:
    xx = x.to(f64)
    mean = xx.mean(-1, keepdim=True)
    var = (xx - mean).pow(2).mean(-1, keepdim=True)
    y = (xx - mean) / torch.sqrt(var + eps)
    if gamma is not None:
        y = y * gamma.to(f64)
    if beta is not None:
        y = y + beta.to(f64)
    if mod_scale is not None:
        bidx = torch.arange(x.shape[0], device=x.device) // rows_per_batch
        y = y * (1.0 + mod_scale.to(device=x.device, dtype=f64)[bidx]) + mod_shift.to(device=x.device, dtype=f64)[bidx]
    return y


def rms_norm_ref64(x: torch.Tensor, gamma, eps: float, unit: int = 0) -> torch.Tensor:
    """x * rsqrt(mean(x^2) + eps) * gamma over the last dim, or over consecutive blocks of `unit` channels (per-head norm; gamma is
    then [unit])."""
    xx = x.to(f64)
    shp = xx.shape
    if unit:
        xx = xx.reshape(shp[0], -1, unit)
    y = xx / torch.sqrt(xx.pow(2).mean(-1, keepdim=True) + eps)
    if gamma is not None:
        y = y * gamma.to(f64)
    return y.reshape(shp)


def rmsnorm_channels_ref64(x: torch.Tensor, gamma: torch.Tensor, real_channels: int, silu: bool = False) -> torch.Tensor:
    """WanRMS_norm: x / max(||x||, 1e-12) * sqrt(real_channels) * gamma (+ SiLU), without the reference's intermediate roundings."""
    xx = x.to(f64)
    y = xx / xx.norm(dim=-1, keepdim=True).clamp_min(1e-12) * math.sqrt(real_channels) * gamma.to(f64)
    return _silu64(y) if silu else y


# ----------------------------------------------------------------------------------------------------------------------
# row softmax: hostile rows
# ----------------------------------------------------------------------------------------------------------------------
SOFTMAX_M = 64
SOFTMAX_NS = (4, 77, 1000, 4096)
SOFTMAX_FAMILIES = ("all_equal", "dominant", "offset+1e4", "offset-1e4", "offset+1e30", "offset-1e30", "masked-1e30", "masked-inf",
                    "tied_max")


def softmax_family(name: str, N: int, M: int = SOFTMAX_M, seed: int = 0) -> torch.Tensor:
    """[M][N] fp32 scores."""
    z = _randn((M, N), 6000 + seed)
    rows = torch.arange(M)
    pos = torch.randint(0, N, (M,), generator=torch.Generator("cpu").manual_seed(7000 + seed))
    if name == "all_equal":
        return torch.full((M, N), 1.25) * (rows % 3 - 1).float()[:, None]          # rows of -1.25, 0, 1.25
    if name == "dominant":
        z[rows, pos] = z.max(dim=1).values + 100.0
        return z
    if name.startswith("offset"):
        return z * 3.0 + float(name[len("offset"):])
    if name.startswith("masked"):
        z = z * 3.0
        z[:, N - N // 3:] = -1e30 if name == "masked-1e30" else float("-inf")
        return z
    if name == "tied_max":
        top = z.max(dim=1).values + 5.0
        z[rows, pos] = top
        z[rows, (pos + 1 + N // 2) % N] = top
        return z
    raise KeyError(name)


def softmax_ref64(s: torch.Tensor) -> torch.Tensor:
    return torch.softmax(s.to(f64), dim=-1)


def check_softmax(p: torch.Tensor, s: torch.Tensor, what: str) -> None:
    """One family: the existing tolerance of softmax_rows against fp64 (its absolute term scaled to THIS family's rms), finite, and
    every row's fp32 sum of the bf16 probabilities within N * 2^-9 of 1 (each of N terms carries at most half a bf16 ulp)."""
    N = s.shape[1]
    assert_close64(p, softmax_ref64(s), what, **TOL_SOFTMAX)
    sums = p.float().sum(dim=1).cpu()
    dev = float((sums - 1.0).abs().max())
    print(f"[value-domain] {what}: max |row sum - 1| = {dev:.3e}")
    assert dev <= N * 2.0 ** -9, f"{what}: a row sums to 1 +- {dev:.3e}"


# ----------------------------------------------------------------------------------------------------------------------
# shapes: the smallest that still reach every code path of the kernel they feed
# ----------------------------------------------------------------------------------------------------------------------
GN_SHAPES = [(2, 77, 64, 32), (1, 1000, 96, 4), (2, 256, 960, 32)]            # (B, HW, C, G): two-kernel and one-launch forms
# the several-workgroup form.  It takes slabs over one CU's LDS (144 KiB) of group sets of at most 2 groups (norm.hip gn_fused_plan):
# (2, 4096, 320, 32) has 10 channels per group -> sets of 4 groups, which that form leaves to the two-kernel form (it is kept: the
# knobs must not break that hand-back); (2, 4001, 640, 32) and (2, 4096, 256, 8) take it with 4 parts (gn_multi_parts below).
GN_SHAPES_MULTI = [(2, 4096, 320, 32), (2, 4001, 640, 32), (2, 4096, 256, 8)]
GN_TWO_SOURCE = (2, 77, 64, 32, 4)                                          # (B, HW, C1, C2, G)
GN_TWO_SOURCE_MULTI = (2, 4096, 128, 128, 8)                                # 32 channels per group: 4 parts
LN_SHAPES = [(7, 1536), (33, 64), (64, 3072)]
RMS_NORM_WIDTHS = (512, 1024, 2048, 4096)                                   # rmsnorm_rows_kernel<1 / 2 / 4 / 8>
RMS_CHANNELS_WIDTHS = (64, 128, 256, 512, 1024)                             # launch buckets of 8 / 16 / 32 / 64 / 2 x 64 chunks
RMS_ROPE_SHAPES = [(64, 8), (128, 8), (128, 12), (64, 32), (128, 24), (128, 32)]   # (head_dim, heads): 1 / 2 / 3 / 4 / 6 / 8 chunks per lane
FOLD_SHAPES = [(512, 320, 384), (512, 1280, 256)]                           # (M, C, N)
FOLD_GEGLU_SHAPE = (256, 320, 640)                                          # (M, C, packed N) the k3:256x320 consumer admits
FOLD_EXTREME_LEVELS = (128.0, 256.0)
LN_EPS = 1e-5


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm fold: LN(x; gamma, beta) @ W^T + b
# ----------------------------------------------------------------------------------------------------------------------
def fold_problem(C: int, N: int, seed: int = 0):
    """(gamma, beta, W [N][C], b [N]) bf16, distributed like test_layernorm_fold_producer_and_consumers'."""
    gamma = (_randn((C,), 8000 + seed) * 0.3 + 1.0).to(bf16)
    beta = (_randn((C,), 8100 + seed) * 0.2).to(bf16)
    w = (_randn((N, C), 8200 + seed) * C ** -0.5).to(bf16)
    b = _randn((N,), 8300 + seed).to(bf16)
    return gamma, beta, w, b


def fold_families(M: int, C: int) -> dict:
    """name -> [M][C] bf16 rows for the fold: the four offset levels a quarter of the rows each, constant rows (c = 0, 1, -3.5 in
    turn), one 2^15 outlier per row, and the two scales."""
    const = torch.tensor([FOLD_CONSTANTS[r % len(FOLD_CONSTANTS)] for r in range(M)])[:, None].expand(M, C).to(bf16).contiguous()
    return {"offset 0/8/32/64": offset_mix_rows(M, C, OFFSET_LEVELS), "constant 0/1/-3.5": const,
            "outlier 2^15": family_rows("outlier", OUTLIER, M, C, 1), "scale 2^-20": family_rows("scale", SCALES[0], M, C, 2),
            "scale 2^16": family_rows("scale", SCALES[1], M, C, 3)}


def fold_ref64(x: torch.Tensor, gamma, beta, w: torch.Tensor, b, eps: float = LN_EPS) -> torch.Tensor:
    y = layer_norm_ref64(x, gamma, beta, eps) @ w.to(f64).t()
    return y if b is None else y + b.to(f64)


def geglu_ref64(pre: torch.Tensor, tanh: bool = False) -> torch.Tensor:
    """[M][2n] = [value | gate] pre-activations (fp64) -> value * gelu(gate)."""
    h, g = pre.chunk(2, dim=-1)
    if tanh:
        u = math.sqrt(2.0 / math.pi) * (g + 0.044715 * g * g * g)
        return h * g * torch.sigmoid(2.0 * u)
    return h * 0.5 * g * torch.special.erfc(-g / math.sqrt(2.0))


def gn_multi_parts(B: int, HW: int, C: int, G: int) -> int:
    """How many workgroups share one slab in the several-workgroup GroupNorm form (a restatement of norm.hip gn_fused_plan with the
    sync buffer present and the default knobs); 1 = the shape does not take that form."""
    cpg, gs = C // G, 1
    while gs <= 4 and (gs * cpg) % 8:
        gs += 1
    if gs > 2 or G % gs or B * HW * C < (1 << 20):              # (ops.group_norm_nhwc passes the sync buffer from 2^20 elements)
        return 1
    cw = gs * cpg
    nch, lcm = cw // 8, 64
    while lcm % nch:
        lcm += 64
    threads, wgs, lds = (1024 // lcm) * lcm, B * (G // gs), 144 * 1024
    if lcm > 1024 or wgs < 16 or HW * cw * 2 <= lds:
        return 1
    parts = 2
    while parts <= 32 and -(-HW // parts) * cw * 2 > lds:
        parts *= 2
    while parts * 2 <= 32 and wgs * parts * 2 <= 256 and -(-HW // (parts * 2)) >= 4 * (threads // nch):
        parts *= 2
    return parts if parts <= 32 and wgs * parts <= 256 else 1
