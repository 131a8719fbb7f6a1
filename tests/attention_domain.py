"""TEST INFRASTRUCTURE ONLY: hostile score distributions for flash attention (test_attention_domain_cpu.py /
test_attention_domain_gpu.py), in the style of value_domain.py.  The rest of the suite feeds the attention kernels N(0, 1) data;
this module holds what that data never reaches -- large common score offsets, offsets whose sign alternates inside one wave, scores
that climb or fall from key tile to key tile around the deferral threshold of the second-generation kernel, one key that wins by
hundreds of log2-units, no preference at all, values far from 1 -- and the masked families (a fully masked first or middle key tile,
interleaved masks, causal, biases with a large offset, a row without a visible key), together with

  * attention_ref64: the operation in fp64 from the bf16-rounded inputs, and
  * flash_model_f32: the arithmetic of csrc/attention.hip / csrc/attention2.hip restated in plain fp32 (64-key tiles, exp2 of
    s * scale * log2 e - m, P rounded to bf16 for the second product, the deferred maximum voted over 32-query waves, the AUG form
    with Q and m rounded to bf16, the row sum of the rounded P).  It shows which conditions a plain implementation can meet and
    gives the rel-rms floor the kernels are held to (1.5 x, the factor the suite already uses between a variant and its baseline).

Every generator puts the controlled part of the score into column 0 of each head of q and k: q's entry is a power of two, so the
product with k's bf16 entry is exact and the level (in score units AFTER `scale`) is what k's rounding leaves of the nominal one.
`onehot` needs one direction per key and uses columns 0 .. 9 (a +-32 binary code of the key index).  Everything runs on the CPU."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from value_domain import rel_rms64

bf16 = torch.bfloat16
f64 = torch.float64
LOG2E = 1.4426950408889634
TILE = 64                                # keys per tile of every flash kernel
WAVE = 32                                # queries per wave: the unit of the deferred-maximum vote
DEFER_LOG2 = 8.0                         # attention2.hip kDeferLog2
Q0 = 128.0                               # column 0 of q (a power of two)
ONEHOT_BITS, ONEHOT_AMP = 10, 32.0       # key index code: 10 columns of +-32 (products of 1024: exact)

# the suite's element-wise attention bounds (tests/test_kernels_gpu.py): |o - ref| <= tol * rms(ref) + tol * |ref|
TOL_DEFAULT = 1.6e-2                     # test_flash_attention: algo 0 / 1 / 2 / 4 and the first generation
TOL_AUG = 3e-2                           # test_flash_attention_v2_deferred_maximum: algo 3 / 5
REL_RMS_MASKED = 6e-3                    # test_masked_flash_attention
FLOOR_FACTOR = 1.5                       # kernel rel-rms <= 1.5 x the fp32 model's on the same inputs

OFFSET_LEVELS = (30.0, -30.0, 300.0, -300.0, 3000.0, -3000.0)     # (+-20000: fp32 score resolution alone breaks the bound)
ROWMIX_LEVELS = (300.0, 3000.0)
RAMP_STEPS = (7.5, 8.5, -7.5, -8.5, 40.0)                         # log2-units per 64-key tile
VSCALE_EXPONENTS = (-60, 60, 100)
FAMILIES = ([("offset", lv) for lv in OFFSET_LEVELS] + [("rowmix", lv) for lv in ROWMIX_LEVELS] + [("ramp", st) for st in RAMP_STEPS]
            + [("late_low_to_high", 300.0), ("late_high_to_low", 300.0), ("onehot", 0.0), ("uniform_keys", 0.0), ("uniform_q0", 0.0)]
            + [("vscale", float(e)) for e in VSCALE_EXPONENTS] + [("voutlier", 1e4)])
SPLIT_FAMILIES = [("offset", -300.0), ("ramp", 8.5), ("late_low_to_high", 300.0)]
SPLIT_SHAPE = (2, 20, 64, 1024, 1024)    # (B, H, D, Sq, Skv): the spiked-keys case of tests/test_attention_split.py

B_, H_, SQ = 1, 2, 130                   # one full 128-query block + a ragged one
SKVS = (333, 77)                         # five full tiles + 13 keys; one full tile + 13 keys
MASKED_S, MASKED_D = 130, 64


def family_id(f) -> str:
    return f"{f[0]}{f[1]:+g}" if f[1] else f[0]


def _randn(shape, seed: int) -> torch.Tensor:
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed))


# ----------------------------------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------------------------------
def onehot_pi(Sq: int, Skv: int) -> torch.Tensor:
    """The key query i selects: the first 64 queries hit key positions 0 .. 63 mod 64 spread over the full tiles, the rest walk the
    ragged tail (or, without a tail, the keys in steps of 7)."""
    full, tail = Skv // TILE, Skv % TILE
    pi = []
    for i in range(Sq):
        if i < TILE and full:
            pi.append(i + TILE * (i % full))
        elif tail:
            pi.append(full * TILE + (i % tail))
        else:
            pi.append((7 * i) % Skv)
    return torch.tensor(pi)


def family(kind: str, level: float, B: int, H: int, Sq: int, Skv: int, D: int, scale: float, seed: int = 0):
    """(q [B][Sq][H*D], k [B][Skv][H*D], v [B][Skv][H*D]) bf16 of one family; `level` in score units after `scale` (ramp: log2-units
    per tile; vscale: the exponent of two; voutlier: the factor)."""
    q = _randn((B, Sq, H, D), 100 + seed)
    k = _randn((B, Skv, H, D), 200 + seed)
    v = _randn((B, Skv, H, D), 300 + seed)
    tile = torch.arange(Skv) // TILE
    ntiles = (Skv + TILE - 1) // TILE
    unit = 1.0 / (Q0 * scale)                               # k's column-0 entry for a score of one unit
    if kind == "offset":
        q[..., 0], k[..., 0] = Q0, level * unit
    elif kind == "rowmix":
        q[..., 0] = (Q0 * (1.0 - 2.0 * (torch.arange(Sq) % 2)))[None, :, None]          # + - + - ... inside every wave
        k[..., 0] = level * unit
    elif kind == "ramp":
        q[..., 1:] *= 0.25                                  # score noise of 1 / 16: the tile maxima differ by the step, not by chance
        k[..., 1:] *= 0.25
        q[..., 0] = Q0
        k[..., 0] = (tile.float() * (level / LOG2E) * unit)[None, :, None]
    elif kind in ("late_low_to_high", "late_high_to_low"):
        lv = torch.zeros(Skv)
        lv[tile == 0], lv[tile == ntiles - 1] = -level, level
        q[..., 0] = Q0
        k[..., 0] = ((lv if kind == "late_low_to_high" else -lv) * unit)[None, :, None]
    elif kind == "onehot":
        assert Skv <= 1 << ONEHOT_BITS
        bits = lambda idx: ONEHOT_AMP * (2.0 * ((idx[:, None] >> torch.arange(ONEHOT_BITS)) & 1).float() - 1.0)    # noqa: E731
        q[..., :ONEHOT_BITS] = bits(onehot_pi(Sq, Skv))[None, :, None, :]
        k[..., :ONEHOT_BITS] = bits(torch.arange(Skv))[None, :, None, :]
    elif kind == "uniform_keys":
        k = k[:, :1].expand(B, Skv, H, D).clone()
    elif kind == "uniform_q0":
        q = torch.zeros_like(q)
    elif kind == "vscale":
        v = v * 2.0 ** level
    elif kind == "voutlier":
        v[:, Skv // 2] *= level
    else:
        raise KeyError(kind)
    return tuple(t.reshape(t.shape[0], t.shape[1], H * D).to(bf16) for t in (q, k, v))


def heads(t: torch.Tensor, H: int) -> torch.Tensor:
    """[B][S][H*D] -> [B][H][S][D]"""
    B, S, C = t.shape
    return t.view(B, S, H, C // H).permute(0, 2, 1, 3)


def scores64(q, k, H: int, scale: float) -> torch.Tensor:
    """scale * q . k^T in fp64: [B][H][Sq][Skv]"""
    return heads(q, H).to(f64) @ heads(k, H).to(f64).transpose(2, 3) * scale


# ----------------------------------------------------------------------------------------------------------------------
# fp64 reference
# ----------------------------------------------------------------------------------------------------------------------
def attention_ref64(q, k, v, H: int, scale: float, bias=None, causal: bool = False) -> torch.Tensor:
    """softmax(scale q k^T + bias) v in fp64 from the bf16 inputs: [B][Sq][H*D].  Bias entries <= -1e29 and causal positions
    (key > query) are -inf.  THE CONTRACT of a query without a visible key: its output row is zero."""
    B, Sq, C = q.shape
    Skv = k.shape[1]
    sc = scores64(q, k, H, scale)
    if bias is not None:
        bb = bias[..., :Skv].to(f64)
        sc = torch.where(bb <= -1e29, torch.full_like(sc, float("-inf")), sc + bb)
    if causal:
        sc = sc.masked_fill(torch.arange(Skv)[None, :] > torch.arange(Sq)[:, None], float("-inf"))
    dead = torch.isinf(sc).all(dim=-1, keepdim=True)
    p = torch.softmax(sc.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    return (p @ heads(v, H).to(f64)).permute(0, 2, 1, 3).reshape(B, Sq, C)


# ----------------------------------------------------------------------------------------------------------------------
# fp32 model of the kernels
# ----------------------------------------------------------------------------------------------------------------------
def _fma(a: torch.Tensor, b, c: torch.Tensor) -> torch.Tensor:
    """fp32 a * b + c with one rounding (the product of two fp32 values is exact in fp64)."""
    return (a.double() * float(b) + c.double()).float()


def flash_model_f32(q, k, v, H: int, scale: float, defer=None, aug: bool = False, rsm: bool = False, bias=None, causal: bool = False,
                    first_tile_rescale: bool = False, forget_alpha_on_l: bool = False) -> torch.Tensor:
    """The flash kernels' arithmetic in plain fp32 with exactly rounded exp2 / reciprocal: [B][Sq][H*D] bf16.
    defer = None: online softmax, the shift follows every tile's maximum (first generation; with bias / causal: the masked kernel).
    defer = 8:    the shift is raised only when some row of a 32-query wave outgrows it by more than 2^8 (second generation).
    aug:          Q * scale * log2 e rounded to bf16, the shift kept bf16-exact and subtracted inside the first product, first tile
                  sets it from 0 (algo 3 / 5; implies defer = 8).  first_tile_rescale: alpha = exp2(-shift) on the first tile as well
                  (what attention2.hip did before the zero accumulators were left alone: 0 * inf once the shift is below -128).
    rsm:          l is the sum of the bf16-ROUNDED probabilities (algo 4 / 5).
    forget_alpha_on_l: a deliberately wrong kernel (the negative control): the rescale reaches O but not l."""
    B, Sq, C = q.shape
    Skv, D = k.shape[1], C // H
    f = torch.float32
    sqp, skp = -(-Sq // WAVE) * WAVE, -(-Skv // TILE) * TILE
    qh = torch.zeros((B, H, sqp, D), dtype=f)
    kh, vh = torch.zeros((B, H, skp, D), dtype=f), torch.zeros((B, H, skp, D), dtype=f)
    qh[:, :, :Sq], kh[:, :, :Skv], vh[:, :, :Skv] = heads(q, H).float(), heads(k, H).float(), heads(v, H).float()
    sl2 = float(np.float32(scale) * np.float32(LOG2E))
    if aug:
        defer = DEFER_LOG2 if defer is None else defer
        qh = (qh * sl2).to(bf16).float()
    masked = bias is not None or causal
    assert not (masked and (aug or rsm or defer is not None)), "the masked kernel is the first generation's"
    m = torch.full((B, H, sqp), 0.0 if aug else -1e30, dtype=f)
    l = torch.zeros((B, H, sqp), dtype=f)
    o = torch.zeros((B, H, sqp, D), dtype=f)
    one = torch.ones((), dtype=f)
    wave_any = lambda c: c.view(B, H, sqp // WAVE, WAVE).any(-1, keepdim=True).expand(B, H, sqp // WAVE, WAVE).reshape(B, H, sqp)  # noqa: E731
    qi = torch.arange(sqp)[:, None]
    if bias is not None:
        bpad = torch.zeros((bias.shape[0], bias.shape[1], bias.shape[2], skp), dtype=f)
        bpad[..., :Skv] = bias[..., :Skv].float()
        if bias.shape[2] > 1:                                # rows of the padded queries: the kernel reads row Sq - 1 for them
            bpad = torch.cat([bpad[:, :, :Sq], bpad[:, :, Sq - 1:Sq].expand(-1, -1, sqp - Sq, -1)], 2)
        inv_scale = float(np.float32(1.0) / np.float32(scale))
    for j in range(skp // TILE):
        kv = torch.arange(j * TILE, (j + 1) * TILE)
        s = qh @ kh[:, :, kv].transpose(2, 3)
        if aug:
            s = s - m[..., None]
        s = torch.where(kv >= Skv, torch.full_like(s, -1e30), s)
        if bias is not None:
            bt = bpad[..., kv]
            s = torch.where((bt <= -1e29) | (s <= -1e29), torch.full_like(s, -1e30), _fma(bt, inv_scale, s).expand_as(s))
        if causal:
            s = torch.where(kv[None, :] > qi, torch.full_like(s, -1e30), s)
        mx = s.max(-1).values
        if aug:
            vote = torch.ones_like(mx, dtype=torch.bool) if j == 0 else wave_any(mx > defer)
            m_new = (m + (mx if j == 0 else mx.clamp_min(0.0))).to(bf16).float()
            d_eff = torch.where(vote, m_new - m, torch.zeros_like(m))
            alpha = torch.exp2(-d_eff)
            if j == 0 and not first_tile_rescale:
                alpha = torch.ones_like(alpha)
            m = m + d_eff
            p = torch.exp2(s - d_eff[..., None])
        else:
            mxs = mx * sl2
            vote = torch.ones_like(mx, dtype=torch.bool) if defer is None else wave_any(mxs - m > defer)
            m_new = torch.where(vote, torch.maximum(m, mxs), m)
            alpha = torch.exp2(m - m_new)
            m = m_new
            p = torch.exp2(_fma(s, sl2, -m[..., None]))
            if masked:
                p = torch.where(s <= -1e29, torch.zeros_like(p), p)
        pb = p.to(bf16).float()
        l = l * (one if forget_alpha_on_l else alpha) + (pb if rsm else p).sum(-1)
        o = o * alpha[..., None] + pb @ vh[:, :, kv]
    inv = 1.0 / l
    if masked:
        inv = torch.where(l > 0, inv, torch.zeros_like(inv))          # a query without a visible key: zeros
    return (o * inv[..., None])[:, :, :Sq].permute(0, 2, 1, 3).reshape(B, Sq, C).to(bf16)


# which model form restates which variant (da_attention_params.algo; "v1" = the first generation)
MODEL_FORMS = {"v1": dict(), 0: dict(defer=DEFER_LOG2), 2: dict(defer=DEFER_LOG2), 4: dict(defer=DEFER_LOG2, rsm=True), 3: dict(aug=True),
               5: dict(aug=True, rsm=True), 1: dict()}


def tol_of(variant) -> float:
    return TOL_AUG if variant in (3, 5) else TOL_DEFAULT


# ----------------------------------------------------------------------------------------------------------------------
# the conditions
# ----------------------------------------------------------------------------------------------------------------------
def check(out: torch.Tensor, ref: torch.Tensor, model_rr, what: str, tol: float, rel_rms_max=None) -> list:
    """The conditions of one (case, variant): finite wherever the fp64 reference is, |out - ref| <= tol * rms(ref) + tol * |ref| for
    EVERY element, rel-rms <= 1.5 x the fp32 model's (model_rr; None: not compared) and <= rel_rms_max.  Prints the figures and
    returns the list of failed conditions (empty: all met), so that a test can report every variant before it asserts."""
    out, ref = out.detach().to("cpu").to(f64).reshape(ref.shape), ref.to(f64)
    rms = float(ref.pow(2).mean().sqrt())
    err = (out - ref).abs()
    bad = int((~(err <= tol * rms + tol * ref.abs())).sum())            # (a NaN counts as a violation)
    nonfin = int((~torch.isfinite(out) & torch.isfinite(ref)).sum())
    rr = rel_rms64(out, ref)
    floor = "-" if model_rr is None else f"{model_rr:.3e}"
    print(f"[parity] {what}: rel_rms={rr:.3e} model_rel_rms={floor} max_abs={float(err.nan_to_num(float('inf')).max()):.3e} "
          f"ref_rms={rms:.3e} violations={bad}/{err.numel()} non_finite={nonfin}")
    fails = []
    if nonfin:
        fails.append(f"{what}: {nonfin} non-finite outputs")
    if bad:
        fails.append(f"{what}: {bad} elements outside {tol:g} (rel_rms {rr:.3e})")
    if model_rr is not None and not rr <= FLOOR_FACTOR * model_rr:
        fails.append(f"{what}: rel_rms {rr:.3e} > {FLOOR_FACTOR} x the fp32 model's {model_rr:.3e}")
    if rel_rms_max is not None and not rr <= rel_rms_max:
        fails.append(f"{what}: rel_rms {rr:.3e} > {rel_rms_max:g}")
    return fails


def bf16_step(x: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 at |x| (fp64; normal range)."""
    _, e = torch.frexp(x.to(f64).abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=f64), e - 8)


def check_onehot(out: torch.Tensor, v: torch.Tensor, Sq: int, what: str) -> list:
    """`onehot`: row i of the output is row pi(i) of V to within one bf16 step; prints whether it is bit-equal."""
    want = v[:, onehot_pi(Sq, v.shape[1])]
    out = out.detach().to("cpu").reshape(want.shape)
    equal = bool(torch.equal(out, want))
    off = int(((out.to(f64) - want.to(f64)).abs() > bf16_step(want)).sum()) + int((~torch.isfinite(out.float())).sum())
    print(f"[parity] {what}: selected V rows bit-equal: {equal}; elements further than one bf16 step: {off}")
    return [f"{what}: {off} elements further than one bf16 step from the selected V row"] if off else []


# ----------------------------------------------------------------------------------------------------------------------
# cases, computed once and shared
# ----------------------------------------------------------------------------------------------------------------------
def default_scale(D: int) -> float:
    return D ** -0.5


class Case:
    """One (family, shape): inputs, the fp64 reference, and the fp32 model's rel-rms per form (computed on first use)."""

    def __init__(self, q, k, v, H, scale, bias=None, causal=False):
        self.q, self.k, self.v, self.H, self.scale, self.bias, self.causal = q, k, v, H, scale, bias, causal
        self.ref = attention_ref64(q, k, v, H, scale, bias, causal)
        self._rr = {}

    def model(self, variant="v1", **extra) -> torch.Tensor:
        return flash_model_f32(self.q, self.k, self.v, self.H, self.scale, bias=self.bias, causal=self.causal,
                               **MODEL_FORMS[variant], **extra)

    def model_rr(self, variant="v1") -> float:
        key = tuple(sorted(MODEL_FORMS[variant].items()))
        if key not in self._rr:
            self._rr[key] = rel_rms64(self.model(variant), self.ref)
        return self._rr[key]


@functools.lru_cache(maxsize=None)
def case(kind: str, level: float, D: int, Skv: int, B: int = B_, H: int = H_, Sq: int = SQ) -> Case:
    scale = default_scale(D)
    return Case(*family(kind, level, B, H, Sq, Skv, D, scale, seed=D + Skv), H, scale)


# ----------------------------------------------------------------------------------------------------------------------
# masked families (D = 64, Sq = Skv = 130: tiles 0 .. 63, 64 .. 127 and two keys)
# ----------------------------------------------------------------------------------------------------------------------
MASKED_FAMILIES = ("left_padding", "middle_tile", "interleaved", "causal", "causal_bias", "bias_offset+1e4", "bias_offset-1e4",
                   "dead_row")
SHARED_ROW_FAMILIES = ("left_padding", "middle_tile", "interleaved", "bias_offset+1e4", "bias_offset-1e4")    # bias_row_stride 0 as well
DEAD_ROW = 5


@functools.lru_cache(maxsize=None)
def masked_case(name: str, bias_dtype: torch.dtype, shared_row: bool, H: int = H_) -> Case:
    """One masked family: bias [1][H or 1][S or 1][192] of `bias_dtype` (None for plain causal), rounded to that type BEFORE the
    reference is taken."""
    S, D = MASKED_S, MASKED_D
    ld = -(-S // TILE) * TILE
    scale = 1.0 if name == "causal_bias" else default_scale(D)          # (T5's biased attention runs with scale 1)
    amp = 0.35 if name == "causal_bias" else 1.0
    q, k, v = (_randn((1, S, H * D), 400 + i) * (amp if i < 2 else 1.0) for i in range(3))
    q, k, v = q.to(bf16), k.to(bf16), v.to(bf16)
    if name == "causal":
        return Case(q, k, v, H, scale, None, True)
    assert not (shared_row and name not in SHARED_ROW_FAMILIES)
    bz = torch.zeros((1, 1, 1, ld)) if shared_row else torch.cat([_randn((1, H, S, S), 500) * 0.5, torch.zeros((1, H, S, ld - S))], -1)
    key = torch.arange(ld)
    if name == "left_padding":
        bz[..., key < 70] = -1e30                            # the whole first tile and six keys of the second
    elif name == "middle_tile":
        bz[..., (key >= TILE) & (key < 2 * TILE)] = -1e30
    elif name == "interleaved":
        bz[..., key % 2 == 1] = -1e30
    elif name.startswith("bias_offset"):
        bz = bz + float(name[len("bias_offset"):])
    elif name == "dead_row":
        bz[..., S - 30:] = -1e30                             # an ordinary padded tail ...
        bz[:, :, DEAD_ROW, :] = -1e30                        # ... and one query that sees no key at all
    elif name != "causal_bias":
        raise KeyError(name)
    return Case(q, k, v, H, scale, bz.to(bias_dtype), name == "causal_bias")


def masked_variants(name: str):
    """(bias dtype, shared row) combinations of one masked family."""
    if name == "causal":
        return [(None, False)]
    out = [(bf16, False), (torch.float32, False)]
    if name in SHARED_ROW_FAMILIES:
        out += [(bf16, True), (torch.float32, True)]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the kernels' operand layout
# ----------------------------------------------------------------------------------------------------------------------
def operands(q, k, v, device="cpu"):
    """(q [B*Sq][C], k [B*sa][C] zero padded, vt [C][B*sa] zero padded, keyword arguments of ops.attention) as the tests of
    test_kernels_gpu.py lay them out (Skv_alloc = ceil16(Skv))."""
    B, Sq, C = q.shape
    Skv = k.shape[1]
    sa = (Skv + 15) // 16 * 16
    kp = torch.zeros((B, sa, C), dtype=bf16)
    kp[:, :Skv] = k
    vt = torch.zeros((C, B, sa), dtype=bf16)
    vt[:, :, :Skv] = v.permute(2, 0, 1)
    kw = dict(B=B, Sq=Sq, Skv=Skv, Skv_alloc=sa, q_row_stride=C, k_row_stride=C, q_batch_stride=Sq * C, k_batch_stride=sa * C,
              vt_ld=B * sa, vt_batch_stride=sa)
    return q.reshape(B * Sq, C).to(device), kp.view(B * sa, C).to(device), vt.view(C, B * sa).to(device), kw


def log2_tile_maxima(c: Case) -> torch.Tensor:
    """[B][H][Sq][tiles]: every query's largest score of each key tile, in log2-units (fp64)."""
    sc = scores64(c.q, c.k, c.H, c.scale) * LOG2E
    Skv = sc.shape[-1]
    return torch.stack([sc[..., j:j + TILE].max(-1).values for j in range(0, Skv, TILE)], -1)


assert math.isclose(LOG2E, math.log2(math.e))
