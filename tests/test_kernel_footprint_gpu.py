"""Memory footprint of the HIP kernels: guard bands around every output, poison around every input (tests/footprint.py).

Each case runs a kernel twice through the C ABI on operands with leading dimensions wider than their rows: once with NaN sentinels
in everything that is not part of an operand (bands before and after, row tails, batch gaps), once on a zero-padded copy in the same
layout.  It asserts that (1) every byte outside the logical outputs -- and outside the inputs, which nothing may write -- is
unchanged, (2) the result is finite and within the existing tolerance (tests/test_kernels_gpu.py, same op) of a plain fp32 PyTorch
reference, (3) the two runs agree bit for bit: what lies next to an operand does not influence the result.

Declared exemptions (region a kernel may touch outside its nominal rectangle, and the header sentence that allows it):

    kernel                    region                                         include/diffusers_amd.h
    ------------------------  ---------------------------------------------  ---------------------------------------------------
    da_attention_bf16         reads keys [Skv, Skv_alloc) of K and V^T       "Skv_alloc ... = keys present in memory per batch";
                              (filled with +-bf16 max here, never NaN)       they may hold any finite value
    da_attention_bf16 (bias)  reads bias columns [Skv, ceil64(Skv))          "rows of bias_row_stride >= ceil64(Skv) elements"

(da_conv_thin_out_bf16 itself writes exactly [B][Cout][H][W]; the channels padded to 16 belong to the implicit-GEMM route of
ops.conv_thin_out, whose take pass is tested here with cpad 16.)  Nothing else is exempt; no entry point is exempt as a whole.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_bf16
from footprint import big_finite, bits_equal, guarded, poisoned

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
f32 = torch.float32
DEV = "cuda"


def _ops():
    from diffusers_amd import _lib as L
    from diffusers_amd import ops
    return ops, L


def rnd(shape, seed, scale=1.0, dtype=bf16):
    g = torch.Generator("cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Unsupported(Exception):
    pass


def _check(L, rc, what):
    if rc == 3:
        raise Unsupported(what)
    L.check(rc, what)


def run_both(what, launch, ins, make_outs, inplace=()):
    """launch(i, o) with i / o = dicts of views.  Runs it on the poisoned inputs and on clean (zero-padded) copies, each time into
    fresh guarded outputs; checks every guard band and that the two results agree bit for bit.  ``inplace``: names of ``ins`` the
    kernel updates in place (returned with the outputs; fresh copies per run).  Returns the poisoned run's results."""
    results = []
    for kind in ("poisoned", "clean"):
        src = {k: (g if g is None else (g.clean() if kind == "clean" else (poisoned(g.view, ld=g.ld, batch_stride=g._batch_stride_arg)
                                                                           if k in inplace else g)))
               for k, g in ins.items()}
        outs = make_outs()
        before = {k: g.snapshot() for k, g in src.items() if g is not None and k not in inplace}
        launch({k: (None if g is None else g.view) for k, g in src.items()}, {k: g.view for k, g in outs.items()})
        torch.cuda.synchronize()
        for k, g in outs.items():
            g.check(f"{what}: output {k} ({kind} inputs)")
        for k, g in src.items():
            if g is None:
                continue
            g.check(f"{what}: operand {k} ({kind} run)")
            if k not in inplace:
                assert torch.equal(g.bits, before[k]), f"{what}: read-only operand {k} was written ({kind} run)"
        res = {k: g.view.clone() for k, g in outs.items()}
        res.update({k: src[k].view.clone() for k in inplace})
        results.append(res)
    for k in results[0]:
        assert bool(torch.isfinite(results[0][k].float()).all()), f"{what}: {k} is not finite with poisoned surroundings"
        assert bits_equal(results[0][k], results[1][k]), \
            f"{what}: {k} differs between poisoned and zero-padded surroundings: something outside the operands was read"
    return results[0]


# ----------------------------------------------------------------------------------------------------------------------
# GEMM (da_gemm_bf16, conv == 0)
# ----------------------------------------------------------------------------------------------------------------------
def _gemm_launch(L, i, o, *, M, N, K, tile, staging, act=0, out_f32=False, split_k=1, rows_per_batch=0, gate_f32=0, vt_col0=0):
    ops, _ = _ops()
    p = L.GemmParams()
    p.A, p.W, p.C = i["A"].data_ptr(), i["W"].data_ptr(), o["C"].data_ptr()
    p.M, p.N, p.K = M, N, K
    p.lda, p.ldw, p.ldc = i["A"].stride(0), i["W"].stride(0), o["C"].stride(0)
    for name, field, ldf in (("bias", "bias", None), ("rowvec", "rowvec", "ld_rowvec"), ("gate", "gate", "ld_gate"),
                             ("residual", "residual", "ldr")):
        t = i.get(name)
        if t is not None:
            setattr(p, field, t.data_ptr())
            if ldf:
                setattr(p, ldf, t.stride(0))
    p.rows_per_batch, p.alpha, p.out_scale, p.act, p.out_f32, p.conv = rows_per_batch, 1.0, 1.0, act, int(out_f32), 0
    p.gate_f32, p.tile, p.staging, p.split_k = gate_f32, tile, staging, split_k
    if split_k > 1:
        ws, flags = ops.splitk_workspace(torch.device(DEV, torch.cuda.current_device()), _stream())
        p.workspace, p.sync_flags, p.workspace_bytes = ws.data_ptr(), flags.data_ptr(), ws.numel()
    if "vt" in o:
        p.vt, p.vt_col0, p.ld_vt = o["vt"].data_ptr(), vt_col0, o["vt"].stride(0)
    _check(L, L.load().da_gemm_bf16(C.byref(p), _stream()), f"da_gemm_bf16 tile {tile} staging {staging}")


def _gemm_variants(L):
    first = [(t, s) for t in range(0, 5) for s in (L.STAGE_REGISTER, L.STAGE_LDS_DIRECT)]
    second = [(t, s) for t in range(L.FIRST_K2_TILE, len(L.TILE_NAMES))
              for s in (L.STAGE_LDS_DIRECT, L.STAGE_LDS_DIRECT3, L.STAGE_PINGPONG, L.STAGE_PINGPONG3)]
    return first, second


def _sweep(L, what, variants, run, must_run, families=()):
    """run(*variant) for every variant; DA_ERR_UNSUPPORTED skips one exactly as _run_variants does, but at least ``must_run``
    of them have to run, and at least one tile of every family named in ``families`` (prefixes of L.TILE_NAMES), so that no family
    drops out of the test unnoticed; the failure names what was skipped."""
    ran, skipped = [], []
    for v in variants:
        try:
            run(*v)
        except Unsupported:
            skipped.append(v)
            continue
        ran.append(v)
    assert len(ran) >= must_run, f"{what}: only {len(ran)} of {len(variants)} variants ran; refused: {skipped}"
    for fam in families:
        assert any(L.TILE_NAMES[v[0]].startswith(fam) for v in ran), f"{what}: no {fam}* tile ran; refused: {skipped}"
    return len(ran)


GEMM_SHAPES = [(M, N, K) for M in (1, 130, 257) for N in (68, 132) for K in (64, 192)]


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_footprint(M, N, K, out_f32):
    """Every tile family, both tails (M, N no multiple of any tile), lda = ldw = K + 8, ldc = N + 8, ldr = N + 16; bias, rowvec and
    residual present (the gate has its own test below)."""
    ops, L = _ops()
    rpb = (M + 1) // 2
    nb = (M + rpb - 1) // rpb
    x, w = rnd((M, K), 1), rnd((N, K), 2, K ** -0.5)
    bias, rowvec, res = rnd((N,), 3), rnd((nb, N), 4), rnd((M, N), 5)
    ins = dict(A=poisoned(x, ld=K + 8), W=poisoned(w, ld=K + 8), bias=poisoned(bias), rowvec=poisoned(rowvec, ld=N + 4),
               residual=poisoned(res, ld=N + 16))
    ref = x.float() @ w.float().t() + bias.float() + rowvec.float().repeat_interleave(rpb, 0)[:M] + res.float()
    tol = dict(rtol=1e-4, atol_rms=1e-4) if out_f32 else dict(rtol=8e-3, atol_rms=4e-3)
    if out_f32:   # the existing fp32-output tolerance is that of a bare product (test_gemm_epilogues)
        ins.update(bias=None, rowvec=None, residual=None)
        ref = x.float() @ w.float().t()
    first, second = _gemm_variants(L)

    def run(t, s):
        what = f"gemm {M}x{N}x{K} f32={out_f32} {L.TILE_NAMES[t]}/{s}"
        y = run_both(what, lambda i, o: _gemm_launch(L, i, o, M=M, N=N, K=K, tile=t, staging=s, out_f32=out_f32,
                                                     rows_per_batch=rpb),
                     ins, lambda: dict(C=guarded((M, N), ld=N + 8, dtype=f32 if out_f32 else bf16)))["C"]
        assert_close_bf16(y, ref, what, **tol)
    _sweep(L, "first family", first, run, must_run=10)
    _sweep(L, "second / third family", second, run, must_run=8, families=("k2:", "k1:", "k3:"))


@pytest.mark.parametrize("gate_f32", [0, 1])
def test_gemm_gate_footprint(gate_f32):
    ops, L = _ops()
    M, N, K, rpb = 130, 132, 192, 65
    x, w, bias, res = rnd((M, K), 6), rnd((N, K), 7, K ** -0.5), rnd((N,), 8), rnd((M, N), 9)
    gate = rnd((2, N), 10, dtype=f32 if gate_f32 else bf16)
    ins = dict(A=poisoned(x, ld=K + 8), W=poisoned(w, ld=K + 8), bias=poisoned(bias), gate=poisoned(gate, ld=N + 4),
               residual=poisoned(res, ld=N + 16))
    lin = x.float() @ w.float().t() + bias.float()
    gg = gate.float().repeat_interleave(rpb, 0)
    ref = res.float() + (lin.to(bf16).float() * gg if gate_f32 else (lin.to(bf16).float() * gg).to(bf16).float())
    first, _ = _gemm_variants(L)

    def run(t, s):
        what = f"gemm gate f32={gate_f32} {L.TILE_NAMES[t]}/{s}"
        y = run_both(what, lambda i, o: _gemm_launch(L, i, o, M=M, N=N, K=K, tile=t, staging=s, rows_per_batch=rpb,
                                                     gate_f32=gate_f32), ins, lambda: dict(C=guarded((M, N), ld=N + 8)))["C"]
        assert_close_bf16(y, ref, what, rtol=8e-3, atol_rms=4e-3)
    _sweep(L, "gate", first, run, must_run=10)


def test_gemm_split_k_footprint():
    """Split-K on one shape (workspace and flags are the library's, C is guarded)."""
    ops, L = _ops()
    M, N, K = 130, 132, 512
    x, w, bias, res = rnd((M, K), 11), rnd((N, K), 12, K ** -0.5), rnd((N,), 13), rnd((M, N), 14)
    ins = dict(A=poisoned(x, ld=K + 8), W=poisoned(w, ld=K + 8), bias=poisoned(bias), residual=poisoned(res, ld=N + 16))
    ref = x.float() @ w.float().t() + bias.float() + res.float()
    ran = 0
    for sk in (2, 4):
        def run(t, s, sk=sk):
            what = f"gemm split_k={sk} {L.TILE_NAMES[t]}/{s}"
            y = run_both(what, lambda i, o: _gemm_launch(L, i, o, M=M, N=N, K=K, tile=t, staging=s, split_k=sk), ins,
                         lambda: dict(C=guarded((M, N), ld=N + 8)))["C"]
            assert_close_bf16(y, ref, what, rtol=8e-3, atol_rms=4e-3)
        ran += _sweep(L, f"split_k {sk}", [(t, 1) for t in range(0, 5)], run, must_run=1)
    assert not ops.splitk_error()


def test_gemm_geglu_footprint():
    """GEGLU epilogue: the packed weight has N = 256 rows (the entry point wants N % 128 == 0), the output 128 columns."""
    ops, L = _ops()
    M, Cc, K = 130, 128, 192
    x, w, b = rnd((M, K), 15), rnd((2 * Cc, K), 16, K ** -0.5), rnd((2 * Cc,), 17, 0.1)
    wp, bp = ops.pack_geglu(w, b)
    ins = dict(A=poisoned(x, ld=K + 8), W=poisoned(wp, ld=K + 8), bias=poisoned(bp))
    h = x.float() @ w.float().t() + b.float()
    hv, gate = h.chunk(2, dim=-1)
    ref = hv * F.gelu(gate)
    first, second = _gemm_variants(L)

    def run(t, s):
        what = f"geglu {L.TILE_NAMES[t]}/{s}"
        y = run_both(what, lambda i, o: _gemm_launch(L, i, o, M=M, N=2 * Cc, K=K, tile=t, staging=s, act=L.ACT_GEGLU), ins,
                     lambda: dict(C=guarded((M, Cc), ld=Cc + 8)))["C"]
        assert_close_bf16(y, ref, what, rtol=1.6e-2, atol_rms=8e-3)
    _sweep(L, "geglu first family", first, run, must_run=4)
    _sweep(L, "geglu second family", second, run, must_run=4)


def test_gemm_fused_qkv_footprint():
    """Transposed column block: columns >= vt_col0 leave as vt[n - vt_col0][m] with ld_vt > M; both C and vt are guarded.
    vt_col0 = 1280 is a multiple of every carrying tile's column count (80, 160, 128, 256)."""
    ops, L = _ops()
    M, K, col0, Nv = 130, 64, 1280, 72
    N = col0 + Nv
    x, w, bias = rnd((M, K), 18), rnd((N, K), 19, K ** -0.5), rnd((N,), 20)
    ins = dict(A=poisoned(x, ld=K + 8), W=poisoned(w, ld=K + 8), bias=poisoned(bias))
    ref = x.float() @ w.float().t() + bias.float()
    _, second = _gemm_variants(L)

    def run(t, s):
        what = f"fused qkv {L.TILE_NAMES[t]}/{s}"
        r = run_both(what, lambda i, o: _gemm_launch(L, i, o, M=M, N=N, K=K, tile=t, staging=s, vt_col0=col0), ins,
                     lambda: dict(C=guarded((M, col0), ld=col0 + 8), vt=guarded((Nv, M), ld=M + 14)))
        assert_close_bf16(r["C"], ref[:, :col0], what + " C", rtol=8e-3, atol_rms=4e-3)
        assert_close_bf16(r["vt"], ref[:, col0:].t(), what + " vt", rtol=8e-3, atol_rms=4e-3)
    _sweep(L, "fused qkv", second, run, must_run=4)


# ----------------------------------------------------------------------------------------------------------------------
# flash attention (da_attention_bf16)
# ----------------------------------------------------------------------------------------------------------------------
def _attn_operands(B, H, D, Sq, Skv, sa, seed):
    """Q [B][Sq][C] rows C + 8 apart; K [B][sa][C] rows C + 8 apart; V^T [C][B][sa] with vt_ld = B * sa + 8.  Keys [Skv, sa) of K
    and V^T hold +-bf16 max ("present in memory", any finite value); everything else outside is NaN."""
    Cc = H * D
    q, k, v = rnd((B, Sq, Cc), seed), rnd((B, Skv, Cc), seed + 1), rnd((B, Skv, Cc), seed + 2)
    kp = big_finite((B, sa, Cc), seed + 3)
    kp[:, :Skv] = k
    vt = big_finite((Cc, B, sa), seed + 4)
    vt[:, :, :Skv] = v.permute(2, 0, 1)
    ins = dict(q=poisoned(q.view(B * Sq, Cc), ld=Cc + 8), k=poisoned(kp.view(B * sa, Cc), ld=Cc + 8),
               vt=poisoned(vt.view(Cc, B * sa), ld=B * sa + 8))
    return q, k, v, ins


def _attn_launch(L, i, o, *, B, H, D, Sq, Skv, sa, scale=None, algo=0, q_block=0, ring_slots=0, causal=False, kv_split=1, ws=None):
    p = L.AttentionParams()
    p.q, p.k, p.vt, p.out = i["q"].data_ptr(), i["k"].data_ptr(), i["vt"].data_ptr(), o["out"].data_ptr()
    p.B, p.H, p.Sq, p.Skv, p.Skv_alloc, p.D = B, H, Sq, Skv, sa, D
    p.q_row_stride, p.k_row_stride, p.vt_ld, p.o_row_stride = i["q"].stride(0), i["k"].stride(0), i["vt"].stride(0), o["out"].stride(0)
    p.q_batch_stride, p.k_batch_stride, p.vt_batch_stride = Sq * p.q_row_stride, sa * p.k_row_stride, sa
    p.o_batch_stride = Sq * p.o_row_stride
    p.scale = (D ** -0.5) if scale is None else scale
    p.algo, p.q_block, p.ring_slots, p.causal, p.kv_split = algo, q_block, ring_slots, int(causal), kv_split
    b = i.get("bias")
    if b is not None:       # [Bb][H][Sq | 1][ceil64(Skv)], rows / heads / batches as the view's strides say
        p.bias, p.bias_f32 = b.data_ptr(), int(b.dtype == f32)
        p.bias_batch_stride = b.stride(0) if b.shape[0] > 1 else 0
        p.bias_head_stride = b.stride(1) if b.shape[1] > 1 else 0
        p.bias_row_stride = b.stride(2) if b.shape[2] > 1 else 0
    if ws is not None:
        p.split_ws, p.split_ws_bytes = ws.data_ptr(), ws.numel()
    _check(L, L.load().da_attention_bf16(C.byref(p), _stream()), "da_attention_bf16")


def _attn_ref(q, k, v, H, bias=None, causal=False, scale=None):
    B, Sq, Cc = q.shape
    D = Cc // H
    qh, kh, vh = (t.float().view(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    sc = qh @ kh.transpose(-1, -2) * (D ** -0.5 if scale is None else scale)
    if bias is not None:
        sc = torch.where(bias <= -1e29, torch.full_like(sc, float("-inf")), sc + bias)
    if causal:
        Skv = k.shape[1]
        sc = sc.masked_fill(torch.arange(Skv, device=sc.device)[None, :] > torch.arange(Sq, device=sc.device)[:, None], float("-inf"))
    return (torch.softmax(sc, -1) @ vh).transpose(1, 2).reshape(B * Sq, Cc)


# (algo, q_block, ring_slots): first generation with 64- / 128-query workgroups, second generation 128 / 256, its three variants
ATTN_VARIANTS = [(1, 128, 0), (1, 64, 2), (1, 128, 3), (2, 128, 0), (2, 256, 0), (2, 128, 4), (3, 128, 0), (3, 256, 0), (4, 128, 0),
                 (4, 256, 0), (5, 128, 0), (5, 256, 0)]


@pytest.mark.parametrize("D", [64, 96, 128, 160])
@pytest.mark.parametrize("Sq,Skv,wide", [(1, 1, False), (33, 77, False), (130, 200, False), (130, 77, True), (33, 200, True),
                                         (1, 200, False), (130, 1, False)])
def test_attention_footprint(D, Sq, Skv, wide):
    """Skv_alloc = next multiple of 8 (``wide``: next multiple of 64, plus 8); q rows C + 8 apart, vt_ld = B * Skv_alloc + 8, output
    rows C + 4 apart."""
    ops, L = _ops()
    B, H = 2, 2
    Cc = H * D
    sa = ((Skv + 63) // 64 * 64 + 8) if wide else (Skv + 7) // 8 * 8
    q, k, v, ins = _attn_operands(B, H, D, Sq, Skv, sa, 100 + D + Sq)
    ref = _attn_ref(q, k, v, H)

    def run(algo, qb, ns):
        what = f"attention D{D} Sq{Sq} Skv{Skv} alloc{sa} algo{algo} q_block{qb} ring{ns}"
        y = run_both(what, lambda i, o: _attn_launch(L, i, o, B=B, H=H, D=D, Sq=Sq, Skv=Skv, sa=sa, algo=algo, q_block=qb,
                                                     ring_slots=ns), ins, lambda: dict(out=guarded((B * Sq, Cc), ld=Cc + 4)))["out"]
        assert_close_bf16(y, ref, what, rtol=1.6e-2, atol_rms=1.6e-2)
    # the second generation exists for D = 64 / 128 only; the 64-query first-generation workgroup for D = 64 only
    _sweep(L, f"attention D{D}", ATTN_VARIANTS, run, must_run=11 if D == 64 else (9 if D == 128 else 2))


@pytest.mark.parametrize("kind", ["causal", "bias_bf16", "bias_f32", "shared_row", "causal_bias"])
@pytest.mark.parametrize("S", [33, 130])
def test_masked_attention_footprint(kind, S):
    """The masked variant (D = 64): causal, bf16 / fp32 bias with rows ceil64(S) + 8 apart, one bias row shared by all queries.  Bias
    columns [S, ceil64(S)) exist by contract and hold +-bf16 max."""
    ops, L = _ops()
    B, H, D = 2, 2, 64
    Cc, sa, ld = H * D, (S + 7) // 8 * 8, (S + 63) // 64 * 64
    causal = kind.startswith("causal")
    q, k, v, ins = _attn_operands(B, H, D, S, S, sa, 300 + S)
    bias = None
    if kind != "causal":
        shared = kind == "shared_row"
        dt = f32 if kind == "bias_f32" else bf16
        shape = (B, 1, 1, ld) if shared else (B, H, S, ld)
        bz = big_finite(shape, 310 + S, dtype=dt)
        bz[..., :S] = rnd(shape[:-1] + (S,), 311 + S, 0.5, dtype=dt)
        if shared:
            bz[0, ..., S // 2:S] = -10000.0
        else:
            bz[1, ..., S - 5:S] = -1e30
        ins["bias"] = poisoned(bz.view(-1, ld), ld=ld + 8)
        bias = bz[..., :S].float()

    def launch(i, o):
        if "bias" in i and i["bias"] is not None:
            i = dict(i)
            b2 = i["bias"]
            i["bias"] = b2.as_strided(bz.shape, (bz.shape[1] * bz.shape[2] * (ld + 8), bz.shape[2] * (ld + 8), ld + 8, 1), b2.storage_offset())
        _attn_launch(L, i, o, B=B, H=H, D=D, Sq=S, Skv=S, sa=sa, causal=causal, scale=1.0 if bias is not None else None)
    what = f"masked attention {kind} S{S}"
    y = run_both(what, launch, ins, lambda: dict(out=guarded((B * S, Cc), ld=Cc + 4)))["out"]
    assert_close_bf16(y, _attn_ref(q, k, v, H, bias=bias, causal=causal,
                                   scale=1.0 if bias is not None else None), what, rel_rms_max=6e-3)


def test_attention_key_split_footprint():
    """kv_split = 2 splits the keys of the tail blocks: it needs >= 8 key tiles (da_attention_split_plan), so Skv = 461 is the nearest
    accepted shape; the scratch part of the workspace is the test's own and is poisoned, its counters are zeroed once."""
    ops, L = _ops()
    B, H, D, Sq, Skv = 2, 2, 64, 130, 461
    sa, Cc = 464, H * D
    q, k, v, ins = _attn_operands(B, H, D, Sq, Skv, sa, 400)
    p = L.AttentionParams()
    p.B, p.H, p.Sq, p.Skv, p.Skv_alloc, p.D, p.kv_split = B, H, Sq, Skv, sa, D, 2
    full, tail, units = C.c_int(), C.c_int(), C.c_int()
    need = int(L.load().da_attention_split_plan(C.byref(p), C.byref(full), C.byref(tail), C.byref(units)))
    assert units.value == 2 and tail.value > 0 and need > L.ATTN_SPLIT_COUNTER_BYTES, "this shape no longer splits: pick another"
    ws = guarded(need, dtype=torch.uint8)
    ws.view[:L.ATTN_SPLIT_COUNTER_BYTES] = 0
    ref = _attn_ref(q, k, v, H)
    for algo in (2, 3, 4, 5):
        what = f"attention kv_split=2 algo{algo}"
        y = run_both(what, lambda i, o: _attn_launch(L, i, o, B=B, H=H, D=D, Sq=Sq, Skv=Skv, sa=sa, algo=algo, kv_split=2, ws=ws.view),
                     ins, lambda: dict(out=guarded((B * Sq, Cc), ld=Cc + 4)))["out"]
        ws.check(what + ": workspace")
        assert_close_bf16(y, ref, what, rtol=1.6e-2, atol_rms=1.6e-2)


# ----------------------------------------------------------------------------------------------------------------------
# row and norm kernels (norm.hip)
# ----------------------------------------------------------------------------------------------------------------------
LN_WIDTHS = [8, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 3072, 3080, 4096]      # each instantiation at its two ends


def _ln_launch(L, i, o, M, Cc, eps, rpb=0):
    sc = i.get("mod_scale")
    _check(L, L.load().da_layernorm_bf16(i["x"].data_ptr(), None if i.get("gamma") is None else i["gamma"].data_ptr(),
                                         None if i.get("beta") is None else i["beta"].data_ptr(), o["y"].data_ptr(),
                                         None if sc is None else sc.data_ptr(), None if sc is None else i["mod_shift"].data_ptr(),
                                         0 if sc is None else sc.stride(0), int(sc is not None and sc.dtype == f32), rpb, M, Cc,
                                         i["x"].stride(0), o["y"].stride(0), eps, _stream()), "da_layernorm_bf16")


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("Cc", LN_WIDTHS)
def test_layernorm_footprint(M, Cc):
    ops, L = _ops()
    x = rnd((M, Cc), 47, 1.5) + 0.3
    g, b = rnd((Cc,), 48) * 0.1 + 1.0, rnd((Cc,), 49, 0.1)
    outs = lambda: dict(y=guarded((M, Cc), ld=Cc + 16))        # noqa: E731
    xin = poisoned(x, ld=Cc + 8)
    ln = F.layer_norm(x.float(), (Cc,), None, None, 1e-5)
    y = run_both(f"layernorm affine {M}x{Cc}", lambda i, o: _ln_launch(L, i, o, M, Cc, 1e-5),
                 dict(x=xin, gamma=poisoned(g), beta=poisoned(b)), outs)["y"]
    assert_close_bf16(y, ln * g.float() + b.float(), f"layernorm affine {M}x{Cc}", rtol=8e-3, atol_rms=4e-3)
    y = run_both(f"layernorm plain {M}x{Cc}", lambda i, o: _ln_launch(L, i, o, M, Cc, 1e-5), dict(x=xin), outs)["y"]
    assert_close_bf16(y, ln, f"layernorm plain {M}x{Cc}", rtol=8e-3, atol_rms=4e-3)
    rpb = (M + 1) // 2
    nb = (M + rpb - 1) // rpb
    for dt, tol in ((bf16, dict(rtol=1.6e-2, atol_rms=8e-3)), (f32, dict(rtol=8e-3, atol_rms=4e-3))):
        sc, sh = rnd((nb, Cc), 50, 0.3, dtype=dt), rnd((nb, Cc), 51, 0.3, dtype=dt)
        what = f"layernorm {dt} modulation {M}x{Cc}"
        y = run_both(what, lambda i, o: _ln_launch(L, i, o, M, Cc, 1e-5, rpb),
                     dict(x=xin, mod_scale=poisoned(sc, ld=Cc + 8), mod_shift=poisoned(sh, ld=Cc + 8)), outs)["y"]
        ref = ln * (1 + sc.float().repeat_interleave(rpb, 0)[:M]) + sh.float().repeat_interleave(rpb, 0)[:M]
        assert_close_bf16(y, ref, what, **tol)


def test_layernorm_and_rmsnorm_refuse_rows_wider_than_their_largest_instantiation():
    ops, L = _ops()
    x, y, g = poisoned(rnd((1, 4104), 1), ld=4112), guarded((1, 4104), ld=4120), rnd((4104,), 2)
    with pytest.raises(Unsupported):
        _ln_launch(L, dict(x=x.view), dict(y=y.view), 1, 4104, 1e-5)
    with pytest.raises(Unsupported):
        _check(L, L.load().da_rmsnorm_bf16(x.ptr(), g.data_ptr(), y.ptr(), 1, 4104, 4112, 4120, 1e-6, _stream()), "da_rmsnorm_bf16")
    torch.cuda.synchronize()
    y.check("refused launch")


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("Cc", [8, 512, 520, 1024, 1032, 2048, 2056, 4096])      # rmsnorm_rows_kernel<1 / 2 / 4 / 8> at both ends
def test_rmsnorm_footprint(M, Cc):
    ops, L = _ops()
    x, g = rnd((M, Cc), 52, 1.5), rnd((Cc,), 53) * 0.1 + 1.0
    what = f"rmsnorm {M}x{Cc}"
    y = run_both(what, lambda i, o: _check(L, L.load().da_rmsnorm_bf16(i["x"].data_ptr(), i["gamma"].data_ptr(), o["y"].data_ptr(), M, Cc,
                                                                       i["x"].stride(0), o["y"].stride(0), 1e-6, _stream()), what),
                 dict(x=poisoned(x, ld=Cc + 8), gamma=poisoned(g)), lambda: dict(y=guarded((M, Cc), ld=Cc + 16)))["y"]
    xf = x.float()          # the check of test_text_encoder_epilogues_and_rmsnorm: the reference chain's two roundings, one ulp of its maximum
    want = g.float() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)).to(bf16).float()
    assert bits_equal(y, want.to(bf16)) or float((y.float() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max()), what


@pytest.mark.parametrize("N", [4, 76, 4096])
def test_softmax_rows_footprint(N):
    """ld = N + 4, ldo = ceil64(N) + 4: columns >= N of the output are left untouched (the promise of ops.softmax_rows).  Row 1 holds
    all-equal scores, row 2 one +80 spike among -80."""
    ops, L = _ops()
    M, ldo = 3, (N + 63) // 64 * 64 + 4
    s = rnd((M, N), 54, 3.0, dtype=f32)
    s[1] = 1.25
    s[2] = -80.0
    s[2, N // 2] = 80.0
    what = f"softmax rows N{N}"
    y = run_both(what, lambda i, o: _check(L, L.load().da_softmax_rows_f32_bf16(i["s"].data_ptr(), o["p"].data_ptr(), M, N, i["s"].stride(0),
                                                                                o["p"].stride(0), _stream()), what),
                 dict(s=poisoned(s, ld=N + 4)), lambda: dict(p=guarded((M, N), ld=ldo)))["p"]
    assert_close_bf16(y, torch.softmax(s.float(), -1), what, rtol=8e-3, atol_rms=1e-3)
    assert float(y[2, N // 2]) == 1.0 and float(y[2].float().sum()) == 1.0


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
def test_rmsnorm_rope_footprint(D, parts, rope):
    """In place on `parts` column blocks of x [rows][ld], ld wider than the parts: the columns between and after the blocks are part
    of the logical view here and must come back bit-identical, like the rows past `rows` and everything outside."""
    ops, L = _ops()
    heads, rows, extra = 2, 5, 3
    Cc = heads * D
    offs = [j * (Cc + 8) for j in range(parts)]            # 8 foreign columns between the blocks
    width = offs[-1] + Cc + 8
    x = rnd((rows + extra, width), 71)
    ws = [rnd((D,), 72 + j, 0.2) + 1 for j in range(parts)]
    ang = torch.rand((rows + 2, D // 2), generator=torch.Generator("cpu").manual_seed(74)) * 6.0
    cos, sin = (f(ang).repeat_interleave(2, 1).contiguous().to(DEV) for f in (torch.cos, torch.sin))
    ins = dict(x=poisoned(x, ld=width + 8), cos=poisoned(cos) if rope else None, sin=poisoned(sin) if rope else None,
               **{f"w{j}": poisoned(ws[j]) for j in range(parts)})

    def launch(i, o):
        co = (C.c_int * parts)(*offs)
        wp = (C.c_void_p * parts)(*[i[f"w{j}"].data_ptr() for j in range(parts)])
        _check(L, L.load().da_rmsnorm_rope_bf16(i["x"].data_ptr(), i["x"].stride(0), rows, rows, heads, D, parts, co, wp, 1e-6,
                                                None if not rope else i["cos"].data_ptr(), None if not rope else i["sin"].data_ptr(),
                                                2 if rope else 0, 1, _stream()), "da_rmsnorm_rope_bf16")
    what = f"rmsnorm_rope D{D} parts{parts} rope{rope}"
    y = run_both(what, launch, ins, dict, inplace=("x",))["x"]
    keep = torch.ones((rows + extra, width), dtype=torch.bool, device=DEV)
    for j in range(parts):
        keep[:rows, offs[j]:offs[j] + Cc] = False
        v = F.rms_norm(x[:rows, offs[j]:offs[j] + Cc].float().view(rows, heads, D), (D,), ws[j].float(), 1e-6).to(bf16).float()
        if rope:
            c, s = cos[2:2 + rows, None, :], sin[2:2 + rows, None, :]
            xr, xi = v.reshape(rows, heads, -1, 2).unbind(-1)
            v = v * c + torch.stack([-xi, xr], -1).flatten(2) * s
        assert_close_bf16(y[:rows, offs[j]:offs[j] + Cc], v.reshape(rows, Cc), f"{what} block {j}", rtol=1.6e-2, atol_rms=8e-3)
    assert bits_equal(y[keep], x[keep]), f"{what}: columns outside the parts or rows past `rows` changed"


@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("Cc", [8, 64, 72, 128, 136, 256, 264, 512, 520, 1024])      # launch buckets of 8 / 16 / 32 / 64 / 2 x 64 chunks
def test_rmsnorm_channels_footprint(Cc, rows):
    ops, L = _ops()
    x, g = rnd((rows, Cc), 81), rnd((Cc,), 82) * 0.1 + 1.0
    scale = float(Cc) ** 0.5
    what = f"rmsnorm_channels {rows}x{Cc}"
    y = run_both(what, lambda i, o: _check(L, L.load().da_rmsnorm_channels_bf16(i["x"].data_ptr(), i["gamma"].data_ptr(), o["y"].data_ptr(), rows,
                                                                                Cc, scale, L.ACT_NONE, _stream()), what),
                 dict(x=poisoned(x), gamma=poisoned(g)), lambda: dict(y=guarded((rows, Cc))))["y"]
    ref = (F.normalize(x.float(), dim=1).to(bf16) * scale * g).float()      # the chain and bound of test_rmsnorm_channels_vs_reference_ops
    d = (y.float() - ref).abs()
    assert int((d > ref.abs() * 2.0 ** -7 + 1e-6).sum()) == 0, f"{what}: more than one bf16 ulp from the reference chain"


@pytest.mark.parametrize("HW", [1, 77, 1000])
@pytest.mark.parametrize("Cc,G,C2", [(64, 32, 0), (96, 4, 0), (960, 32, 0), (96, 4, 32)])
def test_groupnorm_footprint(HW, Cc, G, C2):
    """The two-kernel and the one-launch form, as the shape selects them; x / x2 poisoned outside, y guarded, the workspace guarded
    beyond da_groupnorm_workspace_bytes."""
    ops, L = _ops()
    B, C1 = 2, Cc - C2
    x1, x2 = rnd((B, HW, C1), 91, 1.5) + 0.3, (rnd((B, HW, C2), 92, 1.5) if C2 else None)
    g, b = rnd((Cc,), 93) * 0.1 + 1.0, rnd((Cc,), 94, 0.1)
    lib = L.load()
    nbytes = max(int(lib.da_groupnorm_workspace_bytes(B, HW, Cc, G)), 4)
    ws = guarded(nbytes, dtype=torch.uint8)
    what = f"groupnorm HW{HW} C{Cc} G{G} C2={C2}"
    ins = dict(x=poisoned(x1.view(B * HW, C1)), x2=poisoned(x2.view(B * HW, C2)) if C2 else None, gamma=poisoned(g), beta=poisoned(b))
    y = run_both(what, lambda i, o: _check(L, lib.da_groupnorm_nhwc_bf16(i["x"].data_ptr(), None if i["x2"] is None else i["x2"].data_ptr(), C1,
                                                                         i["gamma"].data_ptr(), i["beta"].data_ptr(), o["y"].data_ptr(), ws.ptr(),
                                                                         B, HW, Cc, G, 1e-5, L.ACT_SILU, None, _stream()), what),
                 ins, lambda: dict(y=guarded((B * HW, Cc))))["y"]
    ws.check(what + ": workspace")
    xx = (x1 if x2 is None else torch.cat([x1, x2], -1)).float()
    ref = F.silu(F.group_norm(xx.transpose(1, 2), G, g.float(), b.float(), 1e-5)).transpose(1, 2).reshape(B * HW, Cc)
    assert_close_bf16(y, ref, what, rtol=1.6e-2, atol_rms=8e-3)


# ----------------------------------------------------------------------------------------------------------------------
# misc.hip
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 8, 33, 130])
@pytest.mark.parametrize("Cc", [1, 8, 33, 130])
def test_transpose_footprint(R, Cc):
    ops, L = _ops()
    x = rnd((R, Cc), 95)
    what = f"transpose {R}x{Cc}"
    try:
        y = run_both(what, lambda i, o: _check(L, L.load().da_transpose_bf16(i["x"].data_ptr(), o["y"].data_ptr(), R, Cc, i["x"].stride(0),
                                                                             o["y"].stride(0), _stream()), what),
                     dict(x=poisoned(x, ld=Cc + 8)), lambda: dict(y=guarded((Cc, R), ld=R + 8)))["y"]
    except Unsupported:
        pytest.fail(f"{what}: refused")
    assert bits_equal(y, x.t().contiguous())


@pytest.mark.parametrize("M,N,K", [(1, 132, 64), (5, 68, 192), (8, 132, 320)])
def test_linear_small_m_footprint(M, N, K):
    ops, L = _ops()
    x, w, b, res = rnd((M, K), 96), rnd((N, K), 97, K ** -0.5), rnd((N,), 98), rnd((M, N), 99)
    what = f"small-M linear {M}x{N}x{K}"
    y = run_both(what, lambda i, o: _check(L, L.load().da_linear_small_m_bf16(i["x"].data_ptr(), i["w"].data_ptr(), i["b"].data_ptr(),
                                                                              i["res"].data_ptr(), o["y"].data_ptr(), M, N, K, i["x"].stride(0),
                                                                              o["y"].stride(0), i["res"].stride(0), L.ACT_NONE, L.ACT_SILU,
                                                                              _stream()), what),
                 dict(x=poisoned(x, ld=K + 8), w=poisoned(w), b=poisoned(b), res=poisoned(res, ld=N + 16)),
                 lambda: dict(y=guarded((M, N), ld=N + 8)))["y"]
    assert_close_bf16(y, F.silu(x.float() @ w.float().t() + b.float()) + res.float(), what, rtol=1.6e-2, atol_rms=8e-3)


# ----------------------------------------------------------------------------------------------------------------------
# flat kernels (sampler.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _table(rows=3):
    t = torch.zeros((rows, 8))
    t[:, 0], t[:, 1] = torch.tensor([3.0, 2.0, 1.0])[:rows], torch.tensor([2.0, 1.0, 0.5])[:rows]
    t[:, 2] = t[:, 1] - t[:, 0]
    t[:, 3] = (t[:, 0] ** 2 + 1).sqrt()
    t[:, 5] = t[:, 0] ** 2 + 1
    t[:, 4] = -t[:, 0] / t[:, 3]
    return poisoned(t.to(DEV)), poisoned(torch.tensor([1], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("dt", [bf16, f32])
@pytest.mark.parametrize("n", [1, 7, 4097])
def test_flat_sampler_footprint(n, dt, cfg):
    """Out-of-place flat kernels: inputs poisoned outside their n (2n with cfg) elements, outputs guarded."""
    ops, L = _ops()
    lib, code = L.load(), (L.DTYPE_F32 if dt == f32 else L.DTYPE_BF16)
    table, step = _table()
    sigma, dtv, den = 2.0, -1.0, 5.0 ** 0.5
    e2, x = rnd(((2 if cfg else 1) * n,), 110, dtype=dt), rnd((n,), 111, dtype=dt)
    gd = 5.0
    e = (e2[:n].float() + gd * (e2[n:].float() - e2[:n].float())) if cfg else e2.float()
    if cfg and dt == bf16:
        e = e.to(bf16).float()
    ins = dict(e=poisoned(e2), x=poisoned(x), table=table, step=step)
    out = lambda rep=1: (lambda: dict(out=guarded(rep * n, dtype=dt)))       # noqa: E731
    tol = dict(rtol=1.6e-2, atol_rms=1.6e-2)

    y = run_both("euler_step", lambda i, o: _check(L, lib.da_euler_step(i["e"].data_ptr(), i["x"].data_ptr(), o["out"].data_ptr(), i["table"].data_ptr(),
                                                                        i["step"].data_ptr(), int(cfg), gd, n, code, L.PRED_EPSILON, _stream()), "euler"),
                 ins, out())["out"]
    assert_close_bf16(y, x.float() + e * dtv, f"euler_step n{n}", **tol)
    y = run_both("flowmatch_step", lambda i, o: _check(L, lib.da_flowmatch_step(i["e"].data_ptr(), i["x"].data_ptr(), o["out"].data_ptr(),
                                                                                i["table"].data_ptr(), i["step"].data_ptr(), int(cfg), gd, n, code, code,
                                                                                _stream()), "flowmatch"), ins, out())["out"]
    assert_close_bf16(y, x.float() + e * dtv, f"flowmatch_step n{n}", **tol)
    if not cfg:
        y = run_both("euler_scale_model_input", lambda i, o: _check(L, lib.da_euler_scale_model_input(i["x"].data_ptr(), o["out"].data_ptr(),
                                                                                                      i["table"].data_ptr(), i["step"].data_ptr(), 2, n, code,
                                                                                                      _stream()), "scale"), ins, out(2))["out"]
        assert_close_bf16(y, (x.float() / den).repeat(2), f"euler_scale_model_input n{n}", **tol)
        y = run_both("mul_scalar", lambda i, o: _check(L, lib.da_mul_scalar(i["x"].data_ptr(), o["out"].data_ptr(), 0.75, 2, n, code, _stream()), "mul"),
                     ins, out(2))["out"]
        assert_close_bf16(y, (x.float() * 0.75).repeat(2), f"mul_scalar n{n}", **tol)
        if dt == f32:
            y = run_both("cast_f32_bf16", lambda i, o: _check(L, lib.da_cast_f32_bf16(i["x"].data_ptr(), o["out"].data_ptr(), 2, n, _stream()), "cast"),
                         ins, lambda: dict(out=guarded(2 * n, dtype=bf16)))["out"]
            assert bits_equal(y, x.to(bf16).repeat(2))


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("dt", [bf16, f32])
@pytest.mark.parametrize("n", [1, 7, 4097])
def test_dpmpp_2m_step_in_place_footprint(n, dt, cfg):
    """In place on x and the fp32 history m1: nothing beyond their n elements changes.  Second-order row: x' = cx x + c0 x0 +
    cd (x0 - m1), x0 = (x - sigma e) / alpha, m1 <- x0."""
    ops, L = _ops()
    code = L.DTYPE_F32 if dt == f32 else L.DTYPE_BF16
    t = torch.zeros((3, 8))
    t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4], t[:, 6] = 0.8, 0.6, 0.5, 0.4, 0.25, 1.0
    e2, x, m1 = rnd(((2 if cfg else 1) * n,), 120, dtype=dt), rnd((n,), 121, dtype=dt), rnd((n,), 122, dtype=f32)
    gd = 3.0
    e = (e2[:n].float() + gd * (e2[n:].float() - e2[:n].float())) if cfg else e2.float()
    ins = dict(e=poisoned(e2), x=poisoned(x), m1=poisoned(m1), table=poisoned(t.to(DEV)),
               step=poisoned(torch.tensor([1], dtype=torch.int32, device=DEV)), begin=poisoned(torch.tensor([0], dtype=torch.int32, device=DEV)))
    r = run_both(f"dpmpp_2m n{n}", lambda i, o: _check(L, L.load().da_dpmpp_2m_step(i["e"].data_ptr(), i["x"].data_ptr(), i["m1"].data_ptr(),
                                                                                    i["table"].data_ptr(), i["step"].data_ptr(), i["begin"].data_ptr(),
                                                                                    int(cfg), gd, n, code, code, L.PRED_EPSILON, _stream()), "dpmpp"),
                 ins, dict, inplace=("x", "m1"))
    x0 = (x.float() - 0.6 * e) / 0.8
    assert_close_bf16(r["m1"], x0, f"dpmpp_2m history n{n}", rtol=1.6e-2, atol_rms=1.6e-2)
    assert_close_bf16(r["x"], 0.5 * x.float() + 0.4 * x0 + 0.25 * (x0 - m1), f"dpmpp_2m sample n{n}", rtol=1.6e-2, atol_rms=1.6e-2)


# ----------------------------------------------------------------------------------------------------------------------
# implicit-GEMM conv (da_gemm_bf16, conv == 1 / 3): NHWC sources with NaN directly before the first and after the last pixel
# ----------------------------------------------------------------------------------------------------------------------
CONV_GEOMS = [(1, 1, 1, 1, False), (2, 2, 2, 1, False), (2, 5, 7, 1, False), (1, 13, 9, 1, False),      # B, H, W, stride, up
              (2, 5, 7, 2, False), (1, 17, 17, 2, False), (2, 4, 4, 1, True)]


def _conv_case(B, H, W, stride, up, C2, Cout, ksize, seed=500):
    ops, L = _ops()
    C1, Ct = 64, 64 + C2
    x, x2 = rnd((B, H, W, C1), seed), (rnd((B, H, W, C2), seed + 1) if C2 else None)
    w = rnd((Cout, Ct, ksize, ksize), seed + 2, (ksize * ksize * Ct) ** -0.5)
    b, tv = rnd((Cout,), seed + 3, 0.1), rnd((B, Cout), seed + 4)
    xx = (x if x2 is None else torch.cat([x, x2], -1)).float().permute(0, 3, 1, 2)
    if up:
        xx = F.interpolate(xx, scale_factor=2.0, mode="nearest")
    if stride == 2:      # Downsample2D with padding = 0: F.pad (0, 1, 0, 1), as test_conv_downsample_asymmetric_pad
        ref = F.conv2d(F.pad(xx, (0, 1, 0, 1)), w.float(), b.float(), stride=2)
        geo = dict(stride=2, pad=0, pad_after=1)
    else:
        ref = F.conv2d(xx, w.float(), b.float(), padding=(ksize - 1) // 2)
        geo = dict(stride=1, up=up)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    res = rnd(tuple(ref.shape), seed + 5)
    ref = ref + tv.float()[:, None, None, :] + res.float()
    wp = ops.pack_conv_weight(w) if ksize == 3 else w.reshape(Cout, -1).contiguous()
    ins = dict(x=poisoned(x), x2=poisoned(x2) if C2 else None, w=poisoned(wp), b=poisoned(b), tv=poisoned(tv, ld=Cout + 8),
               res=poisoned(res))
    return ins, ref, geo


def _conv_run(what, ins, ref, geo, ksize, t, s):
    ops, L = _ops()

    def launch(i, o):
        try:
            ops.conv2d_nhwc(i["x"], i["w"], i["b"], ksize=ksize, x2=i["x2"], rowvec=i["tv"], residual=i["res"], tile=t, staging=s,
                            out=o["y"], **geo)
        except RuntimeError as e:
            if "DA_ERR_UNSUPPORTED" in str(e):
                raise Unsupported(str(e))
            raise
    y = run_both(what, launch, ins, lambda: dict(y=guarded(tuple(ref.shape))))["y"]
    assert_close_bf16(y, ref, what, rtol=8e-3, atol_rms=4e-3)


def _conv_variants(L):
    first = [(t, s) for t in (L.TILE_128x128, L.TILE_64x64) for s in (L.STAGE_REGISTER, L.STAGE_LDS_DIRECT)]
    second = [(t, s) for t in range(L.FIRST_K2_TILE, L.TILE_K3_256x256) if t not in (L.TILE_K2_80x128, L.TILE_K1_256x256, L.TILE_K1_256x320)
              for s in (L.STAGE_LDS_DIRECT, L.STAGE_PINGPONG)]
    return first, second


@pytest.mark.parametrize("Cout", [64, 68])
@pytest.mark.parametrize("C2", [0, 64])
@pytest.mark.parametrize("B,H,W,stride,up", CONV_GEOMS)
def test_conv3x3_footprint(B, H, W, stride, up, C2, Cout):
    """A tap that is not zero-filled above image 0 or below image B - 1 reads the NaN band and makes the output non-finite; a tap
    that crosses from one image into its neighbour shows against the reference."""
    ops, L = _ops()
    ins, ref, geo = _conv_case(B, H, W, stride, up, C2, Cout, 3)
    first, second = _conv_variants(L)
    run = lambda t, s: _conv_run(f"conv3x3 {B}x{H}x{W} s{stride} up{up} C64+{C2}->{Cout} {L.TILE_NAMES[t]}/{s}", ins, ref, geo, 3, t, s)  # noqa: E731
    _sweep(L, "conv first family", first, run, must_run=4)
    _sweep(L, "conv second family", second, run, must_run=1, families=("k2:", "k1:"))


@pytest.mark.parametrize("C2,Cout", [(0, 68), (64, 64)])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 5, 7)])
def test_conv1x1_footprint(B, H, W, C2, Cout):
    ops, L = _ops()
    ins, ref, geo = _conv_case(B, H, W, 1, False, C2, Cout, 1, seed=520)
    first, second = _conv_variants(L)
    run = lambda t, s: _conv_run(f"conv1x1 {B}x{H}x{W} C64+{C2}->{Cout} {L.TILE_NAMES[t]}/{s}", ins, ref, geo, 1, t, s)  # noqa: E731
    _sweep(L, "conv1x1 first family", first, run, must_run=4)
    _sweep(L, "conv1x1 second family", second, run, must_run=1, families=("k2:", "k1:"))


def test_conv3x3_chunked_k_order_footprint(monkeypatch):
    """One chunked K order, pinned through DA_CONV_CHUNK as tests/test_conv_chunk_gpu.py pins it: chunks of 64 of the 128 channels."""
    ops, L = _ops()
    monkeypatch.setenv("DA_CONV_CHUNK", "64")
    ins, ref, geo = _conv_case(2, 5, 7, 1, False, 64, 68, 3, seed=540)
    _, second = _conv_variants(L)

    def run(t, s):
        assert ops.conv_chunk_channels(ins["x"].view, ins["w"].view, t, x2=ins["x2"].view) == 64
        _conv_run(f"conv3x3 chunk 64 {L.TILE_NAMES[t]}/{s}", ins, ref, geo, 3, t, s)
    _sweep(L, "chunked conv", second, run, must_run=1, families=("k2:", "k1:"))


# ----------------------------------------------------------------------------------------------------------------------
# GroupNorm: each of the three forms pinned, as tests/test_kernels_gpu.py pins them
# ----------------------------------------------------------------------------------------------------------------------
def _gn_run(monkeypatch, form, B, HW, Cc, G, C2):
    ops, L = _ops()
    env = {"two": dict(DA_GN_FUSED="0", DA_GN_MULTI="0"), "one": dict(DA_GN_FUSED="1", DA_GN_MULTI="0", DA_GN_FUSED_KB="4096", DA_GN_FUSED_MINWG="1"),
           "multi": dict(DA_GN_FUSED="1", DA_GN_MULTI="1", DA_GN_FUSED_KB="0", DA_GN_FUSED_MINWG="1")}[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    C1 = Cc - C2
    x1, x2 = rnd((B, HW, C1), 91, 1.5) + 0.3, (rnd((B, HW, C2), 92, 1.5) if C2 else None)
    g, b = rnd((Cc,), 93) * 0.1 + 1.0, rnd((Cc,), 94, 0.1)
    lib = L.load()
    ws = guarded(max(int(lib.da_groupnorm_workspace_bytes(B, HW, Cc, G)), 4), dtype=torch.uint8)
    ws.view.fill_(0xA5)
    sync = None
    if form == "multi":
        sync = guarded(int(lib.da_groupnorm_sync_bytes()), dtype=torch.uint8)
    what = f"groupnorm [{form}] HW{HW} C{Cc} G{G} C2={C2}"
    ins = dict(x=poisoned(x1.view(B * HW, C1)), x2=poisoned(x2.view(B * HW, C2)) if C2 else None, gamma=poisoned(g), beta=poisoned(b))
    y = run_both(what, lambda i, o: _check(L, lib.da_groupnorm_nhwc_bf16(i["x"].data_ptr(), None if i["x2"] is None else i["x2"].data_ptr(), C1,
                                                                         i["gamma"].data_ptr(), i["beta"].data_ptr(), o["y"].data_ptr(), ws.ptr(),
                                                                         B, HW, Cc, G, 1e-5, L.ACT_SILU, None if sync is None else sync.ptr(),
                                                                         _stream()), what),
                 ins, lambda: dict(y=guarded((B * HW, Cc))))["y"]
    ws.check(what + ": workspace")
    wrote_ws = bool((ws.view != 0xA5).any())
    assert wrote_ws == (form == "two"), f"{what}: the {'two-kernel' if wrote_ws else 'one-launch'} form ran instead"
    if sync is not None:
        sync.check(what + ": sync buffer")
        assert bool((sync.view != 0).any()), f"{what}: the several-workgroup form did not run (its counters are untouched)"
        assert int(sync.view[4096 * 4:4096 * 4 + 4].view(torch.int32).item()) == 0, f"{what}: a part gave up waiting"
    xx = (x1 if x2 is None else torch.cat([x1, x2], -1)).float()
    ref = F.silu(F.group_norm(xx.transpose(1, 2), G, g.float(), b.float(), 1e-5)).transpose(1, 2).reshape(B * HW, Cc)
    assert_close_bf16(y, ref, what, rtol=1.6e-2, atol_rms=8e-3)


@pytest.mark.parametrize("form", ["two", "one"])
@pytest.mark.parametrize("HW", [1, 77, 1000])
@pytest.mark.parametrize("Cc,G,C2", [(64, 32, 0), (96, 4, 0), (960, 32, 0), (96, 4, 32)])
def test_groupnorm_forms_footprint(HW, Cc, G, C2, form, monkeypatch):
    _gn_run(monkeypatch, form, 2, HW, Cc, G, C2)


@pytest.mark.parametrize("C2", [0, 32])
def test_groupnorm_several_workgroups_footprint(C2, monkeypatch):
    """The several-workgroup form takes slabs beyond one CU's LDS (HW * channels of a group set * 2 B > 144 KiB) of group sets of
    at most two groups: none of the small shapes above; HW = 3077 at C = 96, G = 4 is the nearest that enters it."""
    _gn_run(monkeypatch, "multi", 2, 3077, 96, 4, C2)


# ----------------------------------------------------------------------------------------------------------------------
# misc.hip (the rest)
# ----------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else t.data_ptr()


def test_permute_patchify_frames_bcast_footprint():
    ops, L = _ops()
    lib = L.load()
    x = rnd((2, 3, 5, 8), 600)
    y = run_both("permute_0213", lambda i, o: _check(L, lib.da_permute_0213_bf16(_p(i["x"]), _p(o["y"]), 2, 3, 5, 8, _stream()), "permute"),
                 dict(x=poisoned(x)), lambda: dict(y=guarded((2, 5, 3, 8))))["y"]
    assert bits_equal(y, x.permute(0, 2, 1, 3).contiguous())
    B, Cc, Fr, H, W, (pt, ph, pw) = 2, 3, 2, 4, 6, (1, 2, 2)
    v = rnd((B, Cc, Fr, H, W), 601)
    f, h, w = Fr // pt, H // ph, W // pw
    tok = run_both("patchify3d", lambda i, o: _check(L, lib.da_patchify3d_bf16(_p(i["x"]), _p(o["y"]), B, Cc, Fr, H, W, pt, ph, pw, _stream()), "patchify"),
                   dict(x=poisoned(v)), lambda: dict(y=guarded((B * f * h * w, Cc * pt * ph * pw))))["y"]
    assert bits_equal(tok, v.view(B, Cc, f, pt, h, ph, w, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B * f * h * w, -1).contiguous())
    t2 = rnd((B * f * h * w, pt * ph * pw * Cc), 602)
    back = run_both("unpatchify3d", lambda i, o: _check(L, lib.da_unpatchify3d_bf16(_p(i["x"]), _p(o["y"]), B, Cc, Fr, H, W, pt, ph, pw, _stream()), "unpatchify"),
                    dict(x=poisoned(t2)), lambda: dict(y=guarded((B, Cc, Fr, H, W))))["y"]
    assert bits_equal(back, t2.view(B, f, h, w, pt, ph, pw, Cc).permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, Cc, Fr, H, W).contiguous())
    T, HW, Cs, Ck = 3, 7, 8, 3
    fr = rnd((B * T, HW, Cs), 603, 1.5)
    for of32 in (0, 1):
        vid = run_both("frames_to_ncthw", lambda i, o: _check(L, lib.da_frames_to_ncthw_bf16(_p(i["x"]), _p(o["y"]), B, T, HW, Cs, Ck, -1.0, 1.0, of32,
                                                                                             _stream()), "frames"),
                       dict(x=poisoned(fr)), lambda: dict(y=guarded((B, Ck, T, HW), dtype=f32 if of32 else bf16)))["y"]
        want = fr.view(B, T, HW, Cs)[..., :Ck].permute(0, 3, 1, 2).float().clamp(-1, 1)
        assert torch.equal(vid.float(), want)
    a, m = rnd((37,), 604, dtype=f32), rnd((3, 37), 605)
    out = run_both("bcast_add_f32", lambda i, o: _check(L, lib.da_bcast_add_f32(_p(i["a"]), _p(i["m"]), _p(o["y"]), 3, 37, _stream()), "bcast"),
                   dict(a=poisoned(a), m=poisoned(m)), lambda: dict(y=guarded((3, 37), dtype=f32)))["y"]
    assert torch.equal(out, a[None, :] + m.float())


@pytest.mark.parametrize("HW", [1, 7, 4099])
@pytest.mark.parametrize("cpad,cout", [(8, 3), (8, 4), (16, 3), (16, 4)])
def test_nhwc_take_and_postprocess_footprint(cpad, cout, HW):
    ops, L = _ops()
    lib, B = L.load(), 2
    x = rnd((B * HW, cpad), 610, 1.5)
    planes = run_both("nhwc_take_nchw", lambda i, o: _check(L, lib.da_nhwc_take_nchw_bf16(_p(i["x"]), _p(o["y"]), B, HW, cpad, cout, _stream()), "take"),
                      dict(x=poisoned(x)), lambda: dict(y=guarded((B, cout, HW))))["y"]
    assert bits_equal(planes, x.view(B, HW, cpad)[..., :cout].permute(0, 2, 1).contiguous())
    v = (planes.float() * 0.5 + 0.5).clamp(0, 1)
    for mode in (0, 1, 2):
        shape, dt = ((B, cout, HW) if mode == 0 else (B, HW, cout)), (torch.uint8 if mode == 2 else f32)
        fused = run_both(f"nhwc_take_postprocess mode {mode}", lambda i, o: _check(L, lib.da_nhwc_take_postprocess(_p(i["x"]), _p(o["y"]), B, HW, cpad, cout,
                                                                                                                   mode, _stream()), "take_pp"),
                         dict(x=poisoned(x)), lambda: dict(y=guarded(shape, dtype=dt)))["y"]
        sep = run_both(f"image_postprocess mode {mode}", lambda i, o: _check(L, lib.da_image_postprocess(_p(i["x"]), _p(o["y"]), B, cout, HW, 0, mode,
                                                                                                         _stream()), "pp"),
                       dict(x=poisoned(planes)), lambda: dict(y=guarded(shape, dtype=dt)))["y"]
        assert bits_equal(fused, sep), "the header's promise: the same values as take followed by image_postprocess"
        if mode < 2:
            assert_close_bf16(sep, v if mode == 0 else v.permute(0, 2, 1), f"image_postprocess mode {mode}")
    # fp32 input, uint8 output: every step of the chain is exact in fp32 up to torch's own round-half-even
    xf = planes.float()
    u8 = run_both("image_postprocess f32 -> uint8", lambda i, o: _check(L, lib.da_image_postprocess(_p(i["x"]), _p(o["y"]), B, cout, HW, 1, 2, _stream()), "pp"),
                  dict(x=poisoned(xf)), lambda: dict(y=guarded((B, HW, cout), dtype=torch.uint8)))["y"]
    assert torch.equal(u8, ((xf * 0.5 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 1))


def test_timestep_embedding_footprint():
    from oracle.reference_math import timestep_embedding as ref_te
    ops, L = _ops()
    t = torch.tensor([981.0, 1.0, 500.5])
    for dim, flip, shift in ((320, True, 0.0), (128, False, 1.0)):
        for of32 in (1, 0):
            got = run_both("timestep_embedding", lambda i, o: _check(L, L.load().da_timestep_embedding(_p(i["t"]), None, None, _p(o["y"]), 3, dim, int(flip),
                                                                                                       shift, 1.0, 10000.0, of32, _stream()), "temb"),
                           dict(t=poisoned(t.to(DEV))), lambda: dict(y=guarded((3, dim), dtype=f32 if of32 else bf16)))["y"]
            assert float((got.float().cpu() - ref_te(t, dim, flip, shift)).abs().max()) < (2e-3 if of32 else 6e-3)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (17, 30)])
def test_thin_convs_footprint(H, W):
    """conv_thin_in (NCHW source), conv_in_inpaint, vae_conv_in_image and conv_thin_out: poison before and after each source; 17 x 30
    runs the W tail of the four-pixel form."""
    ops, L = _ops()
    lib, B, Cout = L.load(), 2, 64
    tol = dict(rtol=8e-3, atol_rms=4e-3)
    x = rnd((B, 4, H, W), 620)
    w, b = rnd((Cout, 4, 3, 3), 621, 36 ** -0.5), rnd((Cout,), 622, 0.1)
    y = run_both("conv_thin_in", lambda i, o: _check(L, lib.da_conv_thin_in_bf16(_p(i["x"]), _p(i["w"]), _p(i["b"]), _p(o["y"]), B, H, W, 4, Cout, 3, 1,
                                                                                 1.0, 0.0, _stream()), "thin_in"),
                 dict(x=poisoned(x), w=poisoned(ops.pack_conv_weight(w)), b=poisoned(b)), lambda: dict(y=guarded((B, H, W, Cout))))["y"]
    assert_close_bf16(y, F.conv2d(x.float(), w.float(), b.float(), padding=1).permute(0, 2, 3, 1), f"conv_thin_in {H}x{W}", **tol)
    mask, masked = rnd((B, 1, H, W), 623), rnd((B, 4, H, W), 624)
    w9 = rnd((Cout, 9, 3, 3), 625, 81 ** -0.5)
    y = run_both("conv_in_inpaint", lambda i, o: _check(L, lib.da_conv_in_inpaint(_p(i["x"]), _p(i["mask"]), _p(i["masked"]), _p(i["w"]), _p(i["b"]),
                                                                                  _p(o["y"]), None, None, B, H, W, Cout, 2, B, _stream()), "inpaint_in"),
                 dict(x=poisoned(x), mask=poisoned(mask), masked=poisoned(masked), w=poisoned(ops.pack_conv_weight(w9)), b=poisoned(b)),
                 lambda: dict(y=guarded((2 * B, H, W, Cout))))["y"]
    r9 = F.conv2d(torch.cat([x, mask, masked], 1).float(), w9.float(), b.float(), padding=1).permute(0, 2, 3, 1)
    assert_close_bf16(y, torch.cat([r9, r9], 0), f"conv_in_inpaint {H}x{W}", **tol)
    img = rnd((B, 3, H, W), 626, 0.3, dtype=f32) + 0.5
    w3 = rnd((Cout, 3, 3, 3), 627, 27 ** -0.5)
    y = run_both("vae_conv_in_image", lambda i, o: _check(L, lib.da_vae_conv_in_image(_p(i["x"]), L.IMAGE_F32_NCHW, _p(i["w"]), _p(i["b"]), _p(o["y"]), B, H, W,
                                                                                      Cout, 1, _stream()), "vae_in"),
                 dict(x=poisoned(img), w=poisoned(ops.pack_conv_weight(w3)), b=poisoned(b)), lambda: dict(y=guarded((B, H, W, Cout))))["y"]
    assert_close_bf16(y, F.conv2d((2 * img - 1).to(bf16).float(), w3.float(), b.float(), padding=1).permute(0, 2, 3, 1), f"vae_conv_in_image {H}x{W}", **tol)
    xh = rnd((B, H, W, 64), 628)
    for co in (3, 4):
        wo, bo = rnd((co, 64, 3, 3), 629, 576 ** -0.5), rnd((co,), 630, 0.1)
        for of32 in (0, 1):
            y = run_both("conv_thin_out", lambda i, o: _check(L, lib.da_conv_thin_out_bf16(_p(i["x"]), _p(i["w"]), _p(i["b"]), _p(o["y"]), B, H, W, 64, co, of32,
                                                                                           _stream()), "thin_out"),
                         dict(x=poisoned(xh), w=poisoned(ops.pack_conv_weight(wo)), b=poisoned(bo)),
                         lambda: dict(y=guarded((B, co, H, W), dtype=f32 if of32 else bf16)))["y"]
            assert_close_bf16(y, F.conv2d(xh.float().permute(0, 3, 1, 2), wo.float(), bo.float(), padding=1), f"conv_thin_out {H}x{W} Cout {co}", **tol)


# ----------------------------------------------------------------------------------------------------------------------
# sampler.hip / vae_encode.hip (the rest)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("dt", [bf16, f32])
@pytest.mark.parametrize("n", [1, 7, 4097])
def test_x0_linear_and_unipc_footprint(n, dt, cfg):
    ops, L = _ops()
    lib, code, gd = L.load(), (L.DTYPE_F32 if dt == f32 else L.DTYPE_BF16), 3.0
    tol = dict(rtol=1.6e-2, atol_rms=1.6e-2)
    e2, x, noise = rnd(((2 if cfg else 1) * n,), 130, dtype=dt), rnd((n,), 131, dtype=dt), rnd((2 * n,), 132, dtype=dt)
    e = (e2[:n].float() + gd * (e2[n:].float() - e2[:n].float())) if cfg else e2.float()
    step = poisoned(torch.tensor([1], dtype=torch.int32, device=DEV))
    t = torch.zeros((3, 8))
    t[:, 0], t[:, 1], t[:, 2], t[:, 3], t[:, 4], t[:, 5] = 0.6, 0.8, 0.9, 0.2, 0.1, 0.3     # sqrt(beta), sqrt(alpha), k0, ke, kx, kn
    y = run_both("x0_linear_step", lambda i, o: _check(L, lib.da_x0_linear_step(_p(i["e"]), _p(i["x"]), _p(i["noise"]), n, _p(o["y"]), _p(i["table"]),
                                                                                _p(i["step"]), int(cfg), gd, n, code, L.PRED_EPSILON, _stream()), "x0"),
                 dict(e=poisoned(e2), x=poisoned(x), noise=poisoned(noise), table=poisoned(t.to(DEV)), step=step), lambda: dict(y=guarded(n, dtype=dt)))["y"]
    x0 = (x.float() - 0.6 * e) / 0.8
    assert_close_bf16(y, 0.9 * x0 + 0.2 * e + 0.1 * x.float() + 0.3 * noise[n:].float(), f"x0_linear_step n{n}", **tol)
    # UniPC, corrector and predictor of order 2: in place on x / last / m1 / m2
    c = torch.zeros((3, 16))
    c[:] = torch.tensor([0.7, 1, 2, 0.9, 0.3, 0.2, 0.5, 0.4, 0.6, 2, 0.8, 0.25, 0.15, 0.5, 0, 0])
    last, m1, m2 = (rnd((n,), 133 + k, dtype=dt) for k in range(3))
    r = run_both("unipc_flow_step", lambda i, o: _check(L, lib.da_unipc_flow_step(_p(i["e"]), _p(i["x"]), _p(i["last"]), _p(i["m1"]), _p(i["m2"]), _p(i["coef"]),
                                                                                  _p(i["step"]), int(cfg), gd, n, code, code, _stream()), "unipc"),
                 dict(e=poisoned(e2), x=poisoned(x), last=poisoned(last), m1=poisoned(m1), m2=poisoned(m2), coef=poisoned(c.to(DEV)), step=step),
                 dict, inplace=("x", "last", "m1", "m2"))
    xs, m1o, m2o = x.float(), m1.float(), m2.float()
    mn = xs - 0.7 * e
    xc = (0.9 * last.float() - 0.3 * m1o) - 0.2 * (0.4 * ((m2o - m1o) / 0.5) + 0.6 * (mn - m1o))
    xn = (0.8 * xc - 0.25 * mn) - 0.15 * (0.5 * ((m1o - mn) / 0.5))
    assert bits_equal(r["m2"], m1)
    for k, want in (("m1", mn), ("last", xc), ("x", xn)):
        assert_close_bf16(r[k], want, f"unipc {k} n{n}", **tol)


@pytest.mark.parametrize("HW", [1, 7, 4097, 4104])
@pytest.mark.parametrize("Bm", [1, 2])
def test_inpaint_blend_in_place_footprint(HW, Bm):
    """In place over latents [B][C][HW]; HW = 4104 takes the 16-byte form, the others the scalar one."""
    ops, L = _ops()
    B, Cc = 2, 4
    lat, x0, noise, mask = rnd((B, Cc, HW), 140), rnd((B, Cc, HW), 141), rnd((B, Cc, HW), 142), (rnd((Bm, 1, HW), 143) > 0).to(bf16)
    coef = torch.tensor([[0.5, 0.5], [0.75, 0.625], [1.0, 0.0]], device=DEV)
    r = run_both(f"inpaint_blend HW{HW} Bm{Bm}", lambda i, o: _check(L, L.load().da_inpaint_blend(_p(i["lat"]), _p(i["x0"]), _p(i["noise"]), _p(i["mask"]),
                                                                                                  _p(i["coef"]), _p(i["step"]), 3, B, Cc, HW, Bm, _stream()), "blend"),
                 dict(lat=poisoned(lat), x0=poisoned(x0), noise=poisoned(noise), mask=poisoned(mask), coef=poisoned(coef),
                      step=poisoned(torch.tensor([1], dtype=torch.int32, device=DEV))), dict, inplace=("lat",))["lat"]
    m = mask.float()
    assert_close_bf16(r, (1 - m) * (0.75 * x0.float() + 0.625 * noise.float()) + m * lat.float(), f"inpaint_blend HW{HW}")


@pytest.mark.parametrize("dt", [bf16, f32])
@pytest.mark.parametrize("n", [2, 7, 4097])
def test_cfg_rescale_footprint(n, dt):
    """n_per = 1 is refused (a standard deviation of one element): 2 is the nearest accepted.  The scratch ratio_ws is guarded."""
    ops, L = _ops()
    B, gd, gr = 2, 5.0, 0.7
    eps = rnd((2, B, n), 150, dtype=dt)
    code = L.DTYPE_F32 if dt == f32 else L.DTYPE_BF16
    r = run_both(f"cfg_rescale n{n}", lambda i, o: _check(L, L.load().da_cfg_rescale(_p(i["eps"]), _p(o["y"]), _p(o["ws"]), B, n, gd, gr, code, _stream()), "rescale"),
                 dict(eps=poisoned(eps)), lambda: dict(y=guarded((B, n), dtype=dt), ws=guarded(B, dtype=f32)))["y"]
    u, c = eps[0].float(), eps[1].float()
    cfg = u + gd * (c - u)
    want = gr * (cfg * (c.std(dim=1, keepdim=True) / cfg.std(dim=1, keepdim=True))) + (1 - gr) * cfg
    assert_close_bf16(r, want, f"cfg_rescale n{n} {dt}")


@pytest.mark.parametrize("HW", [1, 7, 4097])
def test_vae_posterior_latents_footprint(HW):
    """MOMENTS with quant_conv from the channel-padded NHWC layout (sC = 1, sP = 16), and NOISE (add_noise alone) from NCHW."""
    ops, L = _ops()
    lib, B, Lc = L.load(), 2, 4
    x16 = rnd((B, HW, 16), 160)
    wq, bq = rnd((8, 8), 161, 0.35), rnd((8,), 162, 0.1)
    p = run_both("posterior moments", lambda i, o: _check(L, lib.da_vae_posterior_latents(_p(i["x"]), HW * 16, 1, 16, _p(i["wq"]), _p(i["bq"]), None, None, _p(o["y"]),
                                                                                          B, HW, Lc, L.POSTERIOR_MOMENTS, 0, 0.0, 1.0, 1.0, 0.0, _stream()), "moments"),
                 dict(x=poisoned(x16), wq=poisoned(wq), bq=poisoned(bq)), lambda: dict(y=guarded((B, 8, HW))))["y"]
    assert_close_bf16(p, (x16[..., :8].float() @ wq.float().t() + bq.float()).permute(0, 2, 1), f"posterior moments HW{HW}")
    z, eps2 = rnd((B, Lc, HW), 163), rnd((B, Lc, HW), 164)
    y = run_both("posterior noise", lambda i, o: _check(L, lib.da_vae_posterior_latents(_p(i["x"]), Lc * HW, HW, 1, None, None, None, _p(i["eps2"]), _p(o["y"]),
                                                                                        B, HW, Lc, L.POSTERIOR_NOISE, 0, 0.0, 1.0, 0.75, 0.625, _stream()), "noise"),
                 dict(x=poisoned(z), eps2=poisoned(eps2)), lambda: dict(y=guarded((B, Lc, HW))))["y"]
    assert bits_equal(y, ((0.75 * z.float()).to(bf16).float() + (0.625 * eps2.float()).to(bf16).float()).to(bf16))
