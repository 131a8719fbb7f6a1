"""Every entry point of the launch plan (DA_FN_*, include/diffusers_amd.h) replayed and relocated ON ITS OWN.

The pipeline-sized plan tests (tests/test_plan_gpu.py) replay whole steps of tiny models: most ints fit a few bits, neighbouring
arguments are often equal, and several entry points and parameter-struct fields are never part of such a step.  Here each case is ONE
small launch (or a producer / consumer pair) through its diffusers_amd.ops wrapper, with arguments that discriminate -- pairwise
different dimensions, leading dimensions above the row length, element counts off the vector width, non-zero modes, non-integer
floats -- and goes through the same three stages:

  1. eager: outputs pre-filled with a sentinel where the wrapper takes them, run once, finite, nothing of the sentinel left where the
     op is defined to write.  The eager launch IS the reference: a replay is the same launch, so every comparison is bit for bit.
  2. replay: inputs restored, outputs poisoned, the op recorded (strict) and `launch()`ed twice from restored inputs -- the second
     launch is what a kernel that does not re-arm its own state fails (split-K flags, attention ticket counters, step counters).
  3. relocated replay: `Plan.save`, `create_from_file(new_bases=...)` onto fresh copies of the regions, then the case's ORIGINAL
     buffers are overwritten (floats NaN, counters 0) before the relocated plan runs: the expected bytes must appear in the new
     buffers and not one byte of the originals may change.  An address that was not relocated reads NaN or writes the old buffer.

Two coverage conditions keep the file from quietly leaving something out: the entry points recorded over all cases are exactly
FN_IDS, and the non-NULL pointer fields of the recorded da_gemm_params / da_attention_params cover every pointer field of the structs.
"""
import contextlib
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
DEV = "cuda"
SAMPLE = (2, 3, 17, 29)                    # the flat (sampler / cast) kernels: 2958 elements, not a multiple of 8
ATTN_SPLIT_CASE = (2, 8, 64, 1280, 700)    # (B, H, D, Sq, Skv): the smallest key-split launch of tests/test_attention_split.py


def rnd(shape, seed, scale=1.0, dtype=bf16):
    g = torch.Generator("cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def blank(shape, dtype=bf16):
    """An output (or scratch) buffer; `restore` fills it with the sentinel before every launch."""
    return torch.empty(shape, device=DEV, dtype=dtype)


def poison_(t):
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(0xA5)
    else:
        t.zero_()
    return t


def bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def step_counter(v=2):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def euler_table():
    """[steps][8] rows of the Euler / Euler-ancestral layout: sigma, sigma_next, dt, sqrt(sigma^2+1), c_out, sigma^2+1, sigma_up, t"""
    rows = []
    for s, sn, t in ((14.61, 7.32, 999.0), (7.32, 2.91, 701.5), (2.91, 0.87, 400.25), (0.87, 0.03, 101.75)):
        rows.append([s, sn, sn - s, (s * s + 1) ** 0.5, -s / (s * s + 1) ** 0.5, s * s + 1, 0.37 * sn, t])
    return torch.tensor(rows, dtype=f32, device=DEV)


# ---- the cases: name -> builder() -> (bufs, run) ---------------------------------------------------------------------------------
# bufs: every device tensor the launch touches that the case allocates itself.  Key prefix "out" / "ws": written by the launch
# (sentinel-filled before every launch); "io": read AND written (restored from its initial contents); anything else: read only.
# run(bufs) -> outputs: contiguous tensors, or (buffer, index) where only buffer[index] is defined to be written.
CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


@case
def gemm_epilogue():
    from diffusers_amd import _lib as L, ops
    M, N, K = 520, 132, 64
    b = dict(x=rnd((M, K + 8), 1), w=rnd((N, K), 2, K ** -0.5), bias=rnd((N,), 3), res=rnd((M, N + 4), 4), out=blank((M, N + 4)))

    def run(b):
        ops.linear(b["x"][:, :K], b["w"], b["bias"], residual=b["res"][:, :N], act=L.ACT_SILU, alpha=0.75, out_scale=1.5,
                   out=b["out"][:, :N], tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
        return [(b["out"], (slice(None), slice(0, N)))]
    return b, run


@case
def gemm_split_k():
    from diffusers_amd import _lib as L, ops
    M, N, K = 300, 320, 1024
    b = dict(x=rnd((M, K), 31), w=rnd((N, K), 32, K ** -0.5), bias=rnd((N,), 33), res=rnd((M, N), 34), out=blank((M, N)))

    def run(b):
        ops.linear(b["x"], b["w"], b["bias"], residual=b["res"], out=b["out"], tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT, split_k=4)
        return [b["out"]]
    return b, run


@case
def gemm_layernorm_fold():
    """producer (stats_out) and consumer (ln_stats / ln_s / ln_c) of a folded LayerNorm, two launches of one plan"""
    from diffusers_amd import _lib as L, ops
    M, Cc, N = 520, 320, 384
    gamma, beta = rnd((Cc,), 64) * 0.3 + 1.0, rnd((Cc,), 65) * 0.2
    wl, fold = ops.fold_layernorm(rnd((N, Cc), 66, Cc ** -0.5), gamma, beta, 1e-5)
    st = ops.RowStats(M, DEV)
    b = dict(a=rnd((M, 192), 61), wprod=rnd((Cc, 192), 62, 192 ** -0.5), res=rnd((M, Cc), 63), wl=wl, s=fold.s, c=fold.c,
             bias=rnd((N,), 67), ws_stats=st.buf, out_x=blank((M, Cc)), out_y=blank((M, N)))

    def run(b):
        ops.linear(b["a"], b["wprod"], residual=b["res"], out=b["out_x"], tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT, stats_out=st)
        ops.linear(b["out_x"], b["wl"], b["bias"], out=b["out_y"], tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT, ln=(st, fold))
        return [b["out_x"], b["out_y"]]
    return b, run


@case
def gemm_fused_qkv():
    """the transposed V block (vt) of the fused Q | K | V projection, with a prefetch hint"""
    from diffusers_amd import _lib as L, ops
    M, Cc, inner = 520, 320, 320
    b = dict(x=rnd((M, Cc), 71), wqkv=rnd((3 * inner, Cc), 76, Cc ** -0.5), bias=rnd((3 * inner,), 77), nxt=rnd((128, 256), 78),
             out_qk=blank((M, 2 * inner)), out_vt=blank((inner, M + 8)))

    def run(b):
        ops.linear(b["x"], b["wqkv"], b["bias"], out=b["out_qk"], tile=L.TILE_K2_128x80, staging=L.STAGE_PINGPONG,
                   vt_out=(b["out_vt"], 2 * inner), prefetch=b["nxt"])
        return [b["out_qk"], (b["out_vt"], (slice(None), slice(0, M)))]
    return b, run


@case
def gemm_cross_attention_epilogue():
    from diffusers_amd import _lib as L, layers, ops
    B, seq, Cc, heads, cross, skv = 1, 128, 128, 2, 64, 77
    inner = heads * 64
    pad, s, sa = layers.pad_encoder_states(rnd((B, skv, cross), 8))
    k = ops.linear(pad, rnd((inner, cross), 3, cross ** -0.5), tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
    vt = ops.linear(rnd((inner, cross), 4, cross ** -0.5), pad, tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
    b = dict(x=rnd((B * seq, Cc), 1), wq=rnd((inner, Cc), 2, Cc ** -0.5), bq=rnd((inner,), 91), k=k, vt=vt, out=blank((B * seq, inner)))

    def run(b):
        xa = {"k": b["k"], "vt": b["vt"], "skv": s, "skv_alloc": sa, "seq": seq, "scale": 0.1171875}
        ops.linear(b["x"], b["wq"], b["bq"], out=b["out"], xattn=xa, tile=L.TILE_K2_128x128, staging=L.STAGE_PINGPONG)
        return [b["out"]]
    return b, run


@case
def conv_concat_rowvec_residual():
    from diffusers_amd import _lib as L, ops
    B, H, W, C1, C2, Co = 2, 8, 8, 128, 64, 192
    b = dict(x1=rnd((B, H, W, C1), 23), x2=rnd((B, H, W, C2), 24), w=rnd((Co, 9 * (C1 + C2)), 25, (9 * (C1 + C2)) ** -0.5),
             bias=rnd((Co,), 26, 0.1), tv=rnd((B, Co), 27), res=rnd((B, H, W, Co), 28), out=blank((B, H, W, Co)))

    def run(b):
        ops.conv2d_nhwc(b["x1"], b["w"], b["bias"], ksize=3, x2=b["x2"], rowvec=b["tv"], residual=b["res"], out_scale=0.5,
                        out=b["out"], tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
        return [b["out"]]
    return b, run


@case
def gemm_gate_and_row_bias():
    from diffusers_amd import _lib as L, ops
    M, N, K, B = 640, 384, 256, 2
    b = dict(x=rnd((M, K), 61), w=rnd((N, K), 62, K ** -0.5), bias=rnd((N,), 63), res=rnd((M, N), 64), gate=rnd((B, 3 * N), 65),
             bm=rnd((M,), 66), out_y=blank((M, N)), out_wide=blank((M, 2 * N)))

    def run(b):
        ops.linear(b["x"], b["w"], b["bias"], gate=b["gate"][:, N:2 * N], rows_per_batch=M // B, residual=b["res"], out=b["out_y"],
                   tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
        ops.linear(b["x"], b["w"], bias_rows=b["bm"], out=b["out_wide"][:, N:], tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
        return [b["out_y"], (b["out_wide"], (slice(None), slice(N, 2 * N)))]
    return b, run


@case
def gemm_pair():
    """da_gemm_pair_bf16 through ops.linear_pair: the per-shape table is given the paired entry (and slower separate ones), as the
    tuner would have left it"""
    from diffusers_amd import _lib as L, ops, tuning
    M, K, Nq = 520, 192, 260
    b = dict(x=rnd((M, K), 21), wqk=rnd((Nq, K), 22, K ** -0.5), wv=rnd((Nq // 2, K), 23, K ** -0.5), bias=rnd((Nq,), 24))
    pa, _ = ops._linear_params(b["x"], b["wqk"], b["bias"], tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
    pb, _ = ops._linear_params(b["wv"], b["x"], tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT)
    table = {tuning.pair_key(pa, pb): (L.TILE_128x128, L.STAGE_LDS_DIRECT, 1.0, 1),
             tuning.key_of(pa): (L.TILE_128x128, L.STAGE_LDS_DIRECT, 100.0, 1), tuning.key_of(pb): (L.TILE_128x128, L.STAGE_LDS_DIRECT, 100.0, 1)}

    def run(b):
        keep = (ops.TUNING, tuning._table, tuning._loaded)
        ops.TUNING, tuning._table, tuning._loaded = True, dict(table), True
        try:
            qk, vt = ops.linear_pair({"x": b["x"], "w": b["wqk"], "bias": b["bias"]}, {"x": b["wv"], "w": b["x"]})
        finally:
            ops.TUNING, tuning._table, tuning._loaded = keep
        return [qk, vt]
    return b, run


def _attention_operands(B, H, D, Sq, Skv, seed):
    inner = H * D
    sa = (Skv + 15) // 16 * 16
    kp = torch.zeros((B, sa, inner), device=DEV, dtype=bf16)
    kp[:, :Skv] = rnd((B, Skv, inner), seed + 1, 0.7)
    vt = torch.zeros((inner, B * sa), device=DEV, dtype=bf16)
    vt.view(inner, B, sa)[:, :, :Skv] = rnd((B, Skv, inner), seed + 2).permute(2, 0, 1)
    return rnd((B * Sq, inner), seed, 0.7), kp.view(B * sa, inner), vt, sa, inner


@case
def attention_bias():
    """the masked variant with a bias shared by the batches, rows of a wider buffer"""
    from diffusers_amd import ops
    B, H, D, Sq, Skv = 2, 2, 64, 130, 77
    q, kp, vt, sa, inner = _attention_operands(B, H, D, Sq, Skv, 70)
    b = dict(q=q, k=kp, vt=vt, bias=rnd((1, H, Sq, 192), 75, 0.5, f32), out=blank((B * Sq, inner + 8)))

    def run(b):
        ops.attention(b["q"], b["k"], b["vt"], B=B, H=H, D=D, Sq=Sq, Skv=Skv, Skv_alloc=sa, q_row_stride=inner, k_row_stride=inner,
                      q_batch_stride=Sq * inner, k_batch_stride=sa * inner, vt_ld=B * sa, vt_batch_stride=sa, scale=0.1171875,
                      bias=b["bias"][..., :128], out=b["out"][:, :inner])
        return [(b["out"], (slice(None), slice(0, inner)))]
    return b, run


def _split_plan(B, H, D, Sq, Skv):
    from diffusers_amd import _lib as L
    p = L.AttentionParams()
    p.B, p.H, p.Sq, p.Skv, p.Skv_alloc, p.D = B, H, Sq, Skv, (Skv + 7) // 8 * 8, D
    full, tail, s = C.c_int(), C.c_int(), C.c_int()
    need = L.load().da_attention_split_plan(C.byref(p), C.byref(full), C.byref(tail), C.byref(s))
    return int(need), s.value


@case
def attention_key_split():
    """split_ws: the key-split tail; its operands are the one exception to "well under 1 MiB" (the wrapper hands the workspace
    only to launches of 64 query blocks and more)"""
    from diffusers_amd import ops
    B, H, D, Sq, Skv = ATTN_SPLIT_CASE
    assert _split_plan(B, H, D, Sq, Skv)[1] > 1, "the case is meant to split"
    q, kp, vt, sa, inner = _attention_operands(B, H, D, Sq, Skv, 80)
    b = dict(q=q, k=kp, vt=vt, out=blank((B * Sq, inner)))

    def run(b):
        ops.attention(b["q"], b["k"], b["vt"], B=B, H=H, D=D, Sq=Sq, Skv=Skv, Skv_alloc=sa, q_row_stride=inner, k_row_stride=inner,
                      q_batch_stride=Sq * inner, k_batch_stride=sa * inner, vt_ld=B * sa, vt_batch_stride=sa, out=b["out"])
        return [b["out"]]
    return b, run


@case
def groupnorm_two_sources():
    from diffusers_amd import ops
    B, HW, C1, C2 = 2, 144, 640, 320
    b = dict(x1=rnd((B, HW, C1), 43), x2=rnd((B, HW, C2), 44, 3.0), g=rnd((C1 + C2,), 45) * 0.1 + 1.0, b=rnd((C1 + C2,), 46, 0.1))
    return b, lambda b: [ops.group_norm_nhwc(b["x1"], b["g"], b["b"], 32, 1.5e-5, silu=True, x2=b["x2"])]


@case
def rmsnorm_t5():
    from diffusers_amd import ops
    b = dict(x=rnd((77, 136), 76, 3.0), g=rnd((128,), 77) * 0.2 + 1.0)
    return b, lambda b: [ops.rms_norm(b["x"][:, :128], b["g"], 1.5e-6)]


@case
def layernorm_modulated():
    from diffusers_amd import ops
    M, Cc = 100, 320
    b = dict(x=rnd((M, Cc + 16), 47, 1.5), g=rnd((Cc,), 48) * 0.1 + 1.0, b=rnd((Cc,), 49, 0.1), mod=rnd((2, 3 * Cc), 50, 0.3))
    return b, lambda b: [ops.layer_norm(b["x"][:, :Cc], b["g"], b["b"], 1.5e-6, mod_scale=b["mod"][:, Cc:2 * Cc],
                                        mod_shift=b["mod"][:, :Cc], rows_per_batch=M // 2)]


@case
def rmsnorm_rope():
    from diffusers_amd import ops
    rows, St, heads, D = 80, 16, 2, 64
    Cc = heads * D
    ang = torch.rand((rows, D // 2), generator=torch.Generator("cpu").manual_seed(74)) * 6.0
    b = dict(io_x=rnd((rows, 3 * Cc), 71), wq=rnd((D,), 72, 0.2) + 1, wk=rnd((D,), 73, 0.2) + 1,
             cos=ang.cos().repeat_interleave(2, 1).contiguous().to(DEV), sin=ang.sin().repeat_interleave(2, 1).contiguous().to(DEV))

    def run(b):
        ops.rmsnorm_rope_(b["io_x"][St:], heads=heads, head_dim=D, col_offsets=(0, Cc), weights=(b["wq"], b["wk"]), eps=1.5e-6,
                          cos=b["cos"], sin=b["sin"], rope_row0=St)
        return [b["io_x"]]
    return b, run


@case
def softmax_rows():
    from diffusers_amd import ops
    M, N = 37, 77
    b = dict(s=rnd((M, 80), 52, 3.0, f32), out=blank((M, 96)))

    def run(b):
        ops.softmax_rows(b["s"][:, :N], out=b["out"][:, :N])
        return [(b["out"], (slice(None), slice(0, N)))]
    return b, run


@case
def rmsnorm_channels():
    from diffusers_amd import ops
    b = dict(x=rnd((5, 10, 96), 81), g=rnd((96,), 82) * 0.2 + 1.0)
    return b, lambda b: [ops.rmsnorm_channels(b["x"], b["g"], real_channels=90, silu=True)]


@case
def euler_scale_model_input():
    from diffusers_amd import ops
    b = dict(x=rnd(SAMPLE, 1), table=euler_table(), step=step_counter())
    return b, lambda b: [ops.euler_scale_model_input(b["x"], b["table"], b["step"], rep=2)]


@case
def euler_step():
    from diffusers_amd import _lib as L, ops
    b = dict(eps=rnd((2 * SAMPLE[0],) + SAMPLE[1:], 2), x=rnd(SAMPLE, 1, 3.0), table=euler_table(), step=step_counter(), out=blank(SAMPLE))
    return b, lambda b: [ops.euler_step(b["eps"], b["x"], b["table"], b["step"], cfg=True, guidance=5.5, out=b["out"], pred_type=L.PRED_V)]


@case
def euler_ancestral_step():
    from diffusers_amd import _lib as L, ops
    n = rnd(SAMPLE, 0).numel()
    b = dict(eps=rnd((2 * SAMPLE[0],) + SAMPLE[1:], 2), x=rnd(SAMPLE, 1, 3.0), noise=rnd((4, n + 6), 3), table=euler_table(),
             step=step_counter(), out=blank(SAMPLE))
    return b, lambda b: [ops.euler_ancestral_step(b["eps"], b["x"], b["noise"], b["table"], b["step"], cfg=True, guidance=5.5, out=b["out"],
                                                  pred_type=L.PRED_V, noise_step_stride=n + 6)]


@case
def x0_linear_step():
    from diffusers_amd import _lib as L, ops
    n = rnd(SAMPLE, 0).numel()
    rows = [[0.14, 0.99, 0.31, 0.27, 0.83, 0.19, 1.25, 999.0 - 250 * i] for i in range(4)]
    b = dict(eps=rnd((2 * SAMPLE[0],) + SAMPLE[1:], 2, 1.0, f32), x=rnd(SAMPLE, 1, 1.0, f32), noise=rnd((4, n), 3, 1.0, f32),
             table=torch.tensor(rows, dtype=f32, device=DEV), step=step_counter(), out=blank(SAMPLE, f32))
    return b, lambda b: [ops.x0_linear_step(b["eps"], b["x"], b["noise"], b["table"], b["step"], cfg=True, guidance=5.5, out=b["out"],
                                            noise_step_stride=n, pred_type=L.PRED_SAMPLE)]


@case
def flowmatch_step():
    from diffusers_amd import ops
    rows = [[1.0 - 0.2 * i, 0.8 - 0.2 * i, -0.2, 0, 0, 0, 0, 1000.0 - 200 * i] for i in range(4)]
    b = dict(v=rnd((2 * SAMPLE[0],) + SAMPLE[1:], 2), x=rnd(SAMPLE, 1, 1.0, f32), table=torch.tensor(rows, dtype=f32, device=DEV),
             step=step_counter(), out=blank(SAMPLE))
    return b, lambda b: [ops.flowmatch_step(b["v"], b["x"], b["table"], b["step"], cfg=True, guidance=4.5, out=b["out"])]


@case
def unipc_flow_step():
    from diffusers_amd import ops
    rows = [[0.9 - 0.2 * i, 1.0, 2.0, 0.61, 0.43, 0.27, 0.55, 0.31, 0.47, 2.0, 0.59, 0.41, 0.23, 0.53, 0.0, 0.0] for i in range(4)]
    b = dict(v=rnd((2 * SAMPLE[0],) + SAMPLE[1:], 2), io_x=rnd(SAMPLE, 1, 1.0, f32), io_last=rnd(SAMPLE, 4, 1.0, f32),
             io_m1=rnd(SAMPLE, 5, 1.0, f32), io_m2=rnd(SAMPLE, 6, 1.0, f32), coef=torch.tensor(rows, dtype=f32, device=DEV), step=step_counter())

    def run(b):
        ops.unipc_flow_step_(b["v"], b["io_x"], b["io_last"], b["io_m1"], b["io_m2"], b["coef"], b["step"], cfg=True, guidance=4.5)
        return [b["io_x"], b["io_last"], b["io_m1"], b["io_m2"]]
    return b, run


@case
def dpmpp_2m_step():
    from diffusers_amd import _lib as L, ops
    rows = [[0.6 + 0.1 * i, 0.8 - 0.1 * i, 0.71, 0.33, 0.17, 0.0, 1.0, 999.0 - 250 * i] for i in range(4)]
    b = dict(eps=rnd((2 * SAMPLE[0],) + SAMPLE[1:], 2, 1.0, f32), io_x=rnd(SAMPLE, 1, 3.0), io_m1=rnd(SAMPLE, 5, 1.0, f32),
             table=torch.tensor(rows, dtype=f32, device=DEV), step=step_counter(), begin=step_counter(1))

    def run(b):
        ops.dpmpp_2m_step_(b["eps"], b["io_x"], b["io_m1"], b["table"], b["step"], b["begin"], cfg=True, guidance=5.5, pred_type=L.PRED_V)
        return [b["io_x"], b["io_m1"]]
    return b, run


@case
def advance_step():
    from diffusers_amd import ops
    b = dict(io_step=step_counter(5))

    def run(b):
        ops.advance_step(b["io_step"])
        return [b["io_step"]]
    return b, run


@case
def cfg_rescale():
    from diffusers_amd import ops
    b = dict(eps=rnd((2 * SAMPLE[0],) + SAMPLE[1:], 2), out=blank(SAMPLE))
    return b, lambda b: [ops.cfg_rescale(b["eps"], 5.5, 0.7, out=b["out"])]


@case
def cast_f32_bf16():
    from diffusers_amd import ops
    b = dict(x=rnd(SAMPLE, 1, 1.0, f32))
    return b, lambda b: [ops.cast_f32_bf16(b["x"], rep=2)]


@case
def mul_scalar():
    from diffusers_amd import ops
    b = dict(x=rnd(SAMPLE, 1, 1.0, f32))
    return b, lambda b: [ops.mul_scalar(b["x"], 0.8125, rep=2)]


@case
def bcast_add_f32():
    from diffusers_amd import ops
    b = dict(a=rnd((1001,), 1, 1.0, f32), m=rnd((3, 1001), 2))
    return b, lambda b: [ops.bcast_add_f32(b["a"], b["m"])]


@case
def patchify3d():
    from diffusers_amd import ops
    b = dict(x=rnd((2, 16, 3, 8, 6), 101))
    return b, lambda b: [ops.patchify3d(b["x"], (1, 2, 2))]


@case
def unpatchify3d():
    from diffusers_amd import ops
    B, Cc, Fr, H, W = 2, 16, 3, 8, 6
    b = dict(tok=rnd((B * Fr * (H // 2) * (W // 2), 4 * Cc), 103))
    return b, lambda b: [ops.unpatchify3d(b["tok"], (B, Cc, Fr, H, W), (1, 2, 2))]


@case
def transpose():
    from diffusers_amd import ops
    R, Cc = 37, 50
    b = dict(x=rnd((R, 56), 1), out=blank((Cc, 40)))

    def run(b):
        ops.transpose(b["x"][:, :Cc], out=b["out"][:, :R])
        return [(b["out"], (slice(None), slice(0, R)))]
    return b, run


@case
def conv_out_take_nchw():
    """a thin-output conv on the implicit-GEMM path: da_gemm_bf16 (conv) + da_nhwc_take_nchw_bf16"""
    from diffusers_amd import ops
    b = dict(x=rnd((1, 64, 64, 64), 71), w=rnd((3, 9 * 64), 72, (9 * 64) ** -0.5), bias=rnd((3,), 73, 0.1))
    return b, lambda b: [ops.conv_thin_out(b["x"], b["w"], b["bias"])]


@case
def conv_out_take_postprocess():
    from diffusers_amd import ops
    b = dict(x=rnd((1, 64, 64, 64), 71), w=rnd((3, 9 * 64), 74, (9 * 64) ** -0.5), bias=rnd((3,), 75, 0.1))
    return b, lambda b: [ops.conv_thin_out(b["x"], b["w"], b["bias"], postprocess="uint8")]


@case
def permute_0213():
    from diffusers_amd import ops
    b = dict(x=rnd((3, 5, 7, 8), 41), out=blank((3, 7, 5, 8)))
    return b, lambda b: [ops.permute_0213(b["x"], out=b["out"])]


@case
def image_postprocess():
    from diffusers_amd import ops
    b = dict(img=rnd(SAMPLE, 1, 1.0, f32))
    return b, lambda b: [ops.image_postprocess(b["img"], "np")]


@case
def frames_to_ncthw():
    from diffusers_amd import ops
    b = dict(f=rnd((2 * 3, 5, 7, 8), 42, 0.8))
    return b, lambda b: [ops.frames_to_ncthw(b["f"], batch=2, channels=3, lo=-0.75, hi=0.5, out_f32=True)]


@case
def timestep_embedding():
    from diffusers_amd import ops
    b = dict(table=euler_table(), step=step_counter())
    return b, lambda b: [ops.timestep_embedding(None, 132, batch=3, flip_sin_to_cos=True, shift=0.25, scale=1.5, max_period=9999.5,
                                                table=b["table"], step_idx=b["step"], out_f32=True)]


@case
def linear_small_m():
    from diffusers_amd import _lib as L, ops
    M, N, K = 3, 132, 64
    b = dict(x=rnd((M, K + 8), 60), w=rnd((N, K), 61, K ** -0.5), bias=rnd((N,), 62, 0.1), res=rnd((M, N + 4), 63), out=blank((M, N + 12)))

    def run(b):
        ops.linear_small_m(b["x"][:, :K], b["w"], b["bias"], act_in=L.ACT_SILU, act_out=L.ACT_GELU_TANH, residual=b["res"][:, :N],
                           out=b["out"][:, :N])
        return [(b["out"], (slice(None), slice(0, N)))]
    return b, run


@case
def conv_thin_in():
    from diffusers_amd import ops
    b = dict(x=rnd((2, 4, 9, 11), 90), w=rnd((16, 36), 91, 0.2), bias=rnd((16,), 92))
    return b, lambda b: [ops.conv_thin_in(b["x"], b["w"], b["bias"], ksize=3, in_nchw=True, in_div=0.3611, in_add=0.1159)]


@case
def conv_thin_out():
    from diffusers_amd import ops
    b = dict(x=rnd((2, 9, 11, 128), 68), w=rnd((4, 9 * 128), 69, (9 * 128) ** -0.5), bias=rnd((4,), 70, 0.1))
    return b, lambda b: [ops.conv_thin_out(b["x"], b["w"], b["bias"], out_f32=True)]


@case
def inpaint_blend():
    from diffusers_amd import ops
    coef = torch.tensor([[0.25, 0.96875], [0.5, 0.8671875], [0.75, 0.66015625], [1.0, 0.0]], dtype=f32, device=DEV)
    b = dict(io_lat=rnd((2, 4, 9, 11), 1), x0=rnd((2, 4, 9, 11), 2), noise=rnd((2, 4, 9, 11), 3), mask=rnd((1, 1, 9, 11), 4).sigmoid(),
             coef=coef, step=step_counter())

    def run(b):
        ops.inpaint_blend_(b["io_lat"], b["x0"], b["noise"], b["mask"], b["coef"], b["step"])
        return [b["io_lat"]]
    return b, run


@case
def conv_in_inpaint():
    from diffusers_amd import ops
    b = dict(x=rnd((2, 4, 9, 11), 1), mask=rnd((2, 1, 9, 11), 2).sigmoid(), masked=rnd((2, 4, 9, 11), 3), w=rnd((16, 81), 4, 0.2),
             bias=rnd((16,), 5), table=euler_table(), step=step_counter())
    return b, lambda b: [ops.conv_in_inpaint(b["x"], b["mask"], b["masked"], b["w"], b["bias"], table=b["table"], step_idx=b["step"], rep=2)]


# ---- the three stages ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _case_environment():
    """Pinned variants instead of the tuner (a case is ONE launch), and split-K / key-split workspaces of the size the cases need
    instead of the 64 / 128 MiB ones of a whole model, so that a saved plan stays small.  Everything is put back afterwards."""
    from diffusers_amd import ops
    saved = (ops.TUNING, ops._splitk_ws, ops._attn_split_ws, ops.SPLITK_WS_BYTES, ops.ATTN_SPLIT_WS_BYTES)
    need = _split_plan(*ATTN_SPLIT_CASE)[0]
    ops.TUNING, ops._splitk_ws, ops._attn_split_ws = False, {}, {}
    ops.SPLITK_WS_BYTES, ops.ATTN_SPLIT_WS_BYTES = 4 << 20, (need + (1 << 20) - 1) >> 20 << 20
    try:
        yield
    finally:
        ops.TUNING, ops._splitk_ws, ops._attn_split_ws, ops.SPLITK_WS_BYTES, ops.ATTN_SPLIT_WS_BYTES = saved


def _split(outs):
    """[(buffer, index or None)] of what `run` returned"""
    return [(o if isinstance(o, tuple) else (o, None)) for o in outs]


def _defined(buf, idx):
    return buf if idx is None else buf[idx]


def _check_outputs(outs, what):
    for buf, idx in outs:
        d = _defined(buf, idx)
        if d.dtype.is_floating_point:
            assert torch.isfinite(d.float()).all(), f"{what}: not finite / sentinel left where the op writes"
        if idx is not None:                      # the rest of the buffer is not the op's to write
            rest = buf.clone()
            poison_(rest[idx])
            assert torch.isnan(rest.float()).all(), f"{what}: written outside the defined region"


@functools.lru_cache(maxsize=None)
def run_case(name, tmp):
    """All three stages of one case; returns what the coverage conditions need: (entry points recorded, {struct: non-NULL pointer
    fields})."""
    from diffusers_amd import _lib as L, ops, plan as P
    lib = L.load()
    with _case_environment():
        bufs, run = CASES[name]()
        init = {k: v.clone() for k, v in bufs.items() if k.startswith("io")}

        def restore(extra=()):
            for k, v in bufs.items():
                if k.startswith("io"):
                    v.copy_(init[k])
                elif k.startswith(("out", "ws")):
                    poison_(v)
            for t in extra:
                poison_(t)
            torch.cuda.synchronize()
        own = {v.data_ptr() for v in bufs.values()}
        # 1. eager
        restore()
        eager = _split(run(bufs))
        torch.cuda.synchronize()
        _check_outputs(eager, f"{name} (eager)")
        ref = [buf.clone() for buf, _ in eager]
        del eager
        # 2. replay
        restore()
        pl, outs = P.record(lambda: run(bufs), keep=list(bufs.values()))
        outs = _split(outs)
        torch.cuda.synchronize()
        assert pl.foreign_ops == [] and len(pl) == len(pl.names) >= 1
        fresh = [buf for buf, _ in outs if buf.data_ptr() not in own]          # allocated by the wrapper, inside the recording
        for (buf, _), want in zip(outs, ref):
            assert same_bits(buf, want), f"{name}: the recorded (eager) run differs from the first eager run"
        for n in (1, 2):
            restore(fresh)
            pl.launch()
            torch.cuda.synchronize()
            _check_outputs(outs, f"{name} (replay {n})")
            for i, ((buf, _), want) in enumerate(zip(outs, ref)):
                assert same_bits(buf, want), f"{name}: output {i} of replay {n} differs from the eager launch"
        assert not ops.splitk_error()
        # 3. relocated replay
        restore(fresh)
        path = f"{tmp}/{name}.daplan"
        info = pl.save(path, outputs=[buf for buf, _ in outs])
        doc = P.read_file(path)
        for (ptr, want), r in zip(doc["outputs"], ref):
            assert want == bits(r).cpu().numpy().tobytes(), f"{name}: the launch inside save() differs from the eager launch"
        new = [torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() for _, _, data in doc["regions"]]
        h, _ = P.create_from_file(path, new_bases=[t.data_ptr() for t in new])
        try:
            originals = list(bufs.values()) + fresh
            for t in originals:                  # floats NaN, bytes 0xA5, counters 0 (a counter must stay a valid table row)
                poison_(t)
            torch.cuda.synchronize()
            before = [bits(t).clone() for t in originals]
            failed = C.c_int(-1)
            L.check(lib.da_plan_launch(h, torch.cuda.current_stream().cuda_stream, C.byref(failed)), f"da_plan_launch (op {failed.value})")
            torch.cuda.synchronize()
        finally:
            lib.da_plan_destroy(h)
        for i, (ptr, want) in enumerate(doc["outputs"]):
            r = next(j for j, (base, n, _) in enumerate(doc["regions"]) if base <= ptr < base + n)
            off = ptr - doc["regions"][r][0]
            got = new[r][off:off + len(want)].cpu().numpy().tobytes()
            assert got == want, f"{name}: output {i} of the relocated replay differs from the eager launch"
        for t, was in zip(originals, before):
            assert torch.equal(bits(t), was), f"{name}: the relocated plan wrote into (or through) a buffer of the recording process"
        fields = {}
        for obj in pl._host:
            if isinstance(obj, (L.GemmParams, L.AttentionParams)):
                fields.setdefault(type(obj).__name__, set()).update(f for f, t in obj._fields_ if t is C.c_void_p and getattr(obj, f))
        print(f"[plan] {name}: {pl.names} replayed twice and relocated ({info['regions']} regions, {info['file_bytes'] >> 10} KiB)")
        return tuple(pl.names), {k: frozenset(v) for k, v in fields.items()}


@pytest.fixture(scope="module")
def plan_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("plans"))


@pytest.mark.parametrize("name", list(CASES))
def test_entry_point_replays_and_relocates_bit_identically(name, plan_dir):
    run_case(name, plan_dir)


def test_every_entry_point_and_every_pointer_field_is_covered(plan_dir):
    from diffusers_amd import _lib as L
    names, fields = set(), {"GemmParams": set(), "AttentionParams": set()}
    for name in CASES:
        n, f = run_case(name, plan_dir)
        names |= set(n)
        for k, v in f.items():
            fields[k] |= v
    assert names == set(L.FN_IDS), f"never replayed: {sorted(set(L.FN_IDS) - names)}"
    for mirror in (L.GemmParams, L.AttentionParams):
        want = {f for f, t in mirror._fields_ if t is C.c_void_p}
        assert fields[mirror.__name__] == want, f"{mirror.__name__}: never non-NULL in a replayed launch: {sorted(want - fields[mirror.__name__])}"


# ---- a launch the plan cannot replay ---------------------------------------------------------------------------------------------
def test_flux_prepare_latents_under_a_recording_is_reported_not_dropped():
    from diffusers_amd import _lib as L, ops, plan as P
    B, Lc, H, W = 2, 16, 6, 10
    lat, noise = rnd((B, Lc, H, W), 172), rnd((B, Lc, H, W), 171)

    def prepare():
        return ops.flux_prepare_latents(lat, (Lc * H * W, H * W, 1), batch=B, height=H, width=W, latent_channels=Lc,
                                        mode=L.POSTERIOR_NOISE, noise=noise, a=0.75, b=0.625)[0]
    eager = prepare()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="da_flux_prepare_latents"):
        P.record(prepare, strict=True)
    pl, got = P.record(prepare, strict=False)
    torch.cuda.synchronize()
    assert pl.foreign_ops == ["da_flux_prepare_latents"] and pl.names == [] and len(pl) == 0
    assert torch.isfinite(eager.float()).all() and same_bits(got, eager)
