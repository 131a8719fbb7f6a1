"""FP8 (e4m3) linears, csrc/gemm_fp8.hip: the row quantiser to the bit against the header's arithmetic restated in torch, the GEMM
against float64 on the dequantised operands under a bound derived from fp32 accumulation and one bf16 rounding, refusals by name."""
import ctypes as C

import pytest
import torch

import footprint as FP

pytestmark = pytest.mark.gpu

bf16, f8, f32, f64 = torch.bfloat16, torch.float8_e4m3fn, torch.float32, torch.float64
DEV = "cuda"
BF16_MAX = 3.3895313892515355e38


def _gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def quantize_ref(x):
    """The file header's arithmetic, one fp32 operation per step, on the CPU."""
    xf = x.float()
    amax = xf.abs().amax(dim=1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    q = (xf * (1.0 / scale)[:, None]).clamp(-448.0, 448.0).to(f8)
    return q, scale


@pytest.mark.parametrize("K", [128, 384, 3072])
@pytest.mark.parametrize("R", [1, 3, 129])
def test_quantiser_to_the_bit(R, K):
    from diffusers_amd import ops
    x = (torch.randn((R, K), generator=_gen(R * K)) * 3.0).to(bf16)
    x[0, K // 2] = BF16_MAX                     # a row whose amax is the largest finite bf16
    if R > 1:
        x[1] = 0                                # a zero row: scale 1, q 0
    if R > 2:
        x[2] *= 1e-30                           # a tiny row: 1 / scale is huge, the products stay finite
    src = FP.poisoned(x, ld=K + 8)              # strided input, the sentinel between and around the rows
    q, s = ops.quantize_rows_fp8(src.view)
    q_ref, s_ref = quantize_ref(x)
    assert q.dtype == f8 and s.dtype == f32 and q.shape == (R, K) and s.shape == (R,)
    assert FP.bits_equal(s.cpu(), s_ref), (s.cpu() - s_ref).abs().max()
    assert FP.bits_equal(q.cpu(), q_ref), int((q.cpu().view(torch.uint8) != q_ref.view(torch.uint8)).sum())
    src.check("quantiser input")


def _operands(M, N, K, seed, positive=False):
    g = _gen(seed)
    a, b = torch.randn((M, K), generator=g) * 4, torch.randn((N, K), generator=g) * 4
    if positive:
        a, b = a.abs() + 0.5, b.abs() + 0.5
    sa, sb = torch.rand(M, generator=g) * 0.02 + 0.001, torch.rand(N, generator=g) * 0.02 + 0.001
    return a.to(f8), sa, b.to(f8), sb


def _check(out, a8, sa, b8, sb, what, bias=None, bias_rows=None, gelu=False, gate=None, rpb=0, residual=None):
    """float64 reference on the dequantised operands.  Products of two e4m3 values are exact in fp32, so the accumulator is off by at
    most (K - 1) 2^-24 sa sb sum|a b| (any order); the epilogue's at most 6 further fp32 operations each round a value no larger than
    the largest term by 2^-24 (the floor: 8 x 2^-24 x that term); one bf16 rounding: 2^-8 |ref| (twice the half-ulp).  GELU adds the
    allowance tests/test_kernels_gpu.py gives the bf16 kernel's tanh-GELU epilogue: 1.6e-2 |ref| + 8e-3 rms(ref)."""
    M, K = a8.shape
    ad, bd = a8.to(f64), b8.to(f64)
    s2 = sa.to(f64)[:, None] * sb.to(f64)[None, :]
    y = s2 * (ad @ bd.t())
    acc_err = (K - 1) * 2.0 ** -24 * s2 * (ad.abs() @ bd.abs().t())
    big = y.abs().max()
    for t, dim in ((bias, 0), (bias_rows, 1)):
        if t is not None:
            y = y + t.to(f64).unsqueeze(dim)
            big = torch.maximum(big, t.to(f64).abs().max())
    if gelu:
        y = torch.nn.functional.gelu(y, approximate="tanh")     # |gelu'| <= 1.13
        acc_err = acc_err * 1.13
    if gate is not None:
        gd = gate.to(f64)[torch.arange(M) // (rpb or M)]
        y, acc_err, big = y * gd, acc_err * gd.abs(), big * max(1.0, float(gd.abs().max()))
    if residual is not None:
        y = y + residual.to(f64)
        big = torch.maximum(big, residual.to(f64).abs().max())
    tol = acc_err + 2.0 ** -8 * y.abs() + 8 * 2.0 ** -24 * big
    if gelu:
        tol = tol + 1.6e-2 * y.abs() + 8e-3 * y.pow(2).mean().sqrt()
    err = (out.cpu().to(f64) - y).abs()
    worst = float((err / tol).max())
    print(f"[gemm_fp8] {what}: max err / bound = {worst:.3f}, max abs err {float(err.max()):.3e}")
    assert bool(torch.isfinite(out).all()) and worst <= 1.0, (what, worst)


def _cuda(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.mark.parametrize("K", [128, 256, 640])
@pytest.mark.parametrize("N", [16, 48, 257])
@pytest.mark.parametrize("M", [1, 16, 17, 255, 257])
def test_gemm_against_float64(M, N, K):
    from diffusers_amd import _lib as L, ops
    a8, sa, b8, sb = _operands(M, N, K, M * 1000 + N + K)
    g = _gen(7)
    bias, bias_rows = torch.randn(N, generator=g).to(bf16), torch.randn(M, generator=g).to(bf16)
    rpb = max(1, (M + 2) // 3)                                   # three batches, the last one short (a tail batch)
    gate = torch.randn(((M + rpb - 1) // rpb, N), generator=g).to(bf16)
    res = torch.randn((M, N), generator=g).to(bf16)
    A, SA, Bq, SB, bias_d, br_d, gate_d, res_d = _cuda(a8, sa, b8, sb, bias, bias_rows, gate, res)
    _check(ops.linear_fp8(A, SA, Bq, SB), a8, sa, b8, sb, "plain")
    _check(ops.linear_fp8(A, SA, Bq, SB, bias_d), a8, sa, b8, sb, "bias", bias=bias)
    _check(ops.linear_fp8(A, SA, Bq, SB, bias_rows=br_d), a8, sa, b8, sb, "bias_rows", bias_rows=bias_rows)
    _check(ops.linear_fp8(A, SA, Bq, SB, bias_d, act=L.ACT_GELU_TANH), a8, sa, b8, sb, "gelu", bias=bias, gelu=True)
    _check(ops.linear_fp8(A, SA, Bq, SB, bias_d, gate=gate_d, rows_per_batch=rpb, residual=res_d), a8, sa, b8, sb, "gate + residual",
           bias=bias, gate=gate, rpb=rpb, residual=res)


@pytest.mark.parametrize("tile", [1, 2], ids=["256x256", "128x256"])
def test_forced_tiles_views_and_swapped_operands(tile):
    """M and N past one tile with tails, ``out=`` a column block of a wider NaN-filled buffer (the rest keeps its bits), and the same
    product with the operands swapped and the bias along M."""
    from diffusers_amd import ops
    M, N, K = 257, 300, 640
    a8, sa, b8, sb = _operands(M, N, K, 99)
    bias = torch.randn(N, generator=_gen(8)).to(bf16)
    A, SA, Bq, SB, bias_d = _cuda(a8, sa, b8, sb, bias)
    wide = torch.full((M, N + 24), float("nan"), dtype=bf16, device=DEV)
    before = wide.clone()
    out = ops.linear_fp8(A, SA, Bq, SB, bias_d, out=wide[:, 8:8 + N], tile=tile)
    _check(out, a8, sa, b8, sb, f"view, tile {tile}", bias=bias)
    before[:, 8:8 + N] = out
    assert FP.bits_equal(wide, before), "bytes outside the column block changed"
    _check(ops.linear_fp8(Bq, SB, A, SA, bias_rows=bias_d, tile=tile).t(), a8, sa, b8, sb, f"swapped, tile {tile}", bias=bias)


def test_value_domain():
    from diffusers_amd import ops
    # +-448 against one-hot rows: every output is one product, exactly representable -> exact
    M, N, K = 33, 40, 256
    g = _gen(5)
    a = (torch.randint(0, 2, (M, K), generator=g).float() * 2 - 1) * 448.0
    b = torch.zeros((N, K))
    b[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = 448.0
    ones_m, ones_n = torch.ones(M), torch.ones(N)
    out = ops.linear_fp8(*_cuda(a.to(f8), ones_m, b.to(f8), ones_n))
    assert torch.equal(out.cpu().double(), (a.double() @ b.double().t()).to(bf16).double())
    # K = 15360, all positive: the longest accumulation FLUX has, nothing cancels
    a8, sa, b8, sb = _operands(17, 48, 15360, 6, positive=True)
    _check(ops.linear_fp8(*_cuda(a8, sa, b8, sb)), a8, sa, b8, sb, "K = 15360, positive")


def test_refusals_by_name(monkeypatch):
    from diffusers_amd import _lib as L, ops
    a8, sa, b8, sb = _cuda(*_operands(16, 16, 256, 1))
    x = torch.zeros((4, 256), dtype=bf16, device=DEV)
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.linear_fp8(a8[:, :192].contiguous(), sa, b8[:, :192].contiguous(), sb)
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.quantize_rows_fp8(x[:, :200])
    with pytest.raises(TypeError, match="a_q"):
        ops.linear_fp8(a8.view(torch.uint8), sa, b8, sb)
    with pytest.raises(TypeError, match="w_scale"):
        ops.linear_fp8(a8, sa, b8, sb.double())
    with pytest.raises(TypeError, match="x: expected"):
        ops.quantize_rows_fp8(x.float())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linear_fp8(a8.cpu(), sa, b8, sb)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.quantize_rows_fp8(x.cpu())
    wide = torch.zeros((16, 256 + 16), dtype=f8, device=DEV)
    with pytest.raises(ValueError, match="a_q needs a row stride"):
        ops.linear_fp8(wide[:, 8:8 + 256], sa, b8, sb)                      # base off by 8 bytes
    with pytest.raises(ValueError, match="x needs a row stride"):
        ops.quantize_rows_fp8(torch.zeros((4, 260), dtype=bf16, device=DEV)[:, :256])
    p = L.GemmFp8Params()
    assert L.load().da_gemm_fp8(C.byref(p), None) == 1                       # DA_ERR_INVALID: NULL operands, no launch
    monkeypatch.setattr(L._tls, "recorder", object(), raising=False)
    with pytest.raises(RuntimeError, match="linear_fp8: not replayable by a launch plan"):
        ops.linear_fp8(a8, sa, b8, sb)
    with pytest.raises(RuntimeError, match="quantize_rows_fp8: not replayable by a launch plan"):
        ops.quantize_rows_fp8(x)
