"""GPU tests of WHERE IN MEMORY an operand sits: tensors whose byte offsets pass 2^31 / 2^32 / 2^33 and whose bf16 element indices
pass 2^31 / 2^32 (the Wan 2.1 decoder's last level at 81 x 480 x 832 is 8.3 GB per activation), and operands at the edge of the
31-bit offset budget of the buffer-addressed staging (DESIGN.md "Address arithmetic past 2 GiB / 4 GiB").

Large tensors are periodic (tests/large_address.py): one random block of P = 7 frames of 24 x 40 pixels repeated to just past the
tier's boundary.  Per case: (1) the whole output is bit-periodic; (2) period 0 and the frames that hold each boundary match an fp64
reference at assert_close_bf16's defaults; (3) period 0 is bit-equal to the same op launched on a cloned single period (a
small-address launch) wherever the K order is the same; (4) read-only operands are unchanged.  Every launch pins tile, staging and
split_k = 1, or runs the auto path with live tuning off.  Tier A holds at most ~10 GB at once, tier B ~20 GB (asserted per test from
torch.cuda.max_memory_allocated(); the figures are in profiles/large_address_numbers.md).

The budget tests put a 300-row problem behind strides at both sides of each limit: da_gemm::buffer_staging_fits /
da_gemm2::staging_fits (the largest admitted lda / ldw, and the smallest refused, which sends first-family tiles to the per-lane
pointer staging) and the two checks at the top of da_attn2_dispatch.  Every limit is derived from the predicate's own formula."""
import ctypes
import gc
import time

import pytest
import torch

import large_address as LA
import value_domain as V
from conftest import assert_close_bf16
from test_conv_chunk_gpu import _conv_ref64
from test_gemm_k2_gpu import _ops, rnd
from test_kernels_gpu import _attn_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
bf16 = torch.bfloat16
f64 = torch.float64
GIB = float(1 << 30)
CAP_BYTES = {"A": 10.5e9, "B": 20.5e9, "-": 6.0e9}      # "~10 GB" / "~20 GB" live at once; the budget tests stay far below
LAYOUTS = LA.layouts()
H_, W_ = LA.FRAME_HW
P = 7


@pytest.fixture(autouse=True)
def _memory_and_time(request):
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated()
    name = request.node.name
    tier = "A" if "tier_a" in name else "B" if "tier_b" in name else "-"
    print(f"[memory] {name}: tier {tier} peak_allocated={peak / 1e9:.2f} GB wall={dt:.2f} s")
    gc.collect()
    torch.cuda.empty_cache()
    assert peak <= CAP_BYTES[tier], f"{name}: {peak / 1e9:.2f} GB live at once, tier cap {CAP_BYTES[tier] / 1e9:.1f} GB"


def _no_live_tuning(monkeypatch):
    from diffusers_amd import tuning
    monkeypatch.setattr(tuning, "LIVE", False)
    return tuning


def _check_frames(out, ref_of_frame, pls, what, exact=False):
    """Period 0 and every frame that holds a boundary of the output or of an input (``pls``: the plans of the large operands)
    against the reference (ref_of_frame(f) -> the fp64 reference of frame f)."""
    pls = pls if isinstance(pls, (list, tuple)) else [pls]
    held = sorted({(f, lab) for pl in pls for lab, f in pl.boundary_frames.items()})
    frames = list(range(P)) + sorted({f for f, _ in held})
    got = torch.stack([out[f] for f in frames])
    ref = torch.stack([ref_of_frame(f) for f in frames])
    where = ", ".join(f"{lab} in frame {f}" for f, lab in held)
    if exact:
        assert torch.equal(got, ref.to(got.dtype)), f"{what}: period 0 / boundary frames differ from the reference ({where})"
        print(f"[parity] {what}: period 0 + boundary frames ({where}) bit-equal to the reference")
    else:
        assert_close_bf16(got, ref, f"{what}: period 0 + boundary frames ({where})")


def _unchanged(t, block_dev, what, first_frame=0):
    LA.assert_periodic(t, P, f"{what} (read-only operand)", first_frame)
    assert torch.equal(t[:P], block_dev), f"{what}: read-only operand changed in period 0"


# ----------------------------------------------------------------------------------------------------------------------
# conv2d_nhwc 3 x 3
# ----------------------------------------------------------------------------------------------------------------------
def _conv_weights(Cin, kv, N, seed):
    w4 = rnd((N, Cin, 3, 3), seed, (9 * kv) ** -0.5)
    w4[:, kv:] = 0                                   # k_valid: channels >= kv are zero padding in BOTH operands
    return w4, rnd((N,), seed + 1, 0.1)


def _run_conv(pl_out, pl_in, *, Cin, kv, N, in_hw, up, tile, staging, residual, seed, what, chunk_sensitive=False):
    ops, L = _ops()
    T = pl_out.T
    assert pl_in.T == T and pl_in.frame_elems == in_hw[0] * in_hw[1] * Cin and pl_out.frame_elems == H_ * W_ * N
    xb = LA.random_block((P, in_hw[0], in_hw[1], Cin), seed, zero_from_channel=kv).to(DEV)
    w4, b = _conv_weights(Cin, kv, N, seed + 10)
    w = ops.pack_conv_weight(w4)
    rb = LA.random_block((P, H_, W_, N), seed + 20).to(DEV) if residual else None
    kw = dict(ksize=3, up=up, tile=tile, staging=staging, split_k=1, k_valid=kv if kv < Cin else 0)
    ref = _conv_ref64(xb, None, w4, b, 1, up, 3, res=rb)
    # the small-address launch: one cloned period
    small_out = rb.clone() if residual else None
    small = ops.conv2d_nhwc(xb.clone(), w, b, residual=small_out, out=small_out, **kw)
    w_keep, b_keep = w.clone(), b.clone()

    x = LA.repeat_block(xb, T)
    # the residual variant accumulates in place (out IS the residual, as the temporal taps of the causal Conv3d do): a third
    # 4.3 GB tensor would pass the tier's memory cap
    out = LA.repeat_block(rb, T) if residual else torch.full((T, H_, W_, N), -0.0, dtype=bf16, device=DEV)
    y = ops.conv2d_nhwc(x, w, b, residual=out if residual else None, out=out, **kw)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    LA.assert_periodic(out, P, what)
    _check_frames(out, lambda f: ref[f % P], [pl_out, pl_in], what)
    same_order = not chunk_sensitive or (ops.conv_chunk_channels(x, w, tile, up=up) == ops.conv_chunk_channels(xb, w, tile, up=up))
    if same_order:
        assert torch.equal(out[:P], small), f"{what}: period 0 differs from the small-address launch"
        print(f"[parity] {what}: period 0 bit-equal to the small-address launch")
    else:
        assert_close_bf16(out[:P], small, f"{what}: period 0 vs the small-address launch (another chunk of the K order)")
    _unchanged(x, xb, f"{what} x")
    assert torch.equal(w, w_keep) and torch.equal(b, b_keep), f"{what}: weights / bias changed"


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
def test_tier_a_conv3_c128_n128_w8(residual):
    """Wan decoder, last level: C1 = 128 stored / 96 real, N = 128, 128x128w8 / LDS_DIRECT (the shipped table's tile)."""
    _, L = _ops()
    _run_conv(LAYOUTS["A_c128"], LAYOUTS["A_c128"], Cin=128, kv=96, N=128, in_hw=(H_, W_), up=False, tile=L.TILE_128x128_W8,
              staging=L.STAGE_LDS_DIRECT, residual=residual, seed=100, what=f"A conv3 C128(96)->128 128x128w8 res={int(residual)}")


def test_tier_a_conv3_c128_n4_128x64():
    """conv_out: large input, thin output."""
    _, L = _ops()
    _run_conv(LAYOUTS["A_n4"], LAYOUTS["A_c128"], Cin=128, kv=96, N=4, in_hw=(H_, W_), up=False, tile=L.TILE_128x64,
              staging=L.STAGE_LDS_DIRECT, residual=False, seed=110, what="A conv3 C128(96)->4 128x64")


def test_tier_a_conv3_up_c192_n128():
    """The upsampling conv: 12 x 20 x 192 frames, nearest 2x in the gather, -> 24 x 40 x 128.  The output passes 4 GiB; the input,
    2.67 x smaller, passes 2 GiB (an input past 4 GiB needs an 11.5 GB output: more than tier A holds -- DESIGN.md 3.4)."""
    _, L = _ops()
    assert {"2^31 B", "2^32 B", "2^31 elements"} <= set(LAYOUTS["A_up_out"].boundary_frames)
    assert set(LAYOUTS["A_up_in"].boundary_frames) == {"2^31 B"}
    _run_conv(LAYOUTS["A_up_out"], LAYOUTS["A_up_in"], Cin=192, kv=192, N=128, in_hw=(12, 20), up=True, tile=L.TILE_128x128_W8,
              staging=L.STAGE_LDS_DIRECT, residual=False, seed=120, what="A conv3 up C192->128 128x128w8")


def test_tier_a_conv3_c128_n128_second_family():
    _, L = _ops()
    _run_conv(LAYOUTS["A_c128"], LAYOUTS["A_c128"], Cin=128, kv=96, N=128, in_hw=(H_, W_), up=False, tile=L.TILE_K2_128x128,
              staging=L.STAGE_PINGPONG, residual=False, seed=130, what="A conv3 C128(96)->128 k2:128x128/pingpong", chunk_sensitive=True)


def test_tier_b_conv3_c128_n128_w8():
    """Just over 8 GiB (2^32 bf16 elements) for input and output; 33.6 M pixels stay below the 2^31 the host check admits."""
    _, L = _ops()
    _run_conv(LAYOUTS["B_c128"], LAYOUTS["B_c128"], Cin=128, kv=96, N=128, in_hw=(H_, W_), up=False, tile=L.TILE_128x128_W8,
              staging=L.STAGE_LDS_DIRECT, residual=False, seed=140, what="B conv3 C128(96)->128 128x128w8")


def test_tier_a_causal_conv3d_pattern():
    """CausalConv3d: the last tap writes all frames, then conv(x[:T-1], w_prev) accumulates IN PLACE through the frame-shifted
    view out[1:].  Periodic from frame 1 on; reference conv_last(x[t]) + conv_prev(x[t-1]), rounded as the two launches round."""
    ops, L = _ops()
    pl = LAYOUTS["A_c128"]
    T, kv = pl.T, 96
    what = "A causal conv3d C128(96)->128 128x128w8"
    xb = LA.random_block((P, H_, W_, 128), 150, zero_from_channel=kv).to(DEV)
    w4_last, b = _conv_weights(128, kv, 128, 160)
    w4_prev, _ = _conv_weights(128, kv, 128, 170)
    w_last, w_prev = ops.pack_conv_weight(w4_last), ops.pack_conv_weight(w4_prev)
    kw = dict(ksize=3, tile=L.TILE_128x128_W8, staging=L.STAGE_LDS_DIRECT, split_k=1, k_valid=kv)

    def run(x):
        out = torch.full((x.shape[0], H_, W_, 128), -0.0, dtype=bf16, device=DEV)
        ops.conv2d_nhwc(x, w_last, b, out=out, **kw)
        ops.conv2d_nhwc(x[:-1], w_prev, residual=out[1:], out=out[1:], **kw)
        return out

    xs = torch.cat([xb, xb[:1]])                                       # frames 0 .. P of the periodic tensor
    small = run(xs.clone())
    last = _conv_ref64(xs, None, w4_last, b, 1, False, 3).to(bf16).to(f64)      # the first launch rounds to bf16
    ref = last.clone()
    ref[1:] += _conv_ref64(xs[:-1], None, w4_prev, torch.zeros_like(b), 1, False, 3)
    x = LA.repeat_block(xb, T)
    out = run(x)
    torch.cuda.synchronize()
    LA.assert_periodic(out, P, what, first_frame=1)
    _check_frames(out, lambda f: ref[f if f == 0 else (f - 1) % P + 1], pl, what)
    assert torch.equal(out[:P + 1], small), f"{what}: frames 0 .. {P} differ from the small-address launch"
    print(f"[parity] {what}: frames 0 .. {P} bit-equal to the small-address launch")
    _unchanged(x, xb, f"{what} x")


# ----------------------------------------------------------------------------------------------------------------------
# linear as the 1 x 1 temporal conv
# ----------------------------------------------------------------------------------------------------------------------
_LIN = {}


def _lin_problem():
    """Operands and the fp64 reference of frames 0 .. P, shared by the four variants (computed once, never modified)."""
    if not _LIN:
        K, N, kv = 192, 384, 160
        xb = LA.random_block((P, LA.HW, K), 200, zero_from_channel=kv).to(DEV)
        w_last, w_prev, b = rnd((N, K), 210, kv ** -0.5), rnd((N, K), 211, kv ** -0.5), rnd((N,), 212, 0.1)
        w_last[:, kv:] = 0
        w_prev[:, kv:] = 0
        xs = torch.cat([xb, xb[:1]]).view(-1, K)                                        # frames 0 .. P
        last = (xs.to(f64) @ w_last.to(f64).t() + b.to(f64)).to(bf16).to(f64)
        ref = last.clone()
        ref[LA.HW:] += xs[:-LA.HW].to(f64) @ w_prev.to(f64).t()
        _LIN.update(K=K, N=N, kv=kv, xb=xb, w_last=w_last, w_prev=w_prev, b=b, ref=ref.view(P + 1, LA.HW, N),
                    keep=(xb.clone(), w_last.clone(), w_prev.clone(), b.clone()))
    return _LIN


@pytest.mark.parametrize("variant", ["first:128x128", "k2:128x128", "k3:256x256", "auto"])
def test_tier_a_linear_temporal_conv(variant, monkeypatch):
    """M = 5.6 M rows, K = 192 (160 valid), N = 384: the output passes 4 GiB, the input 2 GiB.  k_valid, bias, out=, and the
    in-place accumulation of the previous frame's tap through the row-shifted view (residual = out = out2d[960:])."""
    ops, L = _ops()
    tuning = _no_live_tuning(monkeypatch)
    q = _lin_problem()
    pl_out, pl_in = LAYOUTS["A_lin_out"], LAYOUTS["A_lin_in"]
    T, K, N, kv, hw = pl_out.T, q["K"], q["N"], q["kv"], LA.HW
    tile, staging = {"first:128x128": (L.TILE_128x128, L.STAGE_LDS_DIRECT), "k2:128x128": (L.TILE_K2_128x128, L.STAGE_PINGPONG),
                     "k3:256x256": (L.TILE_K3_256x256, L.STAGE_LDS_DIRECT), "auto": (None, None)}[variant]
    kw = dict(k_valid=kv, tile=tile, staging=staging, split_k=None if variant == "auto" else 1)
    what = f"A linear M{T * hw} K{K}({kv}) N{N} {variant}"
    if variant == "auto":   # the auto path: the shipped table's entry if there is one, else the library's own first-family choice
        keys = [f"lin:M{tuning._m_key(m)}:N{N}:K{K}:a0:f0:r{r}:v{kv}" for m in (T * hw, (T - 1) * hw) for r in (0, 1)]
        print(f"[parity] {what}: table entries {[tuning.table().get(k) for k in keys]}")

    def run(x2d):
        out = torch.full((x2d.shape[0], N), -0.0, dtype=bf16, device=DEV)
        y = ops.linear(x2d, q["w_last"], q["b"], out=out, **kw)
        assert y.data_ptr() == out.data_ptr()
        ops.linear(x2d[:-hw], q["w_prev"], residual=out[hw:], out=out[hw:], **kw)
        return out

    small = run(torch.cat([q["xb"], q["xb"][:1]]).view(-1, K).clone()).view(P + 1, hw, N)
    x = LA.repeat_block(q["xb"], T)
    out = run(x.view(T * hw, K)).view(T, hw, N)
    torch.cuda.synchronize()
    LA.assert_periodic(out, P, what, first_frame=1)
    _check_frames(out, lambda f: q["ref"][f if f == 0 else (f - 1) % P + 1], [pl_out, pl_in], what)
    # the K order of a Linear does not depend on M in any family: bit-equal (auto: both launches take the first family unless
    # the table says otherwise for one of the two shapes)
    if variant != "auto" or all(tuning.table().get(k) is None for k in keys):
        assert torch.equal(out[:P + 1], small), f"{what}: frames 0 .. {P} differ from the small-address launch"
        print(f"[parity] {what}: frames 0 .. {P} bit-equal to the small-address launch")
    else:
        assert_close_bf16(out[:P + 1], small, f"{what}: frames 0 .. {P} vs the small-address launch")
    assert pl_in.T == T
    _unchanged(x, q["xb"], f"{what} x")
    for t, k in zip((q["xb"], q["w_last"], q["w_prev"], q["b"]), q["keep"]):
        assert torch.equal(t, k), f"{what}: a read-only operand changed"


# ----------------------------------------------------------------------------------------------------------------------
# rmsnorm_channels, permute_0213
# ----------------------------------------------------------------------------------------------------------------------
def _run_rms(pl, silu, what):
    ops, _ = _ops()
    xb = LA.random_block((P, H_, W_, 128), 300, zero_from_channel=96).to(DEV)
    gamma = (V._randn((128,), 301) * 0.1 + 1.0).to(bf16).to(DEV)
    gamma[96:] = 0
    ref = V.rmsnorm_channels_ref64(xb, gamma, 96, silu)
    small = ops.rmsnorm_channels(xb.clone(), gamma, real_channels=96, silu=silu)
    g_keep = gamma.clone()
    x = LA.repeat_block(xb, pl.T)
    y = ops.rmsnorm_channels(x, gamma, real_channels=96, silu=silu)
    torch.cuda.synchronize()
    LA.assert_periodic(y, P, what)
    _check_frames(y, lambda f: ref[f % P], pl, what)
    assert torch.equal(y[:P], small), f"{what}: period 0 differs from the small-address launch"
    assert bool((y[:P, ..., 96:] == 0).all()), f"{what}: channel padding not zero"
    print(f"[parity] {what}: period 0 bit-equal to the small-address launch")
    _unchanged(x, xb, f"{what} x")
    assert torch.equal(gamma, g_keep)


@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
def test_tier_a_rmsnorm_channels(silu):
    _run_rms(LAYOUTS["A_c128"], silu, f"A rmsnorm_channels C128(96) silu={int(silu)}")


@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
def test_tier_b_rmsnorm_channels(silu):
    _run_rms(LAYOUTS["B_c128"], silu, f"B rmsnorm_channels C128(96) silu={int(silu)}")


def _run_permute(pl, what):
    """WanResample upsample3d: [F][HW][2][cp] -> [F][2][HW][cp], cp = 384 (F = the T - 1 frames time_conv produced)."""
    ops, _ = _ops()
    F_, cp = pl.T, 384
    xb = LA.random_block((P, LA.HW, 2, cp), 400).to(DEV)
    ref = xb.permute(0, 2, 1, 3).contiguous()
    small = ops.permute_0213(xb.clone())
    x = LA.repeat_block(xb, F_)
    out = torch.full((F_, 2, LA.HW, cp), -0.0, dtype=bf16, device=DEV)
    y = ops.permute_0213(x, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    LA.assert_periodic(out, P, what)
    _check_frames(out, lambda f: ref[f % P], pl, what, exact=True)      # a pure copy: the reference is exact
    assert torch.equal(out[:P], small), f"{what}: period 0 differs from the small-address launch"
    _unchanged(x, xb, f"{what} x")


def test_tier_a_permute_0213():
    _run_permute(LAYOUTS["A_perm"], "A permute_0213 [F][960][2][384]")


def test_tier_b_permute_0213():
    _run_permute(LAYOUTS["B_perm"], "B permute_0213 [F][960][2][384]")


# ----------------------------------------------------------------------------------------------------------------------
# the 31-bit offset budget of the buffer-addressed staging, and the per-lane-pointer fallback behind it
# ----------------------------------------------------------------------------------------------------------------------
# da_gemm::buffer_staging_fits (csrc/gemm_kernel.cuh:991-994) and da_gemm2::staging_fits (csrc/gemm2_shared.cuh:171-174), nn.Linear:
#     const size_t lim = 0x3fffffffull;
#     if ((size_t)p.ldw * 512 >= lim || (size_t)p.K * 2 >= lim) return false;
#     if (!p.conv) return (size_t)p.lda * 512 < lim;
# da_gemm_bf16 (csrc/gemm.hip:93) also wants lda, ldw multiples of 8.
BUDGET_LIM = 0x3FFFFFFF
LD_ADMITTED = (BUDGET_LIM - 1) // 512 // 8 * 8            # largest multiple of 8 with ld * 512 <  lim  (2^21 - 8)
LD_REFUSED = -(-BUDGET_LIM // 512) + 7 & ~7               # smallest multiple of 8 with ld * 512 >= lim (2^21)
BM_, BN_, BK_ = 300, 320, 192


def test_budget_limits_follow_the_predicate():
    assert LD_ADMITTED * 512 < BUDGET_LIM <= (LD_ADMITTED + 8) * 512 and LD_ADMITTED % 8 == 0
    assert LD_REFUSED * 512 >= BUDGET_LIM > (LD_REFUSED - 8) * 512 and LD_REFUSED % 8 == 0
    assert (LD_ADMITTED, LD_REFUSED) == (2 ** 21 - 8, 2 ** 21)


def _strided_rows(t, ld):
    """``t`` [R][K] as a row view with leading dimension ``ld`` inside ONE allocation of (R - 1) * ld + K elements; only the view is
    written (the rest of the ~1.3 GB is whatever the allocator handed out)."""
    R, K = t.shape
    buf = torch.empty((R - 1) * ld + K, dtype=t.dtype, device=t.device)
    v = buf.as_strided((R, K), (ld, 1))
    v.copy_(t)
    return v


def _first_family(L):
    return [(t, st) for t in range(L.TILE_128x128, L.TILE_128x128_W8 + 1) for st in range(L.STAGE_REGISTER, L.STAGE_LDS_DIRECT8 + 1)]


def _budget_problem():
    x, w, b = rnd((BM_, BK_), 500), rnd((BN_, BK_), 501, BK_ ** -0.5), rnd((BN_,), 502, 0.1)
    ref = x.to(f64) @ w.to(f64).t() + b.to(f64)
    return x, w, b, ref


@pytest.mark.parametrize("operand", ["x", "w"])
@pytest.mark.parametrize("side", ["admitted", "refused"])
def test_first_family_at_both_sides_of_the_staging_budget(operand, side):
    """Every first-family (tile, staging): the operand behind the largest admitted / smallest refused leading dimension gives the
    bits of the contiguous launch -- buffer mode at its largest offsets, and the per-lane-pointer staging behind the refusal."""
    ops, L = _ops()
    x, w, b, ref = _budget_problem()
    ld = LD_ADMITTED if side == "admitted" else LD_REFUSED
    xs, ws = (_strided_rows(x, ld), w) if operand == "x" else (x, _strided_rows(w, ld))
    assert (xs.stride(0) if operand == "x" else ws.stride(0)) == ld
    ran = 0
    for t, st in _first_family(L):
        name = f"{L.TILE_NAMES[t]}/{st}"
        try:
            base = ops.linear(x, w, b, tile=t, staging=st, split_k=1)
        except RuntimeError as e:
            assert "DA_ERR_UNSUPPORTED" in str(e), f"{name}: {e}"
            with pytest.raises(RuntimeError, match="DA_ERR_UNSUPPORTED"):
                ops.linear(xs, ws, b, tile=t, staging=st, split_k=1)
            continue
        y = ops.linear(xs, ws, b, tile=t, staging=st, split_k=1)
        assert torch.equal(y, base), f"linear {operand} ld {ld} ({side}) {name}: differs from the contiguous launch"
        if ran == 0:
            assert_close_bf16(base, ref, f"budget linear contiguous {name}")
            assert_close_bf16(y, ref, f"budget linear {operand} ld={ld} ({side}) {name}")
            first = base
        else:
            assert torch.equal(base, first), f"{name}: first-family variants are bit-identical"
        ran += 1
    assert ran >= 25, f"only {ran} first-family variants ran"
    assert torch.equal(xs, x) and torch.equal(ws, w)
    print(f"[parity] budget linear {operand} ld={ld} ({side}): {ran} first-family variants bit-equal to the contiguous launch")


@pytest.mark.parametrize("operand", ["x", "w"])
def test_past_the_budget_pinned_variants_fail_cleanly(operand):
    """A caller-pinned second-family or eight-phase tile, split_k = 2 and a LayerNorm-fold launch have no per-lane-pointer build:
    DA_ERR_UNSUPPORTED from the host, nothing launched, the output untouched.  At the admitted side the same calls run."""
    ops, L = _ops()
    x, w, b, ref = _budget_problem()
    calls = {
        "k2:128x128/pingpong": dict(tile=L.TILE_K2_128x128, staging=L.STAGE_PINGPONG),
        "k1:256x128": dict(tile=L.TILE_K1_256x128, staging=L.STAGE_LDS_DIRECT),
        "k3:256x256": dict(tile=L.TILE_K3_256x256, staging=L.STAGE_LDS_DIRECT),
        "split_k=2": dict(tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT, split_k=2),
        "ln-fold producer": dict(tile=L.TILE_128x64, staging=L.STAGE_LDS_DIRECT3, stats_out=True),
    }
    for side, ld in (("admitted", LD_ADMITTED), ("refused", LD_REFUSED)):
        xs, ws = (_strided_rows(x, ld), w) if operand == "x" else (x, _strided_rows(w, ld))
        for name, kw in calls.items():
            kw = dict(kw)
            if kw.pop("stats_out", False):
                kw["stats_out"] = ops.RowStats(BM_, DEV)
            out = torch.full((BM_, BN_), float("nan"), dtype=bf16, device=DEV)
            if side == "admitted":
                ops.linear(xs, ws, b, out=out, **kw)
                assert_close_bf16(out, ref, f"budget {operand} ld={ld} {name}")
            else:
                with pytest.raises(RuntimeError, match="DA_ERR_UNSUPPORTED"):
                    ops.linear(xs, ws, b, out=out, **kw)
                torch.cuda.synchronize()
                assert bool(torch.isnan(out).all()), f"{name}: a refused launch wrote to its output"
        del xs, ws


@pytest.mark.parametrize("operand", ["x", "w"])
def test_past_the_budget_table_selected_tile_is_retried(operand, monkeypatch):
    """A TABLE-selected second-family tile that refuses the operand layout is replaced by the library's first-family choice
    (ops._launch_gemm): same bits as a pinned first-family tile."""
    ops, L = _ops()
    tuning = _no_live_tuning(monkeypatch)
    x, w, b, ref = _budget_problem()
    xs, ws = (_strided_rows(x, LD_REFUSED), w) if operand == "x" else (x, _strided_rows(w, LD_REFUSED))
    p, st = ops._linear_params(xs, ws, b)
    monkeypatch.setitem(tuning.table(), tuning.key_of(p), (L.TILE_K2_128x128, L.STAGE_PINGPONG, 1.0, 1))
    # the entry is what the unpinned launch selects ...
    p, st = ops._linear_params(xs, ws, b)
    assert (p.tile, p.staging, p._auto) == (L.TILE_K2_128x128, L.STAGE_PINGPONG, True)
    # ... the library refuses it for this layout, and the retry rewrites the selection
    assert L.load().da_gemm_bf16(ctypes.byref(p), st) == ops.DA_ERR_UNSUPPORTED
    ops._launch_gemm(p, st, "retry")
    assert p.tile == L.TILE_AUTO
    y = ops.linear(xs, ws, b)
    first = ops.linear(xs, ws, b, tile=L.TILE_128x128, staging=L.STAGE_LDS_DIRECT, split_k=1)
    assert torch.equal(y, first) and torch.equal(p._out, first), "the retried launch differs from the first family"
    assert_close_bf16(y, ref, f"budget {operand} ld={LD_REFUSED} table k2 -> retry")
    # on contiguous operands the same entry runs the second-family tile itself
    yc = ops.linear(x, w, b)
    assert torch.equal(yc, ops.linear(x, w, b, tile=L.TILE_K2_128x128, staging=L.STAGE_PINGPONG, split_k=1))


# da_attn2_dispatch (csrc/attention2.hip:660-661):
#     if ((size_t)p.Skv_alloc * (size_t)p.k_row_stride * 2 + 64ull * p.k_row_stride * 2 >= 0x7fffffffull) return DA_ERR_UNSUPPORTED;
#     if ((size_t)p.D * (size_t)p.vt_ld * 2 + (size_t)p.Skv_alloc * 2 >= 0x7fffffffull) return DA_ERR_UNSUPPORTED;
# da_attention_bf16 (csrc/attention.hip:705, 713) wants Skv_alloc, k_row_stride, vt_ld multiples of 8.
ATT = dict(B=1, H=2, D=64, Sq=130, Skv=333)
ATT_SKV_ALLOC = (ATT["Skv"] + 7) // 8 * 8
ATT_LIM = 0x7FFFFFFF


def _attn_limits():
    sa, D = ATT_SKV_ALLOC, ATT["D"]
    k_ok = (ATT_LIM - 1) // (2 * (sa + 64)) // 8 * 8                       # largest k_row_stride the first check admits
    v_ok = (ATT_LIM - 1 - 2 * sa) // (2 * D) // 8 * 8                      # largest vt_ld the second check admits
    return k_ok, k_ok + 8, v_ok, v_ok + 8


def test_attention_limits_follow_the_predicate():
    sa, D = ATT_SKV_ALLOC, ATT["D"]
    k_ok, k_no, v_ok, v_no = _attn_limits()
    assert sa * k_ok * 2 + 64 * k_ok * 2 < ATT_LIM <= sa * k_no * 2 + 64 * k_no * 2
    assert D * v_ok * 2 + sa * 2 < ATT_LIM <= D * v_no * 2 + sa * 2


@pytest.mark.parametrize("which", ["k_row_stride", "vt_ld"])
@pytest.mark.parametrize("side", ["admitted", "refused"])
def test_attention_at_both_sides_of_the_offset_budget(which, side):
    """The largest stride each budget check admits runs the second-generation kernel (pinned with algo = 2 to prove it) at its
    largest offsets; the smallest refused stride is a clean DA_ERR_UNSUPPORTED from that generation and, unpinned, a correct
    result from the first-generation kernel (per-lane 64-bit pointers) the dispatcher falls back to."""
    ops, L = _ops()
    B, H, D, Sq, Skv = (ATT[k] for k in ("B", "H", "D", "Sq", "Skv"))
    C, sa = H * D, ATT_SKV_ALLOC
    k_ok, k_no, v_ok, v_no = _attn_limits()
    krs = (k_ok if side == "admitted" else k_no) if which == "k_row_stride" else C
    vld = (v_ok if side == "admitted" else v_no) if which == "vt_ld" else sa
    q, k, v = rnd((B, Sq, C), 600), rnd((B, Skv, C), 601), rnd((B, Skv, C), 602)
    kp = torch.zeros((sa, C), dtype=bf16, device=DEV)
    kp[:Skv] = k[0]
    vp = torch.zeros((C, sa), dtype=bf16, device=DEV)
    vp[:, :Skv] = v[0].t()
    ks, vs = _strided_rows(kp, krs), _strided_rows(vp, vld)
    kw = dict(B=B, H=H, D=D, Sq=Sq, Skv=Skv, Skv_alloc=sa, q_row_stride=C, k_row_stride=krs, q_batch_stride=Sq * C,
              k_batch_stride=sa * krs, vt_ld=vld, vt_batch_stride=sa)
    ref = _attn_ref(q, k, v, H).view(B * Sq, C)
    what = f"attention D{D} Sq{Sq} Skv{Skv} {which}={krs if which == 'k_row_stride' else vld} ({side})"
    o = ops.attention(q.view(B * Sq, C), ks, vs, **kw)
    assert_close_bf16(o, ref, what, rtol=1.6e-2, atol_rms=1.6e-2)
    base = ops.attention(q.view(B * Sq, C), kp, vp, **dict(kw, k_row_stride=C, k_batch_stride=sa * C, vt_ld=sa))
    assert_close_bf16(base, ref, f"{what}: contiguous operands", rtol=1.6e-2, atol_rms=1.6e-2)
    if side == "admitted":
        o2 = ops.attention(q.view(B * Sq, C), ks, vs, algo=2, **kw)
        assert torch.equal(o2, o) and torch.equal(o, base), f"{what}: differs from the second generation on contiguous operands"
    else:
        out = torch.full((B * Sq, C), float("nan"), dtype=bf16, device=DEV)
        with pytest.raises(RuntimeError, match="DA_ERR_UNSUPPORTED"):
            ops.attention(q.view(B * Sq, C), ks, vs, algo=2, out=out, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), f"{what}: the refused launch wrote to its output"
        v1 = ops.attention(q.view(B * Sq, C), kp, vp, algo=1, **dict(kw, k_row_stride=C, k_batch_stride=sa * C, vt_ld=sa))
        assert torch.equal(o, v1), f"{what}: the fallback is not the first-generation kernel's result"
    assert torch.equal(ks, kp) and torch.equal(vs, vp)
