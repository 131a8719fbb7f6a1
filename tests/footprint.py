"""Memory-footprint helpers for the kernel tests: guarded outputs and poisoned inputs.

A kernel test normally looks only at the elements the kernel is supposed to write and feeds inputs whose surroundings are benign.
The helpers here give every tensor of a test surroundings that the test owns and can inspect:

* ``guarded(shape, ld=..., dtype=...)`` allocates ONE flat buffer and returns the logical tensor as a strided view inside it, with a
  band before the first element, a band after the last one, the ``ld - width`` tail of every row and any gap between batches filled
  with a sentinel bit pattern.  ``Guarded.check()`` compares those bytes as integers (NaN != NaN) and names the first offenders: a
  stray WRITE is caught whatever value it stored (short of the sentinel itself).
* the same object is a poisoned INPUT: the float sentinels are NaNs, so a stray READ that reaches the arithmetic makes the output
  non-finite, and ``Guarded.clean()`` gives the same values in the same layout with zeros outside, for the bit-for-bit comparison
  "the surroundings do not influence the result".  Bytes that exist by contract but must not count (keys [Skv, Skv_alloc) of the
  attention operands) are part of the logical view: the test fills them with ``big_finite``.

Each band is at least ``max(1 MiB, tile_rows * ld * itemsize)``: the furthest one tile of rows of the kernel under test could overrun
lands in memory the test allocated.  This is a plain module (no fixtures, no pytest settings); its CPU self-tests are the
``test_*`` functions at the bottom, collected through tests/test_footprint_cpu.py.
"""
from __future__ import annotations

import math

import torch

# One pattern per element size, chosen once.  The float ones are quiet NaNs with a recognisable payload.
SENTINEL_BF16 = 0x7FA5          # bf16 / any 2-byte float: sign 0, exponent all ones, mantissa 0x25 | quiet bit
SENTINEL_F32 = 0x7FC5A5A5       # fp32: quiet NaN, payload 0x5A5A5
SENTINEL_U8 = 0xA5
MIN_BAND_BYTES = 1 << 20
TILE_ROWS = 256                 # the tallest tile of any kernel in the library (256-row GEMM tiles, 256-query attention blocks)
BF16_MAX = 3.3895313892515355e38

_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
_SENTINEL_OF = {1: SENTINEL_U8, 2: SENTINEL_BF16, 4: SENTINEL_F32}


def _signed(v: int, bits: int) -> int:
    return v - (1 << bits) if bits > 8 and v >= 1 << (bits - 1) else v


class Guarded:
    """A logical tensor (``.view``) inside a flat buffer whose every other element holds the sentinel (or zero, for a clean copy)."""

    def __init__(self, shape, ld, batch_stride, dtype, lead, trail, device, fill_sentinel=True):
        shape = tuple(int(s) for s in shape)
        self.shape, self.dtype, self.device = shape, dtype, torch.device(device)
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.width = shape[-1]
        self._batch_stride_arg = batch_stride
        self.ld = self.width if ld is None else int(ld)
        if self.ld < self.width:
            raise ValueError(f"guarded: ld {self.ld} < row width {self.width}")
        nb = shape[0] if batch_stride is not None else 1
        self.rows = math.prod(shape[:-1]) // nb                       # rows per batch
        self.batch_stride = self.rows * self.ld if batch_stride is None else int(batch_stride)
        if nb > 1 and self.batch_stride < (self.rows - 1) * self.ld + self.width:
            raise ValueError("guarded: batches overlap")
        self.batches = nb
        self.span = (nb - 1) * self.batch_stride + (self.rows - 1) * self.ld + self.width   # first to last logical element
        # a flat tensor has no rows: its band is the floor
        band = max(MIN_BAND_BYTES, TILE_ROWS * self.ld * self.itemsize if len(shape) > 1 else 0) // self.itemsize
        band = (band + 127) // 128 * 128                              # the view keeps the allocation's 256-byte alignment
        self.lead = band if lead is None else int(lead)
        self.trail = band if trail is None else int(trail)
        total = self.lead + self.span + self.trail
        self._int = _INT_OF[self.itemsize]
        self.sentinel = _signed(_SENTINEL_OF[self.itemsize], 8 * self.itemsize)
        self.bits = torch.full((total,), self.sentinel if fill_sentinel else 0, dtype=self._int, device=self.device)
        self.buf = self.bits.view(dtype)
        self._fill = self.sentinel if fill_sentinel else 0
        # element strides of the view: batch, the collapsed row dims (row-major over shape[1:-1] or shape[:-1]), column
        row_dims = shape[1:-1] if batch_stride is not None else shape[:-1]
        strides, s = [], self.ld
        for d in reversed(row_dims):
            strides.append(s)
            s *= d
        strides = ([self.batch_stride] if batch_stride is not None else []) + strides[::-1] + [1]
        self.view = self.buf.as_strided(shape, strides, self.lead)
        self.outside = torch.ones((total,), dtype=torch.bool, device=self.device)
        self.outside.as_strided(shape, strides, self.lead).fill_(False)
        self.view.zero_()

    # ---- positions ----
    def locate(self, flat: int) -> str:
        """Human-readable position of buffer element ``flat``, relative to the view."""
        off = flat - self.lead
        if off < 0:
            return f"lead band, flat offset {off}"
        if off >= self.span:
            return f"trail band, flat offset +{off - self.span} past the last element (offset {off})"
        b, r = divmod(off, self.batch_stride) if self.batches > 1 else (0, off)
        row, col = divmod(r, self.ld)
        where = f"(row {row}, col {col})" if self.batches == 1 else f"(batch {b}, row {row}, col {col})"
        if row >= self.rows:
            return f"batch gap {where}, flat offset {off}"
        return f"row tail {where}, flat offset {off}" if col >= self.width else f"inside {where}"

    def violations(self, limit: int = 8):
        bad = (self.bits != self._fill) & self.outside
        if not bool(bad.any()):
            return 0, []
        idx = torch.nonzero(bad).flatten()
        return int(idx.numel()), [int(i) for i in idx[:limit].cpu()]

    def check(self, what: str = "tensor") -> None:
        """Every element outside the logical footprint still holds the fill pattern, compared as integers."""
        n, first = self.violations()
        if n:
            where = "; ".join(f"{self.locate(i)} = {int(self.bits[i]) & ((1 << 8 * self.itemsize) - 1):#x}" for i in first)
            raise AssertionError(f"{what}: {n} element(s) outside the logical footprint changed: {where}")

    # ---- inputs ----
    def set(self, values: torch.Tensor) -> "Guarded":
        self.view.copy_(values.to(self.device, self.dtype))
        return self

    def clean(self) -> "Guarded":
        """The same logical values in the same layout (same offsets, same alignment) with zeros outside."""
        g = Guarded(self.shape, self.ld, self._batch_stride_arg, self.dtype, self.lead, self.trail, self.device, fill_sentinel=False)
        g.view.copy_(self.view)
        return g

    def snapshot(self) -> torch.Tensor:
        return self.bits.clone()

    def ptr(self) -> int:
        return self.view.data_ptr()


def guarded(shape, ld=None, dtype=torch.bfloat16, lead=None, trail=None, batch_stride=None, device="cuda") -> Guarded:
    """Logical tensor of ``shape`` (last dim contiguous, rows ``ld`` apart, ``shape[0]`` batches ``batch_stride`` apart when given)
    inside a sentinel-filled buffer; the view itself starts out as zeros."""
    if isinstance(shape, int):
        shape = (shape,)
    return Guarded(shape, ld, batch_stride, dtype, lead, trail, device)


def poisoned(values: torch.Tensor, ld=None, batch_stride=None, device="cuda", lead=None, trail=None) -> Guarded:
    """An input holding ``values`` with the sentinel everywhere else."""
    return guarded(tuple(values.shape), ld=ld, dtype=values.dtype, lead=lead, trail=trail, batch_stride=batch_stride,
                   device=device).set(values)


def big_finite(shape, seed: int, dtype=torch.bfloat16, device="cuda") -> torch.Tensor:
    """+-bf16 max with mixed signs: bytes that exist by contract but must not influence a result."""
    g = torch.Generator("cpu").manual_seed(seed)
    sign = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    return (sign * BF16_MAX).to(dtype).to(device)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-for-bit equality of two tensors of one dtype (NaNs compare by pattern)."""
    it = _INT_OF[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


# ----------------------------------------------------------------------------------------------------------------------
# CPU self-tests (unmarked): the helper is not vacuous
# ----------------------------------------------------------------------------------------------------------------------
def _small(dtype=torch.bfloat16, **kw):
    return guarded((2, 3, 5), ld=8, batch_stride=40, dtype=dtype, lead=128, trail=128, device="cpu", **kw)


def test_untouched_buffer_passes_and_view_aliases_the_buffer():
    for dtype in (torch.bfloat16, torch.float32, torch.uint8):
        g = _small(dtype)
        g.check("untouched")
        assert g.view.shape == (2, 3, 5) and g.view.stride() == (40, 8, 1)
        assert g.view.data_ptr() == g.buf.data_ptr() + g.lead * g.itemsize
        g.view[1, 2, 4] = 7
        assert g.buf[g.lead + 40 + 2 * 8 + 4] == 7          # a write through the view lands in the buffer ...
        g.buf[g.lead + 9] = 3
        assert g.view[0, 1, 1] == 3                         # ... and the other way round
        g.check("writes inside the footprint are not violations")
        if dtype != torch.uint8:
            assert torch.isnan(g.buf[0].float()) and torch.isnan(g.buf[g.lead + 5].float())


def test_default_bands_cover_a_tile_of_rows_and_a_mebibyte():
    g = guarded((3, 8), ld=16, dtype=torch.bfloat16, device="cpu")
    assert g.lead * 2 >= MIN_BAND_BYTES and g.trail * 2 >= MIN_BAND_BYTES
    assert (g.view.data_ptr() - g.buf.data_ptr()) % 256 == 0
    g = guarded((2, 8), ld=4104, dtype=torch.float32, device="cpu")
    assert g.lead >= TILE_ROWS * 4104 and g.trail >= TILE_ROWS * 4104


def test_a_planted_change_in_each_region_is_detected_and_located():
    import pytest
    cases = {                                   # flat offset relative to the view -> (region, position text)
        -1: ("lead band", "flat offset -1"),
        2 * 40 - 40 + 2 * 8 + 5: ("trail band", "+0 past"),          # first element after (batch 1, row 2, col 4)
        8 + 5: ("row tail", "row 1, col 5"),
        3 * 8 + 2: ("batch gap", "batch 0, row 3, col 2"),
        40 + 7: ("row tail", "batch 1, row 0, col 7"),
    }
    for dtype in (torch.bfloat16, torch.float32, torch.uint8):
        for off, (region, pos) in cases.items():
            g = _small(dtype)
            g.bits[g.lead + off] = 1
            n, first = g.violations()
            assert (n, first) == (1, [g.lead + off])
            with pytest.raises(AssertionError) as e:
                g.check("planted")
            assert region in str(e.value) and pos in str(e.value) and "0x1" in str(e.value), str(e.value)
    # a flipped payload bit of the sentinel is a change too, NaN or not
    g = _small(torch.float32)
    g.bits[3] = g.sentinel ^ 1
    assert torch.isnan(g.buf[3]) and g.violations()[0] == 1


def test_two_dimensional_and_flat_views_report_rows_and_columns():
    import pytest
    g = guarded((4, 6), ld=8, dtype=torch.bfloat16, lead=128, trail=128, device="cpu")
    g.bits[g.lead + 2 * 8 + 6] = 0
    with pytest.raises(AssertionError, match=r"row tail \(row 2, col 6\)"):
        g.check()
    f = guarded(7, dtype=torch.float32, lead=128, trail=128, device="cpu")
    assert f.span == 7 and f.view.shape == (7,)
    f.bits[f.lead + 7] = 0
    with pytest.raises(AssertionError, match=r"trail band, flat offset \+0"):
        f.check()


def test_clean_copy_has_the_same_layout_and_values_and_zeros_outside():
    vals = torch.arange(30, dtype=torch.float32).reshape(2, 3, 5).to(torch.bfloat16)
    p = poisoned(vals, ld=8, batch_stride=40, device="cpu", lead=128, trail=128)
    c = p.clean()
    assert c.view.stride() == p.view.stride() and c.lead == p.lead and bits_equal(c.view, p.view)
    assert int((c.bits != 0)[c.outside].sum()) == 0 and bool(torch.isnan(p.buf[p.outside].float()).all())
    c.check("clean copy")
    c.bits[0] = 5
    assert c.violations() == (1, [0])
    big = big_finite((4, 4), 0, device="cpu")
    assert bool(torch.isfinite(big.float()).all()) and float(big.float().abs().min()) == BF16_MAX and len(big.unique()) == 2
