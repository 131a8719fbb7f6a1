"""Stand-ins of ops.resample_u8 / ops.gather_resize for the CPU tests: the two passes of include/diffusers_amd.h restated in numpy
int64 over ops.resample_tables, and a torch index_select over ops.nearest_indices."""
import numpy as np
import torch

from diffusers_amd import ops

SHAPES = [((5, 7), (16, 24)), ((37, 53), (16, 24)), ((16, 24), (16, 24)), ((16, 53), (16, 24)), ((53, 16), (24, 16)), ((1, 1), (8, 8)),
          ((9, 9), (1, 1))]


def one_pass(a: np.ndarray, in_size: int, out_size: int, filter: str, axis: int) -> np.ndarray:
    """clip8((2^21 + sum in[xmin + i] * coef[o][i]) >> 22) along ``axis``; skipped where the size stays."""
    if in_size == out_size:
        return a
    coef, bounds, _ = (t.numpy() if torch.is_tensor(t) else t for t in ops.resample_tables(in_size, out_size, filter))
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    rows = [(a[m:m + n] * coef[o, :n].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1))).sum(0) for o, (m, n) in enumerate(bounds)]
    return np.moveaxis(np.clip((np.stack(rows) + (1 << 21)) >> 22, 0, 255).astype(np.uint8), 0, axis)


def resample_u8(src: torch.Tensor, size, filter: str = "lanczos", *, route: int = 0) -> torch.Tensor:
    a = src.cpu().numpy()                                                      # [B][H][W][C]: horizontal, then vertical
    return torch.from_numpy(one_pass(one_pass(a, a.shape[2], size[1], filter, 2), a.shape[1], size[0], filter, 1))


def gather_resize(src: torch.Tensor, size, *, nchw: bool) -> torch.Tensor:
    hd, wd = (2, 3) if nchw else (1, 2)
    y, x = ops.nearest_indices(src.shape[hd], size[0]).long(), ops.nearest_indices(src.shape[wd], size[1]).long()
    return src.index_select(hd, y).index_select(wd, x).contiguous()


def install(monkeypatch, ops_module):
    monkeypatch.setattr(ops_module, "resample_u8", resample_u8)
    monkeypatch.setattr(ops_module, "gather_resize", gather_resize)
