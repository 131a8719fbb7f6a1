"""The reference's fourier_filter / apply_freeu (utils/torch_utils.py) on NHWC tensors; float64 is the tests' yardstick, float32 the
reference's own route (whose error sets their slack)."""
import torch


def fourier_filter(x_nhwc: torch.Tensor, scale: float, dtype=torch.float64, threshold: int = 1) -> torch.Tensor:
    """[B][H][W][C] -> the filtered planes in ``dtype``, NOT rounded to the input's type."""
    x = x_nhwc.permute(0, 3, 1, 2).to(dtype)
    B, C, H, W = x.shape
    x_freq = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = torch.fft.ifftshift(x_freq * mask, dim=(-2, -1))
    return torch.fft.ifftn(x_freq, dim=(-2, -1)).real.permute(0, 2, 3, 1).contiguous()


def apply_freeu(hidden: torch.Tensor, skip: torch.Tensor, s: float, b: float):
    """(hidden with its first half of the channels times b -- torch's own bf16 tensor times Python float --, float64 filtered skip)."""
    hidden = hidden.clone()
    half = hidden.shape[-1] // 2
    hidden[..., :half] = hidden[..., :half] * b
    return hidden, fourier_filter(skip, s)


def data(B, H, W, C, seed):
    """Seeded Gaussian plus a per-channel DC offset (the low-pass term is not negligible), bf16."""
    g = torch.Generator("cpu").manual_seed(seed)
    return (torch.randn((B, H, W, C), generator=g) + 2.0 * torch.randn((1, 1, 1, C), generator=g)).to(torch.bfloat16)
