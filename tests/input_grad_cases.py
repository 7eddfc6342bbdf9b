"""Inputs the CPU and the GPU tests of the input gradients share."""
import torch

from gpu_support import SMALL_BOX


def input_grad_points(n, box=SMALL_BOX, seed=11):
    """n points for the encode gradient: three quarters inside the box, a
    quarter scaled past it (outside on every side), and 96 of the inside ones
    moved exactly onto the min and max faces, 16 per face."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = box
    x = lo + (hi - lo) * torch.rand(n, 3, generator=g)
    k = n // 4
    x[:k] = (x[:k] - 0.5 * (lo + hi)) * 1.6 + 0.5 * (lo + hi)
    i = torch.arange(96)
    x[k + i, i % 3] = torch.where((i // 3) % 2 == 0, lo[i % 3], hi[i % 3])
    return x


def sh_dirs(n, seed=13):
    """n directions: unit ones, un-normalised ones (lengths 0.1 .. 5) and the six axes."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    d[n // 2:] *= 0.1 + 4.9 * torch.rand(n - n // 2, 1, generator=g)
    d[:6] = torch.cat([torch.eye(3), -torch.eye(3)], 0)
    return d
