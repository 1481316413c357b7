"""Sampling grids shared by the kernel tests of mrfa_grid_sample_* (tests/test_bf16_cache.py, tests/test_sample_kernels_gpu.py) and by the CPU tests of the
float64 reference (tests/test_sample_reference.py): coordinates placed on purpose, and the flows the run-merging backward kernel is written for or against."""
import math

import numpy as np
import torch


def gs_grid(N, Ho, Wo, Hi, Wi, mode, seed):
    """sampling grid with ordinary, integer, border, far-outside and NaN coordinates; returns (grid [N*Ho*Wo, 2], rows wholly outside)"""
    g = torch.Generator().manual_seed(seed)
    n = N * Ho * Wo
    if mode == 0:
        grid = torch.rand(n, 2, generator=g) * 2.6 - 1.3
        px = lambda ix, iy: torch.tensor([(2 * ix + 1) / Wi - 1, (2 * iy + 1) / Hi - 1])          # pixel coordinate -> normalised, align_corners=False
        def put(i, ix, iy):
            grid[i] = px(ix, iy)
    else:
        grid = torch.rand(n, 2, generator=g) * 10 - 5
        def put(i, ix, iy):
            ox, oy = i % Wo, (i // Wo) % Ho
            grid[i] = torch.tensor([ix - ox, iy - oy], dtype=torch.float32)
    special = [(2.0, 3.0), (0.0, 0.0), (Wi - 1.0, Hi - 1.0), (-0.5, 2.0), (-1.0, 1.0), (Wi - 0.5, 1.25), (float(Wi), 2.0), (1.5, -0.25), (3.0, -1.0),
               (2.5, Hi - 0.75), (1.0, float(Hi)), (-0.999, -0.999), (Wi - 1.0, 0.0)]
    outside = [(-7.0, 2.0), (1e6, 1e6), (-1e30, 3.0), (2.0, Hi + 40.0), (float("nan"), 1.0), (1.0, float("nan")), (float("nan"), float("nan")),
               (float("inf"), 0.0), (-1.5, -1.5)]
    for i, (ix, iy) in enumerate(special):
        put(3 + 2 * i, ix, iy)
    rows = []
    for i, (ix, iy) in enumerate(outside):
        r = 4 + 2 * len(special) + 2 * i
        if np.isfinite(ix) and np.isfinite(iy):
            put(r, ix, iy)
        else:
            grid[r] = torch.tensor([ix, iy])                                  # NaN / infinite grid values themselves
        rows.append(r)
    return grid, rows


FLOWS = ("shift", "identity", "collapse", "reverse", "stride2", "sinus")


def flow_grid(kind, N, Ho, Wo, Hi, Wi, mode):
    """[N*Ho*Wo, 2] grid that samples pixel (sx(ox, oy), sy(ox, oy)):
      shift     constant fractional shift: the smooth flow the carried tap column is for (a merge on every step of a run)
      identity  exact integer coordinates, fx = fy = 0; the last column's right-hand tap is x1 == Wi
      collapse  every pixel of a row onto one input location (never the neighbour's column: nothing may merge, everything lands on two pixels)
      reverse   a reversed row (x0 decreases: the pending column is never the next left column)
      stride2   x0 advances by two per step
      sinus     a sinusoid that leaves and re-enters the image inside a run of eight: the tap flags flip mid-run and the pending column must still be flushed
    mode 1: the flow in pixels; mode 0: the same pixel coordinates as normalised values -- exact in fp32 where Wi, Hi are powers of two and the pixel
    coordinates multiples of 1/16"""
    ox = torch.arange(Wo, dtype=torch.float64).view(1, 1, Wo).expand(N, Ho, Wo)
    oy = torch.arange(Ho, dtype=torch.float64).view(1, Ho, 1).expand(N, Ho, Wo)
    nn = torch.arange(N, dtype=torch.float64).view(N, 1, 1).expand(N, Ho, Wo)
    if kind == "shift":
        sx, sy = ox + 0.3125 - 1, oy * 0.5 + 0.4375
    elif kind == "identity":
        sx, sy = ox.clone(), oy.clone()
    elif kind == "collapse":
        sx, sy = torch.full_like(ox, 2.25) + nn, oy * 0.25 + 0.5
    elif kind == "reverse":
        sx, sy = (Wi - 1) - ox + 0.25, oy + 0.125
    elif kind == "stride2":
        sx, sy = 2 * ox + 0.5, oy * 0.75 + 0.1875
    elif kind == "sinus":
        sx = ((Wi / 2 - 0.5) + (Wi / 2 + 1.5) * torch.sin(ox * (2 * math.pi / 5) + oy)).mul(16).round().div(16)
        sy = oy * 0.5 + 0.0625
    else:
        raise ValueError(kind)
    if mode == 0:
        g = torch.stack([(2 * sx + 1) / Wi - 1, (2 * sy + 1) / Hi - 1], dim=-1)
    else:
        g = torch.stack([sx - ox, sy - oy], dim=-1)
    return g.reshape(-1, 2).float()
