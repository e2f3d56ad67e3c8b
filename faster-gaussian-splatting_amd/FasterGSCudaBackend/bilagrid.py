"""Per-view bilateral-grid colour correction as autograd operators over the fused HIP kernels (csrc/bilagrid.hip).

A grid is a float32 [12, L, Hg, Wg] tensor: a 3 x 4 affine colour matrix [A | b] per lattice point (channel 4 i + j = entry (i, j)). `bilagrid_slice`
reads a matrix per pixel by trilinear interpolation at (x, y, luma) and applies it -- F.grid_sample(grid[None], 2 (x, y, luma) - 1, 'bilinear',
align_corners=True, padding_mode='border') followed by the matrix product, in one kernel each way. `bilagrid_tv_loss` is the total-variation
regulariser of one grid. Not part of the reference's operator set (its photometric module lives in an un-vendored framework), hence not in `_C`.
"""
from __future__ import annotations

import torch

from ._backend import default_backend
from .rasterization import _require_gpu


class _BilagridSlice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
        _require_gpu(image)
        out = default_backend().bilagrid_slice(image, grid)
        ctx.save_for_backward(image, grid)
        return out

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        image, grid = ctx.saved_tensors
        need_image, need_grid = ctx.needs_input_grad
        grad_grid, grad_image = default_backend().bilagrid_slice_backward(image, grid, grad_out.contiguous(), need_grid=need_grid, need_image=need_image)
        return grad_image, grad_grid


class _BilagridTV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid: torch.Tensor) -> torch.Tensor:
        _require_gpu(grid)
        loss, grad = default_backend().bilagrid_tv(grid, with_grad=ctx.needs_input_grad[0])      # the forward launch keeps the gradient
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_loss: torch.Tensor):
        grad, = ctx.saved_tensors
        return grad * grad_loss.to(dtype=grad.dtype, device=grad.device)


def bilagrid_slice(image: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """image [3,H,W] (float32, any range) through the per-pixel affine colour transform of `grid` [12, L, Hg, Wg]: [3,H,W]. Differentiable in both;
    an input that does not require a gradient gets None and costs nothing in the backward kernel. Tensors must be contiguous float32 on one device."""
    return _BilagridSlice.apply(image, grid)


def bilagrid_tv_loss(grid: torch.Tensor) -> torch.Tensor:
    """Total variation of one grid [12, L, Hg, Wg]: sum over the axes z, y, x of mean((G[next] - G)^2) over all 12 channels (an axis of extent 1 adds 0)."""
    return _BilagridTV.apply(grid)
