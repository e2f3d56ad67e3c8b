"""Photometric loss of the training iteration: 0.8 * L1 + 0.2 * DSSIM (Trainer.py:52-53,190-193; Loss.py:15-16), as ONE
autograd node backed by the fused HIP kernels (csrc/loss.hip): forward launches the SSIM pass and keeps its derivative maps, backward
launches the gradient kernel with the upstream scalar folded in (a device read: no host sync, no `grad * upstream` pass over the image).
With a per-pixel `weight` (masks, confidences) the same node runs the weighted kernels (INTEGRATION.md 'Weighted loss')."""
from __future__ import annotations

from typing import Optional

import torch

from FasterGSCudaBackend._backend import default_backend


class _L1DSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image: torch.Tensor, target: torch.Tensor, lambda_l1: float, lambda_dssim: float, weight: Optional[torch.Tensor]) -> torch.Tensor:
        image, target = image.contiguous(), target.contiguous()
        if weight is None:
            loss, _, scratch = default_backend().l1_dssim_forward(image, target, lambda_l1, lambda_dssim)
            ctx.save_for_backward(image, target, scratch)
        else:
            loss, _, scratch = default_backend().l1_dssim_forward(image, target, lambda_l1, lambda_dssim, weight=weight)
            ctx.save_for_backward(image, target, scratch, weight)
        ctx.lambdas = (lambda_l1, lambda_dssim)
        return loss

    @staticmethod
    def backward(ctx, grad_loss: torch.Tensor):
        image, target, scratch, *weight = ctx.saved_tensors
        upstream = grad_loss.to(dtype=torch.float32, device=image.device)
        if not weight:
            return default_backend().l1_dssim_backward(image, target, scratch, upstream, *ctx.lambdas), None, None, None, None
        return default_backend().l1_dssim_backward(image, target, scratch, upstream, *ctx.lambdas, weight=weight[0]), None, None, None, None


def l1_dssim_loss(image: torch.Tensor, target: torch.Tensor, lambda_l1: float = 0.8, lambda_dssim: float = 0.2,
                  weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lambda_l1 * L1 + lambda_dssim * (1 - SSIM) of two [3,H,W] images. `weight`: [H,W] on the image's device, one weight per pixel shared by the
    channels -- a bool or integer mask (converted to float32 here) or float confidences. A weight > 0 counts as it is, anything else (0, negative,
    NaN) as 0; pixels that do not count are replaced by the target before the SSIM windows are formed, their gradient is exactly 0, and both means
    are taken over the total weight (all zero: loss 0). The weight is NOT differentiable: it gets no gradient (None), whatever its requires_grad."""
    if weight is not None:
        if not isinstance(weight, torch.Tensor):
            raise RuntimeError(f'l1_dssim_loss: weight must be a tensor, got {type(weight).__name__}')
        weight = weight.detach()
        if weight.dtype != torch.float32 and not weight.is_complex():
            weight = weight.to(torch.float32)
        weight = weight.contiguous()
    return _L1DSSIM.apply(image, target, lambda_l1, lambda_dssim, weight)
