"""The normal-consistency regulariser of 2DGS, L_n = sum_i w_i (1 - n_i . N), as autograd operators over the fused HIP kernels
(csrc/normal_consistency.hip), either side of `diff_rasterize_features`:

    features = gaussian_surface_features(means, scales, rotations, w2c, cam_position)            # [N,5]: (n_cam, z, 1) per Gaussian
    image, surface_map = diff_rasterize_features(..., features=features)                         # [5,H,W]: (N_r, D, A), blended with the image's weights
    loss = loss + weight * normal_consistency(surface_map, rasterizer_settings).mean()

The normal of a Gaussian is the axis of its smallest scale, turned towards the camera; the surface normal N of a pixel comes from the rendered
expected-depth map D / A by finite differences of the back-projected points. Definitions: INTEGRATION.md 'Normal consistency'. Not part of the
reference's operator set, hence not in `_C`.
"""
from __future__ import annotations

import torch

from ._backend import RasterizerSettings, default_backend
from .rasterization import _require_gpu


class _SurfaceFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, w2c: torch.Tensor, cam_position: torch.Tensor) -> torch.Tensor:
        _require_gpu(means)
        features = default_backend().surface_features(means, scales, rotations, w2c, cam_position)
        ctx.save_for_backward(means, scales, rotations, w2c, cam_position)
        return features

    @staticmethod
    def backward(ctx, grad_features: torch.Tensor):
        means, scales, rotations, w2c, cam_position = ctx.saved_tensors
        need_means, _, need_rotations = ctx.needs_input_grad[:3]
        grad_rotations, grad_means = default_backend().surface_features_backward(means, scales, rotations, w2c, cam_position, grad_features.contiguous(),
                                                                                need_rotations=need_rotations, need_means=need_means)
        return grad_means, None, grad_rotations, None, None


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, surface_map: torch.Tensor, rasterizer_settings: RasterizerSettings, min_alpha: float, return_normals: bool):
        _require_gpu(surface_map)
        E, normals = default_backend().normal_consistency(surface_map, rasterizer_settings, min_alpha, return_normals)
        ctx.save_for_backward(surface_map)
        ctx.rasterizer_settings, ctx.min_alpha = rasterizer_settings, min_alpha
        if normals is None:
            return E
        ctx.mark_non_differentiable(normals)
        return E, normals

    @staticmethod
    def backward(ctx, grad_E: torch.Tensor, *_):
        surface_map, = ctx.saved_tensors
        grad_map = default_backend().normal_consistency_backward(surface_map, grad_E.contiguous(), ctx.rasterizer_settings, ctx.min_alpha)
        return grad_map, None, None, None


def gaussian_surface_features(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, w2c: torch.Tensor, cam_position: torch.Tensor) -> torch.Tensor:
    """[N,5] per-Gaussian channels (n_cam, z, 1) for `diff_rasterize_features`: n_cam = the axis of the smallest of the three log-`scales` (lowest index on
    a tie), as a column of the rotation of the raw quaternion `rotations` (r, x, y, z), turned towards the camera and taken to camera space with
    w2c[0:3,0:3]; z = the view-space depth of the mean. Differentiable in `rotations` (through the normalisation) and `means` (through z); the scales and
    the camera get no gradient. An input that does not require a gradient gets None and costs nothing. Tensors must be contiguous float32 on one device."""
    return _SurfaceFeatures.apply(means, scales, rotations, w2c, cam_position)


def normal_consistency(surface_map: torch.Tensor, rasterizer_settings: RasterizerSettings, min_alpha: float = 0.5, return_normals: bool = False):
    """E [H,W] of a blended map [5,H,W] = (N_r, D, A) (`diff_rasterize_features` over `gaussian_surface_features`): E = A - N_r . n_d = sum_i w_i (1 - n_i . n_d)
    where the depth normal n_d exists -- an interior pixel with A >= min_alpha at itself and its four neighbours -- and exactly 0, with exactly 0 gradient,
    elsewhere. n_d comes from the points ray(q) D(q) / A(q) of the four neighbours with the intrinsics of `rasterizer_settings`. Differentiable in the map
    (deterministically: no float atomics). return_normals=True: (E, n_d [3,H,W]), n_d for viewing: zeros where invalid, no gradient."""
    return _NormalConsistency.apply(surface_map, rasterizer_settings, float(min_alpha), bool(return_normals))
