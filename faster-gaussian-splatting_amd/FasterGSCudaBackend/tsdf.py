"""Surface extraction over the fused HIP kernels of csrc/tsdf.hip: rendered depth maps are fused into a dense truncated-signed-distance volume and the
zero level set is extracted as an indexed, welded triangle mesh (marching tetrahedra on the Kuhn split; definitions: include/fgs_hip.h).

A volume is two tensors on one device: `tsdf_weight` float32 [nz, ny, nx, 2] (tsdf in [-1, 1], accumulated weight) and, optionally, `color` float32
PLANAR [3, nz, ny, nx]; zeros are an empty volume. Lattice point (i, j, k) lies at origin + voxel_size * (i, j, k). No gradients flow through either
operator. Not part of the reference's operator set (its pipelines leave the GPU for this step), hence not in `_C`.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _lib
from ._backend import RasterizerSettings, default_backend
from .rasterization import _require_gpu


@torch.no_grad()
def tsdf_integrate(tsdf_weight: torch.Tensor, color: Optional[torch.Tensor], origin: Sequence[float], voxel_size: float, trunc: float,
                   settings_list: Sequence[RasterizerSettings], depths: Sequence[torch.Tensor], alphas: Optional[Sequence[torch.Tensor]] = None,
                   colors: Optional[Sequence[torch.Tensor]] = None, near: Optional[float] = None, depth_max: float = math.inf, min_alpha: float = 0.5,
                   max_weight: float = 65536.0) -> None:
    """Folds views into the volume IN PLACE, in list order, eight per launch. Per view: its RasterizerSettings (w2c, intrinsics, size: all views one size),
    a depth map [H, W] of view-space z (`rasterize_aux`'s 'depth_median', or 'depth' with normalize_depth=True), optionally an opacity map [H, W] (pixels
    below `min_alpha` are skipped) and a colour map [3, H, W] (required when the volume has colour). trunc is in world units; near: None = the first
    view's near plane. Splitting the list differently gives the same bits."""
    _require_gpu(tsdf_weight)
    if len(settings_list) == 0:
        raise ValueError('tsdf_integrate: no views')
    near = float(settings_list[0].near_plane) if near is None else float(near)
    be, step = default_backend(), _lib.TSDF_MAX_VIEWS
    for first in range(0, len(settings_list), step):
        cut = slice(first, first + step)
        be.tsdf_integrate(tsdf_weight, color, origin, voxel_size, trunc, settings_list[cut], depths[cut], None if alphas is None else alphas[cut],
                          None if colors is None else colors[cut], near, depth_max, min_alpha, max_weight)


@torch.no_grad()
def tsdf_extract_mesh(tsdf_weight: torch.Tensor, color: Optional[torch.Tensor], origin: Sequence[float], voxel_size: float, iso: float = 0.0,
                      min_weight: float = 1.0) -> tuple:
    """(vertices [Nv, 3] float32, faces [Nf, 3] int32, colors [Nv, 3] float32 or None) of the level set {tsdf = iso} over the cubes whose eight corners have
    weight >= min_weight. Shared vertices are shared by index; the mesh is closed wherever the valid region is; normals point from tsdf < iso to tsdf >= iso.
    Zero-area triangles (a corner exactly at iso) are kept. An empty result has Nv = Nf = 0. One host synchronisation (the sizes)."""
    _require_gpu(tsdf_weight)
    return default_backend().tsdf_extract_mesh(tsdf_weight, color, origin, voxel_size, iso, min_weight)
