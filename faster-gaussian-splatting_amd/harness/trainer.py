"""Stand-in for the callers of the hot path that live in the un-vendored NeRFICG framework:

* `Gaussians`        -- the six nn.Parameters + FusedAdam groups/learning rates of Model.py:51-121, 232-260
* `extract_settings` -- View -> RasterizerSettings, field for field as Renderer.py:19-43
* `training_iteration` -- the per-iteration call order of Trainer.py:170-199
Learning rates are the garden configuration's (fastergs_garden.yaml:102-110). The loss is the reference's
0.8*L1 + 0.2*DSSIM (Trainer.py:52-53) through the fused HIP kernels of harness/loss.py (`fused_dssim` itself lives in the
un-vendored NeRFICG framework; see csrc/loss.hip for what is implemented instead).
"""
from __future__ import annotations

import math

import torch

from FasterGSCudaBackend import (FusedAdam, RasterizerSettings, diff_rasterize, diff_rasterize_absgrad, diff_rasterize_aux, diff_rasterize_distortion, diff_rasterize_features,
                                 diff_rasterize_geometry, gaussian_surface_features, normal_consistency, rasterize, rasterize_aux)

from .scenes import View

GARDEN_LR = {  # fastergs_garden.yaml:102-110
    'means_init': 1.6e-4, 'means_final': 1.6e-6, 'means_max_steps': 30_000,
    'sh_coefficients_0': 2.5e-3, 'sh_coefficients_rest': 1.25e-4, 'opacities': 2.5e-2, 'scales': 5.0e-3, 'rotations': 1.0e-3,
}
PARAM_ORDER = ('means', 'sh_coefficients_0', 'sh_coefficients_rest', 'opacities', 'scales', 'rotations')   # Model.py:238-245


def extract_settings(view: View, active_sh_bases: int, bg_color: torch.Tensor, proper_antialiasing: bool = False) -> RasterizerSettings:
    return RasterizerSettings(view.w2c, view.position, bg_color, active_sh_bases, view.width, view.height, view.focal_x,
                              view.focal_y, view.center_x, view.center_y, view.near_plane, view.far_plane, proper_antialiasing)


class Gaussians(torch.nn.Module):
    def __init__(self, params: dict, device, max_sh_degree: int = 3, active_sh_degree: int | None = None) -> None:
        super().__init__()
        for k in PARAM_ORDER:
            self.register_parameter(k, torch.nn.Parameter(params[k].to(device=device, dtype=torch.float32).contiguous()))
        self.max_sh_degree = max_sh_degree
        self.active_sh_degree = max_sh_degree if active_sh_degree is None else active_sh_degree
        self.densification_info = torch.zeros((2, self.means.shape[0]), dtype=torch.float32, device=device)   # Model.py:308-310
        self.abs_densification_info: 'torch.Tensor | None' = None      # the absolute-gradient statistic [2,N]: made by the first pass that accumulates it
        self.optimizer: FusedAdam | None = None
        self.extent = 1.0

    @property
    def active_sh_bases(self) -> int:
        return (self.active_sh_degree + 1) ** 2

    def increase_used_sh_degree(self) -> None:                      # Model.py:144-148, every 1 000 iterations (Trainer.py:114-118)
        self.active_sh_degree = min(self.active_sh_degree + 1, self.max_sh_degree)

    def training_setup(self, training_cameras_extent: float = 1.0, lr: dict = GARDEN_LR) -> None:   # Model.py:232-253
        self.extent, self._lr = training_cameras_extent, lr
        groups = [{'params': [getattr(self, k)], 'name': k,
                   'lr': lr['means_init'] * training_cameras_extent if k == 'means' else lr[k]} for k in PARAM_ORDER]
        self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)

    def update_learning_rate(self, iteration: int) -> None:         # Model.py:255-260 (log-linear decay of the means lr)
        lr = self._lr
        t = min(max(iteration / lr['means_max_steps'], 0.0), 1.0)
        lr_means = math.exp(math.log(lr['means_init'] * self.extent) * (1.0 - t) + math.log(lr['means_final'] * self.extent) * t)
        for g in self.optimizer.param_groups:
            if g['name'] == 'means':
                g['lr'] = lr_means

    def tensors(self):
        return self.means, self.scales, self.rotations, self.opacities, self.sh_coefficients_0, self.sh_coefficients_rest


def render_image_training(g: Gaussians, view: View, update_densification_info: bool, bg_color: torch.Tensor) -> torch.Tensor:
    """Renderer.py:72-86."""
    return diff_rasterize(*g.tensors(),
                          densification_info=g.densification_info if update_densification_info else torch.empty(0),
                          rasterizer_settings=extract_settings(view, g.active_sh_bases, bg_color))


def render_image_training_aux(g: Gaussians, view: View, update_densification_info: bool, bg_color: torch.Tensor, alpha: bool = True,
                              depth: bool = True):
    """render_image_training plus differentiable accumulated opacity and expected depth: (image, alpha or None, depth or None)."""
    return diff_rasterize_aux(*g.tensors(),
                              densification_info=g.densification_info if update_densification_info else torch.empty(0),
                              rasterizer_settings=extract_settings(view, g.active_sh_bases, bg_color), alpha=alpha, depth=depth)


def render_image_training_absgrad(g: Gaussians, view: View, update_densification_info: bool, bg_color: torch.Tensor, alpha: bool = False,
                                  depth: bool = False):
    """render_image_training_aux whose backward pass accumulates the ABSOLUTE-gradient statistic into g.abs_densification_info (made here, zeroed, if
    the model has none for its current size) instead of the signed one into g.densification_info, which is left alone: (image, alpha or None,
    depth or None), the maps only on request."""
    if update_densification_info and (g.abs_densification_info is None or g.abs_densification_info.shape[1] != g.means.shape[0]):
        g.abs_densification_info = torch.zeros((2, g.means.shape[0]), dtype=torch.float32, device=g.means.device)
    return diff_rasterize_absgrad(*g.tensors(), densification_info=torch.empty(0),
                                  rasterizer_settings=extract_settings(view, g.active_sh_bases, bg_color),
                                  abs_densification_info=g.abs_densification_info if update_densification_info else torch.empty(0), alpha=alpha, depth=depth)


def render_image_training_features(g: Gaussians, view: View, update_densification_info: bool, bg_color: torch.Tensor, features: torch.Tensor,
                                   detach_geometry: bool = False):
    """render_image_training plus the differentiable blend of per-Gaussian feature channels [N, F]: (image, feature_map [F,H,W])."""
    return diff_rasterize_features(*g.tensors(),
                                   densification_info=g.densification_info if update_densification_info else torch.empty(0),
                                   rasterizer_settings=extract_settings(view, g.active_sh_bases, bg_color), features=features,
                                   detach_geometry=detach_geometry)


def render_image_training_distortion(g: Gaussians, view: View, update_densification_info: bool, bg_color: torch.Tensor, normalized: bool = True):
    """render_image_training plus the differentiable depth-distortion map X = sum_ab w_a w_b |t_a - t_b| per pixel: (image, distortion [H,W])."""
    return diff_rasterize_distortion(*g.tensors(),
                                     densification_info=g.densification_info if update_densification_info else torch.empty(0),
                                     rasterizer_settings=extract_settings(view, g.active_sh_bases, bg_color), normalized=normalized)


def render_image_training_normals(g: Gaussians, view: View, update_densification_info: bool, bg_color: torch.Tensor, min_alpha: float = 0.5):
    """render_image_training plus the differentiable normal-consistency map E = sum_i w_i (1 - n_i . n_d) per pixel (0 where the rendered depth gives no
    normal): (image, E [H,W]). One diff_rasterize_features pass over the five surface channels (n_cam, z, 1) of gaussian_surface_features."""
    settings = extract_settings(view, g.active_sh_bases, bg_color)
    features = gaussian_surface_features(g.means, g.scales, g.rotations, view.w2c, view.position)
    image, surface_map = diff_rasterize_features(*g.tensors(),
                                                 densification_info=g.densification_info if update_densification_info else torch.empty(0),
                                                 rasterizer_settings=settings, features=features, detach_geometry=False)
    return image, normal_consistency(surface_map, settings, min_alpha=min_alpha)


def render_image_training_geometry(g: Gaussians, view: View, update_densification_info: bool, bg_color: torch.Tensor, normalized: bool = True,
                                   min_alpha: float = 0.5):
    """render_image_training plus every geometry term of 2DGS-style training from ONE diff_rasterize_geometry pass over the five surface channels of
    gaussian_surface_features: (image, distortion [H,W], E [H,W], alpha [H,W], depth [H,W]) -- the depth-distortion map of
    render_image_training_distortion, the normal-consistency map of render_image_training_normals, and the accumulated opacity and expected depth of
    render_image_training_aux (channels 4 and 3 of the surface map), all differentiable. A term the loss does not use costs nothing backward."""
    settings = extract_settings(view, g.active_sh_bases, bg_color)
    features = gaussian_surface_features(g.means, g.scales, g.rotations, view.w2c, view.position)
    image, distortion, surface_map = diff_rasterize_geometry(*g.tensors(),
                                                             densification_info=g.densification_info if update_densification_info else torch.empty(0),
                                                             rasterizer_settings=settings, surface_features=features, normalized=normalized)
    return image, distortion, normal_consistency(surface_map, settings, min_alpha=min_alpha), surface_map[4], surface_map[3]


def depth_l1_loss(alpha: torch.Tensor, depth: torch.Tensor, depth_target: torch.Tensor, valid: 'torch.Tensor | None' = None) -> torch.Tensor:
    """L1 between the mean depth D / A.clamp_min(1e-8) and the target over the valid pixels (default: target > 0)."""
    valid = depth_target > 0 if valid is None else valid
    diff = (depth / alpha.clamp_min(1e-8) - depth_target).abs()
    return (diff * valid).sum() / valid.sum().clamp_min(1)


@torch.inference_mode()
def render_image_benchmark(g: Gaussians, view: View, to_chw: bool = True) -> torch.Tensor:
    """Renderer.py:107-123."""
    return rasterize(*g.tensors(), rasterizer_settings=extract_settings(view, g.active_sh_bases, view.background_color),
                     to_chw=to_chw, clamp_output=True)


@torch.inference_mode()
def render_image_aux(g: Gaussians, view: View, to_chw: bool = True, alpha: bool = True, depth: 'str | None' = 'expected',
                     normalize_depth: bool = False) -> dict:
    """render_image_benchmark plus the accumulated-opacity and depth maps of the same blend (rasterize_aux): {'rgb', 'alpha', 'depth', 'depth_median'}."""
    return rasterize_aux(*g.tensors(), rasterizer_settings=extract_settings(view, g.active_sh_bases, view.background_color),
                         to_chw=to_chw, clamp_output=True, alpha=alpha, depth=depth, normalize_depth=normalize_depth)


def l1_loss(image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return (image - target).abs().mean()


def photometric_loss(image: torch.Tensor, target: torch.Tensor, weight: 'torch.Tensor | None' = None) -> torch.Tensor:
    """LAMBDA_L1 * L1 + LAMBDA_DSSIM * DSSIM with the garden weights 0.8 / 0.2 (fastergs_garden.yaml:98-99, Loss.py:15-16).
    weight: [H,W] mask or per-pixel confidence of the weighted loss (harness/loss.py); None is the unweighted one."""
    from .loss import l1_dssim_loss
    return l1_dssim_loss(image, target, 0.8, 0.2) if weight is None else l1_dssim_loss(image, target, 0.8, 0.2, weight=weight)


_UNIT = {}


def _unit_gradient(loss: torch.Tensor) -> torch.Tensor:
    """dL/dL = 1 as a tensor that already exists: `loss.backward()` allocates and fills one per call (a 5 us kernel on the critical path of a
    2 ms iteration; profiles/r05_kernel_sequence.txt). Nothing writes to it: autograd only reads the seed."""
    key = (loss.device, loss.dtype)
    one = _UNIT.get(key)
    if one is None:
        one = _UNIT[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
    return one


def training_iteration(g: Gaussians, view: View, target: torch.Tensor, iteration: int, *, densification_end: int = 14_900,
                       loss_scale: float = 1.0, before_step=None, loss_fn=photometric_loss, depth_target: 'torch.Tensor | None' = None,
                       depth_weight: float = 0.0, depth_valid: 'torch.Tensor | None' = None, absgrad: bool = False,
                       bilagrid=None, view_index: 'int | None' = None, tv_weight: float = 10.0,
                       loss_weight: 'torch.Tensor | None' = None, distortion_weight: float = 0.0,
                       distortion_normalized: bool = True, normal_weight: float = 0.0, normal_min_alpha: float = 0.5,
                       geometry_render: bool = False) -> torch.Tensor:
    """One optimisation step in the reference's order (Trainer.py:170-199): lr update -> render -> loss -> backward ->
    optimizer.step -> zero_grad. `before_step` (if given) runs between backward and step (gradient exchange hook).
    depth_target [H,W] with depth_weight > 0 adds depth_weight * L1(D / A, depth_target) over the valid pixels (depth_valid, default target > 0):
    depth supervision through diff_rasterize_aux. Off by default: the step is then exactly the colour-only one.
    absgrad: the densification statistic of the step is the absolute-gradient one (g.abs_densification_info, for a schedule with 'absgrad': True);
    g.densification_info is then not updated. Gradients and loss are the same either way.
    bilagrid (harness.bilagrid.BilateralGrids, after its training_setup) with view_index: the rendered image passes through that view's bilateral grid
    before loss_fn, tv_weight * the grid's total variation is added to the loss, and the module's optimizer steps behind the Gaussians'. None (the
    default): the step is exactly the one without.
    loss_weight [H,W]: a mask or per-pixel confidence handed to loss_fn as `weight=` on every branch (photometric_loss: the weighted L1 + DSSIM of
    harness/loss.py; with a bilagrid the corrected image is what gets weighted). None (the default): loss_fn is called as before.
    distortion_weight > 0 adds distortion_weight * distortion.mean(), the depth-distortion regulariser of diff_rasterize_distortion (t normalized onto
    [0, 1) with the view's planes unless distortion_normalized=False). Not together with depth supervision or absgrad. 0 (the default): the step is
    exactly the one without.
    normal_weight > 0 adds normal_weight * E.mean(), the normal-consistency regulariser of render_image_training_normals (pixels whose accumulated
    opacity, or a neighbour's, is below normal_min_alpha add nothing). Not together with the distortion term, depth supervision or absgrad: each is a
    different render. 0 (the default): the step is exactly the one without.
    geometry_render=True: the distortion term, the normal-consistency term and depth supervision may all be active in one call and all come from the
    ONE render of render_image_training_geometry: the loss is loss_fn's plus distortion_weight * distortion.mean(), normal_weight * E.mean() and
    depth_weight * depth_l1_loss(alpha, depth, ...), each where its weight is positive. Not together with absgrad. False (the default): nothing changes."""
    if geometry_render and absgrad:
        raise ValueError('training_iteration: the geometry render does not combine with absgrad in one render')
    if not geometry_render and distortion_weight > 0.0 and (absgrad or (depth_target is not None and depth_weight > 0.0)):
        raise ValueError('training_iteration: the distortion term does not combine with depth supervision or absgrad in one render')
    if not geometry_render and normal_weight > 0.0 and (distortion_weight > 0.0 or absgrad or (depth_target is not None and depth_weight > 0.0)):
        raise ValueError('training_iteration: the normal-consistency term does not combine with the distortion term, depth supervision or absgrad in one render')
    if bilagrid is not None:
        loss_fn = bilagrid.corrected(loss_fn, view_index, tv_weight)
    if loss_weight is not None:
        unweighted_fn = loss_fn
        loss_fn = lambda image, target: unweighted_fn(image, target, weight=loss_weight)
    g.update_learning_rate(iteration + 1)
    with_depth = depth_target is not None and depth_weight > 0.0
    if geometry_render:
        image, distortion, consistency, alpha, depth = render_image_training_geometry(
            g, view, update_densification_info=iteration < densification_end, bg_color=view.background_color, normalized=distortion_normalized,
            min_alpha=normal_min_alpha)
        loss = loss_fn(image, target)
        if distortion_weight > 0.0:
            loss = loss + distortion_weight * distortion.mean()
        if normal_weight > 0.0:
            loss = loss + normal_weight * consistency.mean()
        if with_depth:
            loss = loss + depth_weight * depth_l1_loss(alpha, depth, depth_target, depth_valid)
    elif absgrad:
        image, alpha, depth = render_image_training_absgrad(g, view, update_densification_info=iteration < densification_end, bg_color=view.background_color,
                                                            alpha=with_depth, depth=with_depth)
        loss = loss_fn(image, target) + depth_weight * depth_l1_loss(alpha, depth, depth_target, depth_valid) if with_depth else loss_fn(image, target)
    elif with_depth:
        image, alpha, depth = render_image_training_aux(g, view, update_densification_info=iteration < densification_end, bg_color=view.background_color)
        loss = loss_fn(image, target) + depth_weight * depth_l1_loss(alpha, depth, depth_target, depth_valid)
    elif distortion_weight > 0.0:
        image, distortion = render_image_training_distortion(g, view, update_densification_info=iteration < densification_end,
                                                             bg_color=view.background_color, normalized=distortion_normalized)
        loss = loss_fn(image, target) + distortion_weight * distortion.mean()
    elif normal_weight > 0.0:
        image, consistency = render_image_training_normals(g, view, update_densification_info=iteration < densification_end,
                                                           bg_color=view.background_color, min_alpha=normal_min_alpha)
        loss = loss_fn(image, target) + normal_weight * consistency.mean()
    else:
        image = render_image_training(g, view, update_densification_info=iteration < densification_end, bg_color=view.background_color)
        loss = loss_fn(image, target)
    if loss_scale != 1.0:                 # (two elementwise launches per iteration otherwise)
        loss = loss * loss_scale
    loss.backward(gradient=_unit_gradient(loss))          # = loss.backward() without the fill kernel that seeds it every iteration
    if before_step is not None:
        before_step()
    g.optimizer.step()
    g.optimizer.zero_grad()
    if bilagrid is not None:
        bilagrid.optimizer.step()
        bilagrid.optimizer.zero_grad()
    return loss.detach()


def render_image_corrected(g: Gaussians, view: View, grids, view_index: int) -> torch.Tensor:
    """The inference render of a training view with its photometric correction, in the reference's order (Renderer.py:101-104): rasterize without the
    clamp -> the view's bilateral grid -> clamp to [0, 1]. [3,H,W]."""
    with torch.no_grad():
        image = rasterize(*g.tensors(), rasterizer_settings=extract_settings(view, g.active_sh_bases, view.background_color), to_chw=True, clamp_output=False)
        return grids(image, view_index).clamp_(0.0, 1.0)
