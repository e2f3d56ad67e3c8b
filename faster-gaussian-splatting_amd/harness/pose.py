"""Camera-pose refinement through the rasterizer's pose gradients (diff_rasterize_pose): correcting a noisy pose of a view against a fixed model --
SfM clean-up, registering a new view, a tracking step.

* `PoseDelta`   -- a 6-DoF correction (axis-angle + translation, zero = identity) composed onto a view's w2c IN THE CAMERA FRAME:
                   w2c' = [exp(omega^) | tau] w2c. Returns (w2c', cam_position') with cam_position' = -R'^T t', both differentiable.
* `refine_pose` -- torch Adam on a PoseDelta, L1 image loss against a target image; the Gaussians stay fixed.
"""
from __future__ import annotations

import torch

from FasterGSCudaBackend import diff_rasterize_pose

from .scenes import View
from .trainer import Gaussians, extract_settings


def _skew(v: torch.Tensor) -> torch.Tensor:
    zero = torch.zeros((), dtype=v.dtype, device=v.device)
    return torch.stack([torch.stack([zero, -v[2], v[1]]), torch.stack([v[2], zero, -v[0]]), torch.stack([-v[1], v[0], zero])])


class PoseDelta(torch.nn.Module):
    def __init__(self, device='cpu') -> None:
        super().__init__()
        self.rotation = torch.nn.Parameter(torch.zeros(3, dtype=torch.float32, device=device))       # axis-angle, radians
        self.translation = torch.nn.Parameter(torch.zeros(3, dtype=torch.float32, device=device))    # camera-space units

    def forward(self, w2c: torch.Tensor) -> tuple:
        """w2c [4,4] or [3,4] -> (corrected w2c of the same shape, its camera position [3])."""
        R = torch.linalg.matrix_exp(_skew(self.rotation))          # smooth at zero, unlike the closed Rodrigues form
        top = torch.cat([R @ w2c[:3, :3], (R @ w2c[:3, 3] + self.translation)[:, None]], dim=1)
        out = top if w2c.shape[0] == 3 else torch.cat([top, w2c[3:4]])
        return out, -top[:, :3].T @ top[:, 3]


def pose_error(w2c: torch.Tensor, w2c_true: torch.Tensor) -> tuple:
    """(rotation angle between the two poses in radians, distance between the two camera positions)."""
    a, b = w2c.detach().double().cpu(), w2c_true.detach().double().cpu()
    cos = ((a[:3, :3] @ b[:3, :3].T).trace() - 1.0) / 2.0
    pos = lambda m: -m[:3, :3].T @ m[:3, 3]
    return float(torch.acos(cos.clamp(-1.0, 1.0))), float((pos(a) - pos(b)).norm())


def refine_pose(gaussians: Gaussians, view: View, target: torch.Tensor, steps: int = 40, lr: float = 2e-3, delta: 'PoseDelta | None' = None) -> tuple:
    """`steps` Adam steps on a PoseDelta (a new one at zero unless given) over view.w2c, minimising mean |image - target|. Returns (delta, losses);
    delta(view.w2c) is the refined pose."""
    delta = PoseDelta(view.w2c.device) if delta is None else delta
    optimizer = torch.optim.Adam(delta.parameters(), lr=lr)
    settings = extract_settings(view, gaussians.active_sh_bases, view.background_color)
    params = [t.detach() for t in gaussians.tensors()]
    losses = []
    for _ in range(steps):
        w2c, cam_position = delta(view.w2c)
        image, _, _ = diff_rasterize_pose(*params, torch.empty(0), settings, w2c=w2c, cam_position=cam_position)
        loss = (image - target).abs().mean()
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        losses.append(float(loss.detach()))
    return delta, losses
