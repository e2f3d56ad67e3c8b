"""Per-view bilateral grids: the harness's handling of photometric variation between training images (exposure, white balance, vignetting).

The reference sends every training, inference and benchmark render through a per-view photometric module of the un-vendored NeRFICG framework
(Renderer.py:84-85, 101-104, 119-122). That module cannot be restated here; this is the per-view affine colour transform of "Bilateral Guided Radiance
Field Processing" (the `bilagrid` of gsplat's trainer) in its place: one grid of 3 x 4 colour matrices per training view, sliced per pixel at
(x, y, luma) by FasterGSCudaBackend.bilagrid_slice, regularised by its total variation.
"""
from __future__ import annotations

import torch

from FasterGSCudaBackend import bilagrid_slice, bilagrid_tv_loss


class BilateralGrids(torch.nn.Module):
    """One [12, L, Hg, Wg] grid per view, each initialised to the identity transform [I | 0]. shape = (Wg, Hg, L)."""

    def __init__(self, n_views: int, shape: tuple = (16, 16, 8), device='cuda') -> None:
        super().__init__()
        gw, gh, gl = (int(s) for s in shape)
        if n_views < 1 or min(gw, gh, gl) < 1:
            raise ValueError(f'BilateralGrids needs at least one view and positive extents, got {n_views} views of {shape}')
        identity = torch.zeros(12, gl, gh, gw, dtype=torch.float32)
        identity[[0, 5, 10]] = 1.0                                      # entries (0, 0), (1, 1), (2, 2) of [A | b]
        self.shape = (gw, gh, gl)
        self.grids = torch.nn.ParameterList([torch.nn.Parameter(identity.clone().to(device)) for _ in range(n_views)])
        self.optimizer: 'torch.optim.Adam | None' = None

    def forward(self, image: torch.Tensor, view_index: int) -> torch.Tensor:
        """The rendered image [3,H,W] (unclamped) through the grid of view `view_index`."""
        return bilagrid_slice(image.contiguous(), self.grids[view_index])

    def tv(self, view_index: int) -> torch.Tensor:
        """Total variation of the grid of view `view_index` (a scalar)."""
        return bilagrid_tv_loss(self.grids[view_index])

    def training_setup(self, lr: float = 2e-3) -> None:
        """A torch Adam over the grids (lr 2e-3 and eps 1e-15 are gsplat's values; they have not been validated here). An iteration renders ONE view, so
        only that view's grid has a gradient when the optimizer steps: torch's Adam skips parameters whose gradient is None, i.e. a view's grid -- its
        moments and its step count -- is stepped only in the iterations that saw it."""
        self.optimizer = torch.optim.Adam(list(self.grids), lr=lr, eps=1e-15)

    def corrected(self, loss_fn, view_index: int, tv_weight: float):
        """loss_fn over the corrected image plus the weighted total variation of that view's grid: what training_iteration minimises with a module.
        Keyword arguments (the per-pixel `weight` of photometric_loss) go through to loss_fn: the CORRECTED image is what gets weighted."""
        return lambda image, target, **kw: loss_fn(self(image, view_index), target, **kw) + tv_weight * self.tv(view_index)

    # ---- checkpoints (harness/checkpoint.py): tensors and plain containers only ----
    @torch.no_grad()
    def checkpoint_state(self) -> dict:
        state = {'shape': list(self.shape), 'grids': [g.detach().cpu() for g in self.grids], 'optimizer': None}
        if self.optimizer is not None:
            moments = []
            for g in self.grids:
                st = self.optimizer.state.get(g, {})
                moments.append(None if not st else {'step': torch.as_tensor(st['step']).detach().cpu(), 'exp_avg': st['exp_avg'].cpu(), 'exp_avg_sq': st['exp_avg_sq'].cpu()})
            state['optimizer'] = {'lr': self.optimizer.param_groups[0]['lr'], 'moments': moments}
        return state

    @torch.no_grad()
    def load_checkpoint_state(self, state: dict) -> None:
        if tuple(state['shape']) != self.shape or len(state['grids']) != len(self.grids):
            raise ValueError(f'checkpoint holds {len(state["grids"])} grids of {tuple(state["shape"])}, the module {len(self.grids)} of {self.shape}')
        for g, saved in zip(self.grids, state['grids']):
            g.copy_(saved.to(g.device))
        if state['optimizer'] is not None:
            self.training_setup(lr=state['optimizer']['lr'])
            for g, saved in zip(self.grids, state['optimizer']['moments']):
                if saved is not None:
                    self.optimizer.state[g] = {'step': saved['step'].clone(), 'exp_avg': saved['exp_avg'].to(g.device).contiguous(),
                                               'exp_avg_sq': saved['exp_avg_sq'].to(g.device).contiguous()}
