"""FusedAdam for the HIP backend.

Public contract = the reference's optimizer (torch_bindings/adam.py:6-36): a `torch.optim.Adam` subclass constructed as
`FusedAdam(param_groups, lr, eps)`, ONE tensor per parameter group, moments created on first use, groups without a gradient
left untouched, `state[param]` holding `step` (int) / `exp_avg` / `exp_avg_sq` so that NeRFICG-style optimizer surgery
(extend / prune / sort of the moments) keeps working.

What differs is the execution: the reference issues one `adam_step` launch per group (6 per iteration); here every group that
has a gradient is collected first and the whole optimizer step is ONE `fgs_adam_step_multi` launch (up to 8 groups per launch).

Quiet blocks: a Gaussian whose moments are still exactly zero and whose gradient is zero is left as it is by an Adam step (for eps > 0). The optimizer
keeps one byte per block of 64 Gaussians, "both moments of the block are zero in every group", next to -- not in -- `state`, and hands it to the
kernel together with the rasterizer's reached-block flags: blocks that are quiet and were not reached are neither read nor written. The flags are
only as good as the optimizer's knowledge of the moments, so they carry a key: the moment tensors themselves (object, address, shape) and their
version counters. The library writes through raw pointers and leaves the counters alone; anything else (a replaced tensor, load_state_dict,
density control, a torch in-place edit, another N or set of groups) changes the key, and the flags are rebuilt by one scan of the moments.
"""
from __future__ import annotations

import weakref
from typing import Iterator, NamedTuple

import torch

from ._backend import default_backend
from .rasterization import clear_live_blocks, match_live_blocks, take_async_overflow

_GROUPS_PER_LAUNCH = 8          # AdamArgs::g[8] in csrc/fgs_kernels.h


class _Update(NamedTuple):
    grad: torch.Tensor
    param: torch.Tensor
    exp_avg: torch.Tensor
    exp_avg_sq: torch.Tensor
    step: int
    lr: float


class FusedAdam(torch.optim.Adam):
    def __init__(self, params, lr, eps) -> None:
        super().__init__(params=params, lr=lr, eps=eps)

    def _moments(self, tensor: torch.Tensor) -> dict:
        """Optimizer state of `tensor`, zero-initialised the first time it is stepped (adam.py:17-21 of the reference)."""
        entry = self.state[tensor]
        if not entry:
            entry.update(step=0, exp_avg=torch.zeros_like(tensor), exp_avg_sq=torch.zeros_like(tensor))
            self.__dict__.setdefault('_fresh_moments', set()).update((id(entry['exp_avg']), id(entry['exp_avg_sq'])))
        return entry

    @staticmethod
    def _moments_key(chunk: 'list[_Update]') -> tuple:
        moments = [t for u in chunk for t in (u.exp_avg, u.exp_avg_sq)]
        return tuple((t.data_ptr(), tuple(t.shape), t._version) for t in moments), tuple(weakref.ref(t) for t in moments)

    def quiet_blocks(self) -> 'torch.Tensor | None':
        """The per-block "both moments are zero" flags of the last step (uint8 [ceil(N / 64)]; 1 is a promise, 0 is none), or None if that step did
        not use them. Valid until somebody other than this optimizer writes the moments."""
        quiet = self.__dict__.get('_quiet')
        return None if quiet is None else quiet[0]

    def _quiet_for(self, chunk: 'list[_Update]', backend, fresh: set) -> torch.Tensor:
        """Flags that are true of the moments of `chunk` (all [N, ...] with one N) as they are now: the kept ones if the key still fits, all ones if
        every moment was created zero in this very step, else one scan."""
        (facts, refs), quiet = self._moments_key(chunk), self.__dict__.get('_quiet')
        moments = [t for u in chunk for t in (u.exp_avg, u.exp_avg_sq)]
        if quiet is not None and quiet[1] == facts and all(r() is t for r, t in zip(quiet[2], moments)):
            return quiet[0]
        n = chunk[0].param.shape[0]
        if all(id(t) in fresh for t in moments):
            flags = torch.ones((n + 63) // 64, dtype=torch.uint8, device=chunk[0].param.device)
        else:
            flags = backend.adam_quiet_scan([u.exp_avg for u in chunk], [u.exp_avg_sq for u in chunk])
        self._quiet = (flags, facts, refs)
        return flags

    def _pending(self) -> Iterator[tuple[tuple, _Update]]:
        """(launch key, update) for every group that has something to do this step."""
        for group in self.param_groups:
            tensors = group['params']
            if len(tensors) != 1:
                raise ValueError(f'FusedAdam expects one tensor per parameter group, group {group.get("name", "?")} has {len(tensors)}')
            tensor = tensors[0]
            gradient = tensor.grad
            if gradient is None or tensor.numel() == 0:
                continue
            moments = self._moments(tensor)
            moments['step'] += 1
            beta1, beta2 = group['betas']
            yield (float(beta1), float(beta2), float(group['eps']), tensor.device), _Update(
                gradient.contiguous(), tensor, moments['exp_avg'], moments['exp_avg_sq'], moments['step'], float(group['lr']))

    @torch.no_grad()
    def step(self) -> None:
        owned = [p for group in self.param_groups for p in group['params']]
        if take_async_overflow(owned):
            # the rasterizer's backward pass returned zeros because its (asynchronously sized) forward pass was truncated: stepping on them would
            # decay the moments, advance the step counts and move every parameter on momentum for a loss that was never evaluated. The mark names
            # the parameters of that pass: only the optimizer that owns them skips (and consumes the mark), any other FusedAdam steps normally
            clear_live_blocks(owned)
            return
        launches: dict[tuple, list[_Update]] = {}
        for key, update in self._pending():
            launches.setdefault(key, []).append(update)
        fresh = self.__dict__.pop('_fresh_moments', set())
        backend = default_backend()
        quiet_used = False
        for (beta1, beta2, eps, _device), updates in launches.items():
            for first in range(0, len(updates), _GROUPS_PER_LAUNCH):
                chunk = updates[first:first + _GROUPS_PER_LAUNCH]
                # gradients that are still exactly what the rasterizer's backward pass wrote come with its per-block "any reached" flags: the
                # zeros of blocks it reached no Gaussian of are not read back (rasterization.match_live_blocks; bit-identical result; gradient
                # reads fall to the reached blocks' share: ~0.04 of them in a dense opaque scene, 0.4-0.5 in a translucent one)
                live = match_live_blocks([u.grad for u in chunk], owned) if len(updates) <= _GROUPS_PER_LAUNCH else None
                # the quiet flags go along only with those flags (they say which blocks get a gradient), for ONE launch that covers every pending
                # group, all of them [N, ...]; the kernel clears the flag of every block it reads a gradient for. Any other step writes moments the
                # flags know nothing of: they are dropped, and the next step that qualifies scans
                n = chunk[0].param.shape[0] if chunk[0].param.dim() >= 1 else 0
                quiet = None
                if live is not None and len(launches) == 1 and n > 0 and all(u.param.dim() >= 1 and u.param.shape[0] == n for u in chunk):
                    quiet = self._quiet_for(chunk, backend, fresh)
                    quiet_used = True
                backend.adam_step_multi([u.grad for u in chunk], [u.param for u in chunk], [u.exp_avg for u in chunk],
                                        [u.exp_avg_sq for u in chunk], [u.step for u in chunk], [u.lr for u in chunk], beta1, beta2, eps,
                                        live_blocks=live, quiet_blocks=quiet)
        if launches and not quiet_used:
            self._quiet = None
        clear_live_blocks(owned)
