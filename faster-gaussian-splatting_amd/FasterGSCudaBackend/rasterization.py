"""Operator surface of the rasterizer: diff_rasterize / rasterize / RasterizerSettings.

Names, argument order and semantics follow the reference's torch_bindings/rasterization.py:41-156 so that
Renderer.py:72-123 runs unmodified against this package; the implementation underneath is libfgs_hip.so through ctypes.
"""
from __future__ import annotations

import math
import warnings
import weakref
from typing import Any

import torch
from torch.autograd.function import once_differentiable

from ._backend import RasterizerSettings, default_backend, gradient_shapes, total_sh_rest


_GRAD_OUT = None   # optional provider of preallocated gradient tensors (harness/distributed.py packs them into one arena)


def set_gradient_buffers(provider) -> None:
    """provider() -> six tensors (means, scales, rotations, opacities, sh0, sh_rest order) or None; None resets."""
    global _GRAD_OUT
    _GRAD_OUT = provider


# ---- host-synchronisation-free training forward (fgs_forward_async) ------------------------------------------------------------------
# The reference blocks the host three times per forward pass (forward.cu:100,102,234) to size its buffers; fgs_forward once. With
# `set_async_forward(True)` the training path sizes the instance stages from what an earlier pass OF THE SAME VIEW needed -- that view's
# instances-per-Gaussian ratio x the current Gaussian count x `headroom` -- and reads the counts back asynchronously; they are looked at in
# `backward` (by then the copy has long completed). A view that has not been seen yet, and any pass that does not need gradients
# (torch.no_grad(), detached inputs: nobody would ever look at the counts), takes the synchronous path -- a ratio borrowed from other views
# overflows in the first epoch (round-2 advisor finding). A view is recognised by the IDENTITY of its w2c tensor (address + a weak reference to
# the tensor object + its version counter, plus image size and intrinsics): an address the caching allocator hands to another tensor, or a w2c
# edited in place, is a new view, never a cache hit (round-3 advisor finding); a training loop that builds a fresh w2c every iteration therefore
# stays synchronous -- correct, only without the saving. The table is bounded (least recently used views are dropped).
# If a pass still needs more than its capacity (the instance count of one view jumped by more than the headroom between two of its visits), its
# image and therefore the loss gradient were incomplete: backward reports it (RuntimeWarning), refreshes the view's ratio, returns ZERO gradients
# (written into the caller's gradient buffers when a provider is set; densification_info is left alone) and marks the step invalid:
# `FusedAdam.step` consumes that mark and skips the step -- no moment decay, no step count, no parameter motion on momentum (any other optimizer
# can ask `take_async_overflow()`). A pass that asked for gradients but whose backward never runs (an evaluation loop without no_grad) is checked
# lazily by the next forward pass, which warns if that image was truncated.
# Scopes: the per-view table records instances PER GAUSSIAN, a property of the model as much as of the view. A process that trains two models over
# the same view tensors gives each its own table with `async_forward_scope(name)` (a context manager around that model's iterations); everything
# outside such a block uses the default scope. Switches (`set_async_forward`) and counters are per scope as well.
def _new_async_table() -> dict:
    return {'enabled': False, 'headroom': 1.25, 'ratio': 0.0, 'overflows': 0, 'per_view': {}, 'pending': {}, 'step_invalid': False, 'ticket': 0}


_ASYNC_SCOPES = {None: _new_async_table()}
_ASYNC = _ASYNC_SCOPES[None]          # the ACTIVE scope's table (rebound by async_forward_scope)
_ASYNC_MAX_VIEWS = 1024


class async_forward_scope:
    """`with async_forward_scope('model_b'): ...` -- the asynchronous-forward bookkeeping (switch, per-view ratios, pending checks, overflow mark) of
    the block is kept apart from every other scope's. Scopes persist across blocks of the same name; `async_forward_scope.drop(name)` forgets one."""

    def __init__(self, name):
        self.name, self._outer = name, None

    def __enter__(self):
        global _ASYNC
        self._outer = _ASYNC
        _ASYNC = _ASYNC_SCOPES.setdefault(self.name, _new_async_table())
        return self

    def __exit__(self, *exc):
        global _ASYNC
        _ASYNC = self._outer

    @staticmethod
    def drop(name) -> None:
        if name is not None:
            _ASYNC_SCOPES.pop(name, None)

# ---- live-block hand-over from this backward pass to FusedAdam.step ------------------------------------------------------------------
# Most gradient rows of a pass are zeros that the backward pass writes (the gradient tensors are dense and valid for any reader) and the optimizer
# reads back: one third of the Gaussians is invisible in a view, and of the visible ones the backward blend pass reaches only those that are not
# hidden behind opaque ones (1 % of them in a dense opaque scene, 40-50 % in a translucent one). The backward pass leaves two bytes per block of
# 64 Gaussians, "any visible" and "any reached" (fgs_backward_reached), and this registry hands the REACHED array to FusedAdam.step, which skips
# READING the gradients of blocks flagged 0 -- 0.96 of all blocks in the dense scene, 0.5-0.6 in the translucent one -- if, and only if, the
# gradients it is handed are still exactly what this backward pass wrote. That is established without trusting anybody: the six gradients are views
# into ONE arena that this registry keeps alive (their addresses cannot be re-used by another tensor while registered).
# The registry holds the ARENA and the views' addresses / shapes, never
# the view tensors themselves: autograd adopts an incoming gradient as `.grad` only if nobody else references that tensor (it looks at the
# reference count of the view, not of its storage) and clones it otherwise -- 708 MB per iteration at 3 M Gaussians. A match needs the same address, the same shape and an unchanged version counter (views share the arena's: any
# in-place edit -- accumulation of a second backward, clipping, scaling -- shows). Anything else takes the ordinary path; results are
# bit-identical either way. Writes the version counter does not see (`.grad.data.add_(...)`, raw pointers) are the kernel's business: it reads
# one sentinel float per flagged-0 block and tensor and, unless that is +-0, the block's gradients after all (csrc/adam.hip).
# The registry holds ONE registration per model, keyed by the address of the `means` tensor of the pass (two models in one process do not evict
# each other's registration; a model's next backward pass replaces its own). An optimizer names the parameters it owns when it asks.
_LIVE = {'enabled': True, 'slots': {}, 'matched': 0, 'missed': 0}
_LIVE_MAX_SLOTS = 8
_ALIGN_FLOATS = 64          # every gradient starts on a 256-byte boundary (16-byte loads in the optimizer kernel)


def set_live_block_handover(enabled: bool) -> None:
    _LIVE['enabled'] = bool(enabled)
    clear_live_blocks()


def live_block_stats() -> dict:
    return {'matched': _LIVE['matched'], 'missed': _LIVE['missed']}


def clear_live_blocks(owned=None) -> None:
    """Forgets the registrations of the passes over the given parameter tensors (an optimizer's own), or all of them (and every spare arena)."""
    if owned is None:
        _LIVE['slots'].clear()
        _RECYCLE['spares'].clear()
        return
    for t in owned:
        _retire(_LIVE['slots'].pop(t.data_ptr(), None))


def _gradient_arena(shapes, device, arena=None):
    """One arena and the six gradient tensors as views into it; `arena`: a spare of exactly these shapes (the layout is a function of the shapes)."""
    numels = [math.prod(sh) for sh in shapes]
    offsets, total = [], 0
    for numel in numels:
        offsets.append(total)
        total += (numel + _ALIGN_FLOATS - 1) // _ALIGN_FLOATS * _ALIGN_FLOATS
    if arena is None:
        arena = torch.empty(max(total, 1), dtype=torch.float32, device=device)
    return arena, tuple(arena[off:off + numel].view(sh) for sh, off, numel in zip(shapes, offsets, numels))


# ---- the arena of the previous pass, used again -----------------------------------------------------------------------------------------
# A new arena has to be written in full, 236 bytes per Gaussian, although in a dense scene all but a few per cent of its blocks get zeros that nobody
# reads (the optimizer looks at the flags and at one sentinel float per block). The zeros only have to be written because the memory is new: in the arena
# of the previous pass a block that was zero then and is unreached again is already correct. So an arena that leaves the registry above -- consumed by
# match_live_blocks, or forgotten by clear_live_blocks(owned) -- is kept as a SPARE together with the version counter recorded for it and the
# `reached_blocks` array its pass wrote, and the next backward pass over tensors of the same shapes on the same device writes into it, handing those flags
# to the kernel as `prior_blocks` (fgs_backward_recycled): "0 = this block is zero now". The invariant is about the arena's content, not about whose
# gradients it held, so spares are keyed by device and shapes: a second model of the same shapes may take the first one's.
# A spare is used only if nobody can tell: its version counter is what was recorded (no torch-visible in-place edit since its pass: the accumulation of
# a second backward, clipping, zero_grad(set_to_none=False)), and nobody else references its storage -- a `.grad` still alive, a kept alias of one
# (`.detach()`, `.view(-1)`): a gradient somebody still holds never changes under them. The storage's reference count is compared with that of a newly
# made tensor; the call that reads it is private torch API, and without it nothing is ever recycled. A write behind the version counter
# (`.grad.data.add_(...)`) is the kernel's business, as it is for the optimizer: it looks at the first element of the block in each tensor and writes
# the block unless all six are zero. Otherwise the pass takes new memory exactly as before, with no promise. Bit-identical results either way.
# Cost: one arena stays allocated through the next forward pass (0.71 GB at 3 M Gaussians); set_gradient_recycling(False) gives it back.
_RECYCLE = {'enabled': True, 'spares': {}, 'recycled': 0, 'fresh': 0, 'baseline': {}}
_RECYCLE_MAX_SPARES = 2
_STORAGE_USE_COUNT = getattr(torch._C, '_storage_Use_Count', None)


def set_gradient_recycling(enabled: bool) -> None:
    _RECYCLE['enabled'] = bool(enabled)
    _RECYCLE['spares'].clear()


def gradient_recycling_stats() -> dict:
    """Backward passes of the hand-over path that wrote into the previous pass's arena / that took new memory."""
    return {'recycled': _RECYCLE['recycled'], 'fresh': _RECYCLE['fresh']}


def _storage_references(t: torch.Tensor) -> int:
    return _STORAGE_USE_COUNT(t.untyped_storage()._cdata)


def _retire(slot) -> None:
    """A registration that leaves the registry: its arena becomes the spare of its device and shapes (one per key, the newest; a few overall)."""
    if slot is None or not _RECYCLE['enabled'] or _STORAGE_USE_COUNT is None:
        return
    spares, arena = _RECYCLE['spares'], slot['arena']
    key = (arena.device, tuple(shape for _, shape in slot['views']))
    spares.pop(key, None)
    spares[key] = {'arena': arena, 'version': slot['version'], 'flags': slot['flags']}
    while len(spares) > _RECYCLE_MAX_SPARES:
        del spares[next(iter(spares))]


def _take_spare(shapes, device):
    """The spare for these shapes if it may be written into (see above), else None; the spare leaves the table either way."""
    spare = _RECYCLE['spares'].pop((device, tuple(tuple(sh) for sh in shapes)), None)
    if spare is None or not _RECYCLE['enabled'] or _STORAGE_USE_COUNT is None:
        return None
    if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():      # a replayed pass would repeat a promise that was true once
        return None
    arena = spare['arena']
    baseline = _RECYCLE['baseline'].get(device.type)
    if baseline is None:
        baseline = _RECYCLE['baseline'][device.type] = _storage_references(torch.empty(1, dtype=torch.float32, device=device))
    if arena._version != spare['version'] or _storage_references(arena) != baseline:
        return None
    return spare


def match_live_blocks(gradients, owned=None) -> 'torch.Tensor | None':
    """The flags of a registered backward pass if `gradients` (the tensors an optimizer is about to consume, one per parameter group) are
    exactly the tensors it wrote -- same addresses, shapes, untouched since -- else None. `owned`: the optimizer's parameter tensors; only the
    registration of a pass over one of them is looked at (and consumed either way). Without it every registration is a candidate."""
    slots = _LIVE['slots']
    keys = list(slots) if owned is None else [t.data_ptr() for t in owned if t.data_ptr() in slots]
    if not keys or len(gradients) == 0:
        return None
    first = gradients[0].data_ptr()
    key = next((k for k in keys if any(address == first for address, _ in slots[k]['views'])), keys[0])
    slot = slots.pop(key)
    _retire(slot)
    arena, flags, views, version = slot['arena'], slot['flags'], slot['views'], slot['version']
    by_address = {address: shape for address, shape in views if address != 0}
    seen = set()
    for g in gradients:
        shape = by_address.get(g.data_ptr())
        if (shape is None or g.data_ptr() in seen or tuple(g.shape) != shape or g.dtype != torch.float32 or not g.is_contiguous()
                or g.device != arena.device or g._version != version):
            _LIVE['missed'] += 1
            return None
        seen.add(g.data_ptr())
    _LIVE['matched'] += 1
    return flags


def set_async_forward(enabled: bool, headroom: float = 1.25) -> None:
    _ASYNC.update(enabled=bool(enabled), headroom=float(headroom))
    if not enabled:
        _ASYNC.update(ratio=0.0, per_view={}, pending={}, step_invalid=False)


def async_forward_stats() -> dict:
    """'ratio': the largest instances-per-Gaussian ratio of any view so far (informational); 'views': views with a recorded ratio."""
    return {'enabled': _ASYNC['enabled'], 'headroom': _ASYNC['headroom'], 'ratio': _ASYNC['ratio'], 'overflows': _ASYNC['overflows'],
            'views': len(_ASYNC['per_view']), 'unchecked_passes': len(_ASYNC['pending'])}


def take_async_overflow(owned=None) -> bool:
    """True once after a backward pass had to return zero gradients because its forward pass overflowed its capacity: the optimizer step that
    would consume them must be skipped (FusedAdam.step does). The mark names the parameter tensors of that pass (their storage addresses): with
    `owned` (an iterable of tensors) only an optimizer that owns one of them takes it -- a second FusedAdam over other parameters neither
    consumes the mark nor skips its own step; without arguments any pending mark is taken. The next forward pass over the same parameters
    drops a mark nobody took (no optimizer step followed: another optimizer, an exception), so it cannot skip a later, valid step."""
    if owned is None:
        marked, _ASYNC['step_invalid'] = _ASYNC['step_invalid'], False
        return bool(marked)
    mine = {a for t in owned for a in _addresses(t)}
    for table in _ASYNC_SCOPES.values():          # the optimizer may step outside the scope block its passes ran in
        if table['step_invalid'] and not mine.isdisjoint(table['step_invalid']):
            table['step_invalid'] = False
            return True
    return False


def _addresses(t: torch.Tensor) -> tuple:
    """What identifies `t` in an overflow mark: its own address and the address of its storage -- a `.contiguous()` copy is neither, but a view, a
    slice or a reshaped alias of a marked parameter (or a parameter that is a view into a marked arena) still is."""
    if t.numel() == 0:
        return ()
    return (t.data_ptr(), t.untyped_storage().data_ptr())


def _tensor_version(t: torch.Tensor) -> int:
    """The autograd version counter, or None for tensors created under torch.inference_mode() (they have none, reading it raises): such a view
    is never cached -- every pass over it is a synchronous one."""
    try:
        return t._version
    except RuntimeError:
        return None


def _view_key(settings: RasterizerSettings):
    return (settings.w2c.data_ptr(), int(settings.width), int(settings.height), float(settings.focal_x), float(settings.focal_y),
            float(settings.center_x), float(settings.center_y))


def _view_ratio(A: dict, key, w2c: torch.Tensor) -> float:
    """The recorded instances-per-Gaussian ratio of this view, or 0.0 if `w2c` is not the very tensor (object and content version) it was recorded for."""
    entry = A['per_view'].get(key)
    if entry is None:
        return 0.0
    ratio, ref, version = entry
    if ref() is not w2c or version is None or _tensor_version(w2c) != version:
        del A['per_view'][key]
        return 0.0
    A['per_view'][key] = A['per_view'].pop(key)          # most recently used last
    return ratio


def _record_ratio(A: dict, key, w2c: torch.Tensor, ratio: float) -> None:
    table = A['per_view']
    table.pop(key, None)
    table[key] = (ratio, weakref.ref(w2c), _tensor_version(w2c))
    while len(table) > _ASYNC_MAX_VIEWS:
        del table[next(iter(table))]
    A['ratio'] = max(A['ratio'], ratio)


def _check_abandoned_passes(A: dict) -> None:
    """Asynchronous passes whose backward never ran: look at their counts now (their copies completed long ago) and say so if an image was truncated."""
    pending = A['pending']
    for ticket in list(pending):
        host, event, capacity = pending[ticket]
        if event is not None and not event.query():
            continue
        del pending[ticket]
        if int(host[2]) != 0:
            A['overflows'] += 1
            warnings.warn(f'FasterGS async forward: an earlier pass whose backward never ran needed {int(host[1])} instances but had capacity {capacity}: '
                          f'the image it returned was incomplete (render evaluation views under torch.no_grad(): those passes are sized synchronously)',
                          RuntimeWarning)
    while len(pending) > 64:                      # never unbounded: drop the oldest tickets unchecked
        del pending[next(iter(pending))]


def _require_gpu(t: torch.Tensor) -> None:
    if not t.is_cuda:
        # Renderer.py:58-59 raises in CPU mode as well; there is no CPU implementation behind this package
        raise RuntimeError('FasterGS rasterizer: tensors must live on a ROCm/HIP device (no CPU implementation)')


class _Rasterize(torch.autograd.Function):
    """Differentiable w.r.t. the six parameter tensors (rasterization.py:41-110 of the reference)."""

    @staticmethod
    def forward(ctx: Any, means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info,
                rasterizer_settings: RasterizerSettings) -> torch.Tensor:
        _require_gpu(means)
        be, n, A = default_backend(), means.shape[0], _ASYNC          # the active scope's table; backward uses the same one
        capacity, key = None, None
        if A['step_invalid']:
            # the step of that overflowed pass never came (no optimizer took the mark: another optimizer class, an exception, inputs that were
            # copies of the optimizer's tensors): a stale mark must not skip a later, valid step -- whatever tensors this pass is over
            A['step_invalid'] = False
        if A['enabled'] and n > 0:
            if A['pending']:
                _check_abandoned_passes(A)
            key = _view_key(rasterizer_settings)
            ratio = _view_ratio(A, key, rasterizer_settings.w2c)
            # only a pass whose backward will run ever looks at the asynchronous counts; everything else is checked now (synchronously)
            if ratio > 0.0 and any(ctx.needs_input_grad[:6]):
                capacity = int(ratio * n * A['headroom']) + 4096
        res = be.forward(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, rasterizer_settings, capacity)
        if capacity is None:
            if key is not None:
                _record_ratio(A, key, rasterizer_settings.w2c, res.state[1] / n)
            ctx.async_check = None
        else:
            host, event = be.forward_counts(res, n)
            A['ticket'] += 1
            A['pending'][A['ticket']] = (host, event, capacity)      # consumed by backward; looked at by a later forward otherwise
            ctx.async_check = (host, event, key, A['ticket'])
        ctx.rasterizer_settings = rasterizer_settings
        ctx.buffer_state = res.state
        ctx.sh0_addresses = _addresses(sh_coefficients_0)
        ctx.async_table = A
        ctx.save_for_backward(res.image, means, scales, rotations, opacities, sh_coefficients_rest, *res.buffers)
        ctx.densification_info = densification_info
        ctx.mark_non_differentiable(densification_info)
        return res.image

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, grad_image: torch.Tensor):
        image, means, scales, rotations, opacities, sh_rest, *buffers = ctx.saved_tensors
        state, A = ctx.buffer_state, ctx.async_table
        if ctx.async_check is not None:
            host, event, key, ticket = ctx.async_check
            A['pending'].pop(ticket, None)
            if event is not None:
                event.synchronize()
            n = means.shape[0]
            _record_ratio(A, key, ctx.rasterizer_settings.w2c, int(host[1]) / max(n, 1))
            if int(host[2]) != 0:          # the capacity was too small: the image (and the loss gradient) missed the instances beyond it
                A['overflows'] += 1
                warnings.warn(f'FasterGS async forward: {int(host[1])} instances exceeded the capacity {state[1]} of this pass: its image was '
                              f'incomplete, so this backward pass returns zero gradients and FusedAdam.step skips the step (the view is rendered with the '
                              f'right capacity next time)', RuntimeWarning)
                clear_live_blocks([means])
                A['step_invalid'] = frozenset(a for t in (means, scales, rotations, opacities, sh_rest) for a in _addresses(t)) | frozenset(ctx.sh0_addresses)
                if _GRAD_OUT is not None:          # a consumer that reads the provider's arena directly must not see the previous step's gradients
                    zeros = tuple(_GRAD_OUT())
                    for z in zeros:
                        z.zero_()
                else:
                    zeros = tuple(torch.zeros(sh, dtype=torch.float32, device=means.device) for sh in gradient_shapes(n, total_sh_rest(sh_rest)))
                return (*zeros, None, None)
        n = means.shape[0]
        handover = _LIVE['enabled'] and _GRAD_OUT is None and n > 0
        prior = None
        if handover:
            shapes = gradient_shapes(n, total_sh_rest(sh_rest))
            spare = _take_spare(shapes, means.device)
            if spare is not None:          # the previous pass's arena and what it says about its zeros; the flags of this pass go to a second array
                prior = spare['flags']
            _RECYCLE['recycled' if spare is not None else 'fresh'] += 1
            arena, out = _gradient_arena(shapes, means.device, None if spare is None else spare['arena'])
            del spare
            live, flags = torch.empty((2, (n + 63) // 64), dtype=torch.uint8, device=means.device)      # "any visible" / "any reached": the optimizer gets the latter
        else:
            clear_live_blocks([means])
            out, live, flags = (_GRAD_OUT() if _GRAD_OUT is not None else None), None, None
        grads = default_backend().backward(ctx.densification_info, grad_image, image, means, scales, rotations, opacities, sh_rest,
                                           buffers, ctx.rasterizer_settings, state, out=out, live_blocks=live, reached_blocks=flags, prior_blocks=prior)
        if handover:
            slots = _LIVE['slots']
            slots.pop(means.data_ptr(), None)
            slots[means.data_ptr()] = {'arena': arena, 'version': arena._version, 'flags': flags,
                                       'views': tuple((v.data_ptr() if v.numel() else 0, tuple(v.shape)) for v in out)}
            while len(slots) > _LIVE_MAX_SLOTS:          # models that backpropagate but never step: their arenas are not kept alive for ever
                del slots[next(iter(slots))]
        del out          # the registry and this frame hold no view tensor: autograd adopts a gradient as `.grad` only if nobody else references it
        return (*grads, None, None)   # densification_info, rasterizer_settings


def diff_rasterize(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
                   sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor, densification_info: torch.Tensor,
                   rasterizer_settings: RasterizerSettings) -> torch.Tensor:
    """Training render: image [3,H,W]; densification_info [2,N] is updated in backward, or pass torch.empty(0)."""
    return _Rasterize.apply(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info,
                            rasterizer_settings)


class _RasterizeAux(torch.autograd.Function):
    """_Rasterize that also returns accumulated opacity and expected depth, differentiable like the image (fgs_forward_aux / fgs_backward_aux).
    Always the synchronous forward pass; gradients in fresh tensors (no arena, no live-block hand-over: an optimizer reads them all)."""

    @staticmethod
    def forward(ctx: Any, means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info,
                rasterizer_settings: RasterizerSettings, alpha: bool, depth: bool):
        _require_gpu(means)
        res = default_backend().forward_aux(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, rasterizer_settings, alpha, depth)
        ctx.rasterizer_settings = rasterizer_settings
        ctx.buffer_state = res.state
        ctx.has_depth = res.depth is not None
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None (= zero), not as a tensor of zeros
        shape = (rasterizer_settings.height, rasterizer_settings.width)
        a = res.alpha if res.alpha is not None else means.new_empty(shape)            # autograd wants tensors: the placeholders are non-differentiable
        d = res.depth if res.depth is not None else means.new_empty(shape)
        ctx.save_for_backward(res.image, d, means, scales, rotations, opacities, sh_coefficients_rest, *res.buffers)
        ctx.densification_info = densification_info
        ctx.mark_non_differentiable(densification_info, *([a] if res.alpha is None else []), *([d] if res.depth is None else []))
        return res.image, a, d

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, grad_image, grad_alpha, grad_depth):
        image, depth, means, scales, rotations, opacities, sh_rest, *buffers = ctx.saved_tensors
        if grad_image is None:
            grad_image = torch.zeros_like(image)
        if not ctx.has_depth:
            grad_depth = None
        clear_live_blocks([means])
        grads = default_backend().backward_aux(ctx.densification_info, grad_image.contiguous(),
                                               grad_alpha.contiguous() if grad_alpha is not None else None,
                                               grad_depth.contiguous() if grad_depth is not None else None,
                                               image, depth, means, scales, rotations, opacities, sh_rest, buffers, ctx.rasterizer_settings, ctx.buffer_state)
        return (*grads, None, None, None, None)


def diff_rasterize_aux(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
                       sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor, densification_info: torch.Tensor,
                       rasterizer_settings: RasterizerSettings, alpha: bool = True, depth: bool = True):
    """Training render that also returns, differentiable, the accumulated opacity A = 1 - T_final and the expected depth D = sum_i w_i z_i
    (w_i = T_i alpha_i, z_i = view-space depth of Gaussian i's mean; not normalised: D / A.clamp_min(1e-8) is a mean depth and autograd handles the
    division). Returns (image [3,H,W], alpha [H,W] or None, depth [H,W] or None). The median depth stays inference-only (rasterize_aux)."""
    if not (alpha or depth):
        raise ValueError('diff_rasterize_aux: neither alpha nor depth requested; use diff_rasterize')
    image, a, d = _RasterizeAux.apply(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info,
                                      rasterizer_settings, bool(alpha), bool(depth))
    return image, (a if alpha else None), (d if depth else None)


class _RasterizeAbsgrad(torch.autograd.Function):
    """_RasterizeAux whose backward pass also accumulates the absolute-gradient densification statistic into `abs_densification_info`
    (fgs_backward_absgrad). The maps are optional: without them the forward pass is the plain one. Always synchronous, gradients in fresh tensors."""

    @staticmethod
    def forward(ctx: Any, means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info, abs_densification_info,
                rasterizer_settings: RasterizerSettings, alpha: bool, depth: bool):
        _require_gpu(means)
        params = (means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest)
        be = default_backend()
        if alpha or depth:
            res = be.forward_aux(*params, rasterizer_settings, alpha, depth)
            res_alpha, res_depth = res.alpha, res.depth
        else:
            res = be.forward(*params, rasterizer_settings)
            res_alpha = res_depth = None
        ctx.rasterizer_settings = rasterizer_settings
        ctx.buffer_state = res.state
        ctx.has_depth = res_depth is not None
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None (= zero), not as a tensor of zeros
        shape = (rasterizer_settings.height, rasterizer_settings.width)
        a = res_alpha if res_alpha is not None else means.new_empty(shape)            # autograd wants tensors: the placeholders are non-differentiable
        d = res_depth if res_depth is not None else means.new_empty(shape)
        ctx.save_for_backward(res.image, d, means, scales, rotations, opacities, sh_coefficients_rest, *res.buffers)
        ctx.densification_info = densification_info
        ctx.abs_densification_info = abs_densification_info
        ctx.mark_non_differentiable(densification_info, abs_densification_info, *([a] if res_alpha is None else []), *([d] if res_depth is None else []))
        return res.image, a, d

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, grad_image, grad_alpha, grad_depth):
        image, depth, means, scales, rotations, opacities, sh_rest, *buffers = ctx.saved_tensors
        if grad_image is None:
            grad_image = torch.zeros_like(image)
        if not ctx.has_depth:
            grad_depth = None
        clear_live_blocks([means])
        grads = default_backend().backward_absgrad(ctx.densification_info, ctx.abs_densification_info, grad_image.contiguous(),
                                                   grad_alpha.contiguous() if grad_alpha is not None else None,
                                                   grad_depth.contiguous() if grad_depth is not None else None,
                                                   image, depth, means, scales, rotations, opacities, sh_rest, buffers, ctx.rasterizer_settings, ctx.buffer_state)
        return (*grads, None, None, None, None, None)


def diff_rasterize_absgrad(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
                           sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor, densification_info: torch.Tensor,
                           rasterizer_settings: RasterizerSettings, abs_densification_info: torch.Tensor, alpha: bool = False, depth: bool = False):
    """Training render whose backward pass also accumulates the absolute-gradient densification statistic (AbsGS; gsplat's absgrad=True):
    (image [3,H,W], alpha [H,W] or None, depth [H,W] or None), the maps as in diff_rasterize_aux. `abs_densification_info`: float32 [2,N] like
    `densification_info`, updated in backward -- row 0 += 1 per visible Gaussian, row 1 += sqrt((0.5 W sum_p |gx_p|)^2 + (0.5 H sum_p |gy_p|)^2) with
    (gx_p, gy_p) pixel p's share of dL/dmean2d: where densification_info[1] takes the norm of the signed sums, which cancel over a large footprint, this
    sums magnitudes. A drop-in statistic for adaptive density control (with a threshold of its own). torch.empty(0) for it gives diff_rasterize_aux
    (or, without maps, diff_rasterize's gradients). `densification_info` may be updated as well, or be torch.empty(0)."""
    image, a, d = _RasterizeAbsgrad.apply(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info,
                                          abs_densification_info, rasterizer_settings, bool(alpha), bool(depth))
    return image, (a if alpha else None), (d if depth else None)


class _RasterizePose(torch.autograd.Function):
    """_RasterizeAux whose camera is an input: w2c ([3,4] or [4,4]) and cam_position ([3]) replace the tensors of the settings and receive gradients
    (fgs_backward_pose). The maps are optional: without them the forward pass is the plain one. Always synchronous, gradients in fresh tensors."""

    @staticmethod
    def forward(ctx: Any, means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info, w2c, cam_position,
                rasterizer_settings: RasterizerSettings, alpha: bool, depth: bool):
        _require_gpu(means)
        settings = rasterizer_settings._replace(w2c=w2c.detach(), cam_position=cam_position.detach())
        params = (means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest)
        be = default_backend()
        if alpha or depth:
            res = be.forward_aux(*params, settings, alpha, depth)
            res_alpha, res_depth = res.alpha, res.depth
        else:
            res = be.forward(*params, settings)
            res_alpha = res_depth = None
        ctx.rasterizer_settings = settings
        ctx.buffer_state = res.state
        ctx.has_depth = res_depth is not None
        ctx.camera = (tuple(w2c.shape), w2c.dtype, cam_position.dtype)
        ctx.set_materialize_grads(False)
        shape = (settings.height, settings.width)
        a = res_alpha if res_alpha is not None else means.new_empty(shape)
        d = res_depth if res_depth is not None else means.new_empty(shape)
        ctx.save_for_backward(res.image, d, means, scales, rotations, opacities, sh_coefficients_rest, *res.buffers)
        ctx.densification_info = densification_info
        ctx.mark_non_differentiable(densification_info, *([a] if res_alpha is None else []), *([d] if res_depth is None else []))
        return res.image, a, d

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, grad_image, grad_alpha, grad_depth):
        image, depth, means, scales, rotations, opacities, sh_rest, *buffers = ctx.saved_tensors
        if grad_image is None:
            grad_image = torch.zeros_like(image)
        if not ctx.has_depth:
            grad_depth = None
        clear_live_blocks([means])
        # a camera input that does not require grad costs nothing: neither asked for is backward_aux exactly, the POSE kernel is not launched
        *grads, grad_w2c, grad_cam = default_backend().backward_pose(
            ctx.densification_info, grad_image.contiguous(), grad_alpha.contiguous() if grad_alpha is not None else None,
            grad_depth.contiguous() if grad_depth is not None else None, image, depth, means, scales, rotations, opacities, sh_rest, buffers,
            ctx.rasterizer_settings, ctx.buffer_state, w2c=ctx.needs_input_grad[7], cam_position=ctx.needs_input_grad[8])
        w2c_shape, w2c_dtype, cam_dtype = ctx.camera
        if grad_w2c is not None:
            if w2c_shape[0] == 4:                 # the last row of a [4,4] w2c is not read
                grad_w2c = torch.cat([grad_w2c, grad_w2c.new_zeros((1, 4))])
            grad_w2c = grad_w2c.to(w2c_dtype)
        if grad_cam is not None:
            grad_cam = grad_cam.to(cam_dtype)
        return (*grads, None, grad_w2c, grad_cam, None, None, None)


def diff_rasterize_pose(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
                        sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor, densification_info: torch.Tensor,
                        rasterizer_settings: RasterizerSettings, w2c: 'torch.Tensor | None' = None, cam_position: 'torch.Tensor | None' = None,
                        alpha: bool = False, depth: bool = False):
    """Training render that is also differentiable in the camera pose: (image [3,H,W], alpha [H,W] or None, depth [H,W] or None), the maps as in
    diff_rasterize_aux. `w2c` ([4,4] or [3,4]) and `cam_position` ([3]) override the tensors of the settings (None: the settings' own) and may
    require grad; they are independent inputs, as in the settings. With cam_position=None and a w2c that requires grad the position is derived
    here as -w2c[:3,:3].T @ w2c[:3,3], so autograd composes both gradients into w2c's. The gradient of a [4,4] w2c has a zero last row. A camera
    input that does not require grad costs nothing. No gradient for the intrinsics."""
    w2c_given = w2c is not None
    if not w2c_given:
        w2c = rasterizer_settings.w2c
    if w2c.dim() != 2 or tuple(w2c.shape) not in ((3, 4), (4, 4)):
        raise ValueError(f'diff_rasterize_pose: w2c must be [4,4] or [3,4], not {tuple(w2c.shape)}')
    if cam_position is None:
        cam_position = -w2c[:3, :3].T @ w2c[:3, 3] if w2c_given else rasterizer_settings.cam_position
    if cam_position.numel() != 3:
        raise ValueError(f'diff_rasterize_pose: cam_position must have 3 entries, not {tuple(cam_position.shape)}')
    image, a, d = _RasterizePose.apply(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info,
                                       w2c, cam_position.reshape(3), rasterizer_settings, bool(alpha), bool(depth))
    return image, (a if alpha else None), (d if depth else None)


class _RasterizeFeatures(torch.autograd.Function):
    """_Rasterize that also blends F per-Gaussian feature channels with the compositing weights of the same pass, differentiable in the features and --
    unless detach_geometry -- through the weights in the Gaussians (fgs_blend_features / fgs_backward_features). Always the synchronous forward pass;
    gradients in fresh tensors (no arena, no live-block hand-over)."""

    @staticmethod
    def forward(ctx: Any, means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info, features,
                rasterizer_settings: RasterizerSettings, detach_geometry: bool):
        _require_gpu(means)
        be = default_backend()
        res = be.forward(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, rasterizer_settings)
        feature_map = be.blend_features(features, res, means.shape[0], rasterizer_settings)
        ctx.rasterizer_settings = rasterizer_settings
        ctx.buffer_state = res.state
        ctx.detach_geometry = bool(detach_geometry)
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None (= zero), not as a tensor of zeros
        ctx.save_for_backward(res.image, feature_map, features, means, scales, rotations, opacities, sh_coefficients_rest, *res.buffers)
        ctx.densification_info = densification_info
        ctx.mark_non_differentiable(densification_info)
        return res.image, feature_map

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, grad_image, grad_feature_map):
        image, feature_map, features, means, scales, rotations, opacities, sh_rest, *buffers = ctx.saved_tensors
        if grad_image is None:
            grad_image = torch.zeros_like(image)
        clear_live_blocks([means])
        # a feature map that is not part of the loss costs nothing: the pass is then the plain one and the features get no gradient
        *grads, grad_features = default_backend().backward_features(
            ctx.densification_info, grad_image.contiguous(), grad_feature_map.contiguous() if grad_feature_map is not None else None, image, feature_map,
            features, means, scales, rotations, opacities, sh_rest, buffers, ctx.rasterizer_settings, ctx.buffer_state, ctx.detach_geometry)
        return (*grads, None, grad_features if ctx.needs_input_grad[7] else None, None, None)


def diff_rasterize_features(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
                            sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor, densification_info: torch.Tensor,
                            rasterizer_settings: RasterizerSettings, features: torch.Tensor, detach_geometry: bool = False):
    """Training render that also returns, differentiable, the blend of per-Gaussian feature channels: (image [3,H,W], feature_map [F,H,W]) with
    feature_map[c] = sum_i w_i features[i, c] over the pairs the image blended (w_i = T_i alpha_i; no background term, not normalised: divide by the
    accumulated opacity -- a channel of ones -- for a mean). `features`: float32 [N, F], any sign, 1 <= F <= 64: semantic or language features, normals,
    ids, an appearance code. One forward and one backward pass whatever F. detach_geometry=True: the feature loss trains the features only (the
    Gaussians get the image's gradients). The image is diff_rasterize's."""
    if features.dtype != torch.float32 or not features.is_contiguous():          # shape and channel count are the backend's to refuse
        features = features.to(torch.float32).contiguous()
    return _RasterizeFeatures.apply(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info, features,
                                    rasterizer_settings, bool(detach_geometry))


class _RasterizeDistortion(torch.autograd.Function):
    """_Rasterize that also returns the depth-distortion map of the same pass, differentiable through the compositing weights and the depths of the
    Gaussians (fgs_blend_distortion / fgs_backward_distortion). Always the synchronous forward pass; gradients in fresh tensors (no arena, no
    live-block hand-over)."""

    @staticmethod
    def forward(ctx: Any, means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info,
                rasterizer_settings: RasterizerSettings, normalized: bool):
        _require_gpu(means)
        be = default_backend()
        res = be.forward(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, rasterizer_settings)
        state = be.blend_distortion(means, res, means.shape[0], rasterizer_settings, normalized)
        ctx.rasterizer_settings = rasterizer_settings
        ctx.buffer_state = res.state
        ctx.normalized = bool(normalized)
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None (= zero), not as a tensor of zeros
        ctx.save_for_backward(res.image, state, means, scales, rotations, opacities, sh_coefficients_rest, *res.buffers)
        ctx.densification_info = densification_info
        ctx.mark_non_differentiable(densification_info)
        return res.image, state[0]

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, grad_image, grad_distortion):
        image, state, means, scales, rotations, opacities, sh_rest, *buffers = ctx.saved_tensors
        if grad_image is None:
            grad_image = torch.zeros_like(image)
        clear_live_blocks([means])
        # a distortion map that is not part of the loss costs nothing: the pass is then the plain one
        grads = default_backend().backward_distortion(
            ctx.densification_info, grad_image.contiguous(), grad_distortion.contiguous() if grad_distortion is not None else None, image, state,
            means, scales, rotations, opacities, sh_rest, buffers, ctx.rasterizer_settings, ctx.buffer_state, ctx.normalized)
        return (*grads, None, None, None)


def diff_rasterize_distortion(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
                              sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor, densification_info: torch.Tensor,
                              rasterizer_settings: RasterizerSettings, normalized: bool = True):
    """Training render that also returns, differentiable, the depth-distortion map of Mip-NeRF 360 / 2DGS: (image [3,H,W], distortion [H,W]) with
    distortion[p] = sum_a sum_b w_a w_b |t_a - t_b| over the pairs the image blended in pixel p (w_i = T_i alpha_i). t is the view-space depth z of the
    Gaussian's mean, mapped onto [0, 1) as far (z - near) / ((far - near) z) with the settings' planes unless normalized=False. A regulariser
    `weight * distortion.mean()` pulls the weight of each ray onto one surface. One extra walk forward and one backward; a map the loss does not use
    costs nothing in the backward pass. The image is diff_rasterize's. No gradient for the planes."""
    return _RasterizeDistortion.apply(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info,
                                      rasterizer_settings, bool(normalized))


class _RasterizeGeometry(torch.autograd.Function):
    """_Rasterize that also returns, from ONE extra walk, the depth-distortion map and the blend of five per-Gaussian surface channels of the same pass,
    differentiable in the Gaussians and in the channels (fgs_blend_geometry / fgs_backward_geometry). Always the synchronous forward pass; gradients in
    fresh tensors (no arena, no live-block hand-over)."""

    @staticmethod
    def forward(ctx: Any, means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info, surface_features,
                rasterizer_settings: RasterizerSettings, normalized: bool):
        _require_gpu(means)
        be = default_backend()
        res = be.forward(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, rasterizer_settings)
        state = be.blend_geometry(means, surface_features, res, means.shape[0], rasterizer_settings, normalized)
        ctx.rasterizer_settings = rasterizer_settings
        ctx.buffer_state = res.state
        ctx.normalized = bool(normalized)
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None (= zero), not as a tensor of zeros
        ctx.save_for_backward(res.image, state, surface_features, means, scales, rotations, opacities, sh_coefficients_rest, *res.buffers)
        ctx.densification_info = densification_info
        ctx.mark_non_differentiable(densification_info)
        return res.image, state[0], state[2:7]

    @staticmethod
    @once_differentiable
    def backward(ctx: Any, grad_image, grad_distortion, grad_surface_map):
        image, state, surface_features, means, scales, rotations, opacities, sh_rest, *buffers = ctx.saved_tensors
        if grad_image is None:
            grad_image = torch.zeros_like(image)
        clear_live_blocks([means])
        # a map that is not part of the loss costs nothing: its sums are not formed, and with neither the pass is the plain one
        *grads, grad_features = default_backend().backward_geometry(
            ctx.densification_info, grad_image.contiguous(), grad_distortion.contiguous() if grad_distortion is not None else None,
            grad_surface_map.contiguous() if grad_surface_map is not None else None, image, state, surface_features,
            means, scales, rotations, opacities, sh_rest, buffers, ctx.rasterizer_settings, ctx.buffer_state, ctx.normalized)
        return (*grads, None, grad_features if ctx.needs_input_grad[7] else None, None, None)


def diff_rasterize_geometry(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
                            sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor, densification_info: torch.Tensor,
                            rasterizer_settings: RasterizerSettings, surface_features: torch.Tensor, normalized: bool = True):
    """Training render that also returns, differentiable and from one extra walk forward and one backward, what the geometry terms of 2DGS-style
    training need: (image [3,H,W], distortion [H,W], surface_map [5,H,W]). distortion is diff_rasterize_distortion's map (same `normalized`);
    surface_map[c] = sum_i w_i surface_features[i, c] is diff_rasterize_features' map of `surface_features`, float32 [N, 5] -- for
    `gaussian_surface_features` the blended normal (0..2), the expected depth (3) and the accumulated opacity (4), which `normal_consistency` takes as
    it is and a depth loss reads as surface_map[3], surface_map[4]. An output the loss does not use costs nothing in the backward pass; with neither
    map in the loss that pass is diff_rasterize's. The image is diff_rasterize's. No gradient for the planes."""
    if surface_features.dtype != torch.float32 or not surface_features.is_contiguous():          # the shape is the backend's to refuse
        surface_features = surface_features.to(torch.float32).contiguous()
    return _RasterizeGeometry.apply(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, densification_info, surface_features,
                                    rasterizer_settings, bool(normalized))


def rasterize(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
              sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor, rasterizer_settings: RasterizerSettings,
              to_chw: bool, clamp_output: bool = True) -> torch.Tensor:
    """Forward-only render (the reference's benchmark path, Renderer.py:107-123): [3,H,W] or [H,W,3]."""
    _require_gpu(means)
    return default_backend().inference(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest,
                                       rasterizer_settings, to_chw, clamp_output)


def rasterize_aux(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
                  sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor, rasterizer_settings: RasterizerSettings,
                  to_chw: bool, clamp_output: bool = True, alpha: bool = True, depth: 'str | None' = 'expected',
                  normalize_depth: bool = False) -> dict:
    """Forward-only render that also returns per-pixel maps of the same blend, float32 [H,W], without gradients:
      'rgb'          : what `rasterize` returns, bit for bit;
      'alpha'        : accumulated opacity 1 - T_final (the background is not part of it)            -- alpha=True;
      'depth'        : sum_i w_i z_i, w_i = T_i alpha_i, z_i = view-space depth of Gaussian i's mean -- depth='expected' or 'both';
                       normalize_depth=True divides it by alpha.clamp_min(1e-8) (a mean depth; 0 where nothing was blended);
      'depth_median' : z of the Gaussian that takes T across 0.5, or of the last one blended if the pixel stays more than half
                       transparent; 0 where nothing was blended                                     -- depth='median' or 'both'."""
    if depth not in ('expected', 'median', 'both', None):
        raise ValueError(f"depth must be 'expected', 'median', 'both' or None, not {depth!r}")
    want_expected, want_median = depth in ('expected', 'both'), depth in ('median', 'both')
    normalize = normalize_depth and want_expected
    if not (alpha or want_expected or want_median):
        raise ValueError('rasterize_aux: no auxiliary map requested (alpha=False, depth=None); use rasterize')
    _require_gpu(means)
    out = default_backend().inference_aux(means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest, rasterizer_settings,
                                          to_chw, clamp_output, alpha or normalize, want_expected, want_median)
    if normalize:
        out['depth'] = out['depth'] / out['alpha'].clamp_min(1e-8)
        if not alpha:
            del out['alpha']
    return out


def update_pruning_scores(scores: torch.Tensor, means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor,
                          opacities: torch.Tensor, sh_coefficients_0: torch.Tensor, sh_coefficients_rest: torch.Tensor,
                          rasterizer_settings: RasterizerSettings) -> None:
    """Speedy-Splat importance scores of one view, accumulated into `scores` (reference rasterization.py:159-178,
    called per training view from Renderer.py:141-156)."""
    _require_gpu(means)
    default_backend().pruning_scores(scores, means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest,
                                     rasterizer_settings)
