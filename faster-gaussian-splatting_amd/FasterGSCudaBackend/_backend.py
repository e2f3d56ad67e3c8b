"""torch <-> C-ABI glue: turns tensors into raw pointers, owns the resize callback, checks status codes.

One `Backend` wraps one loaded library handle. The product uses `default_backend()` (libfgs_hip.so); the test-suite also
builds one around the CPU simulation library to exercise this exact code path without a GPU.
Mirrors what the reference does in C++ in rasterization_api.cu:13-247 and utils/torch_utils.h:6-12.

A check that several entries make is one function below; where the entries differ in what they check it takes a flag (tests/glue_cases.py).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib


class RasterizerSettings(NamedTuple):
    """Same 13 fields, order and meaning as the reference (torch_bindings/rasterization.py:8-38)."""
    w2c: torch.Tensor            # affine transformation from model/world space to view space (row-major, >= 3 rows)
    cam_position: torch.Tensor   # camera position in world space
    bg_color: torch.Tensor       # background colour (RGB)
    active_sh_bases: int         # number of SH bases used for colour
    width: int                   # image width in pixels
    height: int                  # image height in pixels
    focal_x: float               # focal length in pixels
    focal_y: float
    center_x: float              # principal point in pixels, +x right
    center_y: float              # +y down
    near_plane: float
    far_plane: float
    proper_antialiasing: bool

    def as_tuple(self) -> tuple:
        return tuple(self)


class ForwardResult(NamedTuple):
    image: torch.Tensor
    buffers: tuple          # (primitive, tile, instance, bucket) uint8 tensors, opaque
    state: tuple            # (n_visible, n_instances, n_buckets, selector), opaque


class ForwardAuxResult(NamedTuple):
    image: torch.Tensor
    alpha: Optional[torch.Tensor]   # [H,W] accumulated opacity 1 - T_final, or None if not requested
    depth: Optional[torch.Tensor]   # [H,W] expected depth sum_i w_i z_i (not normalised), or None
    buffers: tuple
    state: tuple


PARAMETER_NAMES = ('means', 'scales', 'rotations', 'opacities', 'sh_coefficients_0', 'sh_coefficients_rest')
BACKWARD_PARAMETER_NAMES = PARAMETER_NAMES[:4] + PARAMETER_NAMES[5:]      # the backward passes do not read sh_coefficients_0


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _stream_of(device: torch.device) -> int:
    """The caller's current stream on the tensors' device. The library launches on the CURRENT device (it never switches
    devices), so a mismatch is reported here instead of surfacing as an opaque HIP error later."""
    if device.type != 'cuda':
        return 0
    if device.index is not None and device.index != torch.cuda.current_device():
        raise RuntimeError(f'tensors live on {device} but the current device is cuda:{torch.cuda.current_device()}; '
                           f'call under torch.cuda.device({device.index})')
    return torch.cuda.current_stream(device).cuda_stream


def total_sh_rest(sh_rest: torch.Tensor) -> int:
    """Rest coefficients per channel of a [N, total_rest, 3] tensor; 0 for an (empty) tensor of any other rank."""
    return sh_rest.shape[1] if sh_rest.dim() == 3 else 0


def gradient_shapes(n: int, total_rest: int) -> tuple:
    """Shapes of the six gradients in the order every backward pass writes them: means, scales, rotations, opacities, sh0, sh_rest."""
    return ((n, 3), (n, 3), (n, 4), (n, 1), (n, 1, 3), (n, total_rest, 3))


def _state_tuple(st: _lib.ForwardState) -> tuple:
    return (st.n_visible, st.n_instances, st.n_buckets, st.selector)


def _pointer_array(tensors: Sequence[torch.Tensor], k: int):
    return (C.c_void_p * k)(*[_ptr(t) for t in tensors])


def _shard_counts(shard_counts: Sequence[int] | None) -> tuple:
    """(int32 array or None, its length) of the optional records-per-shard list of the two record entries."""
    k = len(shard_counts) if shard_counts else 0
    return ((C.c_int32 * k)(*[int(c) for c in shard_counts]) if k else None), k


def _empty_bytes(nbytes: int, device: torch.device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _check_block_flags(name: str, flags: Optional[torch.Tensor], n: int, device: torch.device, owner: str = 'parameters') -> None:
    if flags is not None and (flags.dtype != torch.uint8 or flags.device != device or not flags.is_contiguous() or flags.numel() != (n + 63) // 64):
        raise RuntimeError(f'{name} must be a contiguous uint8 tensor of ceil(N / 64) elements on the {owner}\' device')


def _gradients_out(out, shapes: tuple, device: torch.device, shapes_only: bool = False) -> tuple:
    """The six gradient tensors of a backward pass: fresh ones, or the caller's `out` after a check. shapes_only: the sharded owner pass, whose
    parameter check has looked at dtype, strides and device of `out` already."""
    if out is None:
        return tuple(torch.empty(sh, dtype=torch.float32, device=device) for sh in shapes)
    for g, sh in zip(out, shapes):
        if tuple(g.shape) != sh or not (shapes_only or (g.dtype == torch.float32 and g.is_contiguous() and g.device == device)):
            raise RuntimeError(f'preallocated gradient has shape {tuple(g.shape)}, expected {"" if shapes_only else "contiguous float32 "}{sh}')
    return tuple(out)


def _densification(densification_info, n: int, device: torch.device, validate: bool):
    """None and an empty tensor both mean "no statistics" (api:136). validate: the plain backward passes; the fused and sharded ones take it as it comes."""
    dens = densification_info if densification_info is not None and densification_info.numel() > 0 else None
    if validate and dens is not None and (dens.dtype != torch.float32 or not dens.is_contiguous() or dens.device != device or dens.numel() != 2 * n):
        raise RuntimeError('densification_info must be a contiguous float32 [2, N] tensor on the parameters\' device')
    return dens


def _check_acc_records(acc_records: torch.Tensor, n_visible: Sequence[int], k: int, device: torch.device) -> int:
    """sum(n_visible), once the accumulator records of the `k` views have been checked against it."""
    total = int(sum(n_visible))
    if len(n_visible) != k or (total > 0 and (acc_records.dtype != torch.float32 or acc_records.numel() < 9 * total
                                              or not acc_records.is_contiguous() or acc_records.device != device)):
        raise RuntimeError('acc_records must be contiguous float32 [sum(n_visible), 9] and n_visible one entry per view')
    return total


class Backend:
    def __init__(self, lib: C.CDLL):
        self.lib = lib
        self._pending_counts: list = []          # (pinned host tensor, event) of the count read-backs still in flight (forward_counts)
        self._relocation_table: dict = {}        # device -> the 2500-entry table of relocation_adjustment

    # -- helpers ---------------------------------------------------------------------------------------------------
    def _check(self, status: int, what: str) -> None:
        if status != 0:
            raise RuntimeError(f'{what} failed (status {status}): {self.lib.fgs_last_error().decode()}')

    @staticmethod
    def _settings(s: RasterizerSettings, total_sh_rest: int, device: torch.device, keep: list) -> _lib.Settings:
        w2c = s.w2c.to(device=device, dtype=torch.float32).contiguous()
        cam = s.cam_position.to(device=device, dtype=torch.float32).contiguous()
        bg = s.bg_color.to(device=device, dtype=torch.float32).contiguous()
        if w2c.numel() < 12 or cam.numel() < 3 or bg.numel() < 3:
            raise ValueError('w2c needs >= 3x4, cam_position and bg_color 3 entries')
        keep += [w2c, cam, bg]
        return _lib.Settings(w2c.data_ptr(), cam.data_ptr(), bg.data_ptr(), int(s.active_sh_bases), int(total_sh_rest),
                             int(s.width), int(s.height), float(s.focal_x), float(s.focal_y), float(s.center_x),
                             float(s.center_y), float(s.near_plane), float(s.far_plane), int(bool(s.proper_antialiasing)))

    @staticmethod
    def _check_params(tensors: Sequence[torch.Tensor], names: Sequence[str]) -> torch.device:
        device = tensors[0].device
        for t, n in zip(tensors, names):   # utils/torch_utils.h:14-19 (CHECK_INPUT)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
                raise RuntimeError(f"Input tensor '{n}' must be a contiguous float32 tensor on {device}.")
        return device

    @staticmethod
    def _make_resizer(device: torch.device, n_buffers: int):
        buffers = [torch.empty(0, dtype=torch.uint8, device=device) for _ in range(n_buffers)]

        def resize(_user, which, nbytes):          # utils/torch_utils.h:6-12
            try:
                buffers[which].resize_(int(nbytes))
                return buffers[which].data_ptr() if nbytes else 0
            except Exception:                       # never let an exception cross the C boundary
                return 0
        return buffers, _lib.RESIZE_FN(resize)

    def _forward_state(self, settings: RasterizerSettings, total_rest: int, device: torch.device) -> tuple:
        """(Settings, the tensors it points into, the four resizable buffers, their callback, an empty ForwardState): the caller keeps all of it
        referenced until the library call has returned."""
        keep: list = []
        S = self._settings(settings, total_rest, device, keep)
        buffers, cb = self._make_resizer(device, 4)
        return S, keep, buffers, cb, _lib.ForwardState()

    def _forward_setup(self, params: Sequence[torch.Tensor], settings: RasterizerSettings) -> tuple:
        """Checks the six parameter tensors: (their device, *_forward_state)."""
        device = self._check_params(params, PARAMETER_NAMES)
        return (device, *self._forward_state(settings, total_sh_rest(params[5]), device))

    # -- entry points -----------------------------------------------------------------------------------------------
    def forward(self, means, scales, rotations, opacities, sh0, sh_rest, settings: RasterizerSettings,
                instance_capacity: int | None = None) -> ForwardResult:
        """instance_capacity: None = fgs_forward (one host read of the counts); an int = fgs_forward_async, no host wait -- state then
        holds bounds (N, capacity, ...) and `forward_counts` tells later whether the capacity was enough."""
        device, S, keep, buffers, cb, st = self._forward_setup((means, scales, rotations, opacities, sh0, sh_rest), settings)
        image = torch.empty((3, settings.height, settings.width), dtype=torch.float32, device=device)
        if instance_capacity is None:
            self._check(self.lib.fgs_forward(_ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh0), _ptr(sh_rest),
                                             means.shape[0], C.byref(S), image.data_ptr(), cb, None, C.byref(st), _stream_of(device)),
                        'fgs_forward')
        else:
            self._check(self.lib.fgs_forward_async(_ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh0), _ptr(sh_rest),
                                                   means.shape[0], C.byref(S), image.data_ptr(), int(instance_capacity), cb, None, C.byref(st),
                                                   _stream_of(device)), 'fgs_forward_async')
        return ForwardResult(image, tuple(buffers), _state_tuple(st))

    def forward_aux(self, means, scales, rotations, opacities, sh0, sh_rest, settings: RasterizerSettings, alpha: bool = True,
                    depth: bool = True, instance_capacity: int | None = None) -> ForwardAuxResult:
        """fgs_forward_aux: the training forward pass plus accumulated opacity and / or expected depth [H,W] of the same walk, and the depth
        checkpoints `backward_aux` needs. The buffers are valid input to the plain `backward` / `backward_adam_fused` too."""
        if instance_capacity is not None:
            raise RuntimeError('forward_aux: the asynchronous forward pass (instance_capacity) does not return maps; use forward() or drop the capacity')
        if not (alpha or depth):
            raise RuntimeError('forward_aux: neither alpha nor depth requested (use forward)')
        device, S, keep, buffers, cb, st = self._forward_setup((means, scales, rotations, opacities, sh0, sh_rest), settings)
        image = torch.empty((3, settings.height, settings.width), dtype=torch.float32, device=device)
        maps = [torch.empty((settings.height, settings.width), dtype=torch.float32, device=device) if wanted else None for wanted in (alpha, depth)]
        self._check(self.lib.fgs_forward_aux(_ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh0), _ptr(sh_rest),
                                             means.shape[0], C.byref(S), image.data_ptr(), *[m.data_ptr() if m is not None else None for m in maps],
                                             cb, None, C.byref(st), _stream_of(device)), 'fgs_forward_aux')
        return ForwardAuxResult(image, maps[0], maps[1], tuple(buffers), _state_tuple(st))

    def forward_counts(self, result: ForwardResult, n_primitives: int):
        """Enqueues the read-back of (n_visible, n_instances, capacity_exceeded) of a forward pass; returns (pinned int32[3] tensor, event).
        The values are valid after event.synchronize() -- typically free by the time backward runs."""
        host = torch.empty(3, dtype=torch.int32, pin_memory=result.image.is_cuda)
        self._check(self.lib.fgs_forward_counts(_ptr(result.buffers[0]), int(n_primitives), host.data_ptr(), _stream_of(result.image.device)),
                    'fgs_forward_counts')
        event = None
        if result.image.is_cuda:
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(result.image.device))
            # The copy is a raw hipMemcpyAsync that torch's caching host allocator knows nothing about: if the caller drops `host` before the
            # copy has run (forward under no_grad, an exception, a freed graph), the pinned block would go back to the cache and the late copy
            # would land in whoever got it next. Keep every buffer referenced here until its event has completed.
            self._pending_counts[:] = [(h, e) for h, e in self._pending_counts if not e.query()]
            self._pending_counts.append((host, event))
        return host, event

    def inference(self, means, scales, rotations, opacities, sh0, sh_rest, settings: RasterizerSettings, to_chw: bool,
                  clamp_output: bool, return_state: bool = False):
        device, S, keep, buffers, cb, st = self._forward_setup((means, scales, rotations, opacities, sh0, sh_rest), settings)
        shape = (3, settings.height, settings.width) if to_chw else (settings.height, settings.width, 3)
        image = torch.empty(shape, dtype=torch.float32, device=device)
        self._check(self.lib.fgs_inference(_ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh0), _ptr(sh_rest),
                                           means.shape[0], C.byref(S), image.data_ptr(), int(to_chw), int(clamp_output), cb, None,
                                           C.byref(st), _stream_of(device)), 'fgs_inference')
        if return_state:
            return ForwardResult(image, tuple(buffers), _state_tuple(st))
        return image

    def inference_aux(self, means, scales, rotations, opacities, sh0, sh_rest, settings: RasterizerSettings, to_chw: bool,
                      clamp_output: bool, alpha: bool = True, depth_expected: bool = True, depth_median: bool = True) -> dict:
        """fgs_inference_aux: the forward-only render plus the requested per-pixel maps of the same walk, float32 [H,W] (include/fgs_hip.h).
        Returns {'rgb', 'alpha'?, 'depth'?, 'depth_median'?}; 'rgb' is bit-identical to `inference`."""
        device, S, keep, buffers, cb, st = self._forward_setup((means, scales, rotations, opacities, sh0, sh_rest), settings)
        shape = (3, settings.height, settings.width) if to_chw else (settings.height, settings.width, 3)
        out = {'rgb': torch.empty(shape, dtype=torch.float32, device=device)}
        for name, wanted in (('alpha', alpha), ('depth', depth_expected), ('depth_median', depth_median)):
            if wanted:
                out[name] = torch.empty((settings.height, settings.width), dtype=torch.float32, device=device)
        maps = [out[k].data_ptr() if k in out else None for k in ('alpha', 'depth', 'depth_median')]
        self._check(self.lib.fgs_inference_aux(_ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh0), _ptr(sh_rest),
                                               means.shape[0], C.byref(S), out['rgb'].data_ptr(), int(to_chw), int(clamp_output), *maps, cb, None,
                                               C.byref(st), _stream_of(device)), 'fgs_inference_aux')
        return out

    def pruning_scores(self, scores, means, scales, rotations, opacities, sh0, sh_rest, settings: RasterizerSettings) -> None:
        """Accumulates the Speedy-Splat importance scores of one view into `scores` [N] (rasterization.py:159-178)."""
        device = self._check_params((scores, means, scales, rotations, opacities, sh0, sh_rest), ('scores',) + PARAMETER_NAMES)
        if scores.numel() != means.shape[0]:
            raise RuntimeError('scores must have one entry per Gaussian')
        S, keep, buffers, cb, st = self._forward_state(settings, total_sh_rest(sh_rest), device)
        self._check(self.lib.fgs_pruning_scores(_ptr(scores), _ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh0),
                                                _ptr(sh_rest), means.shape[0], C.byref(S), cb, None, C.byref(st), _stream_of(device)),
                    'fgs_pruning_scores')

    def _scratch(self, n: int, settings: RasterizerSettings, device: torch.device) -> torch.Tensor:
        return _empty_bytes(self.lib.fgs_backward_scratch_bytes(n, int(settings.width), int(settings.height)), device)

    def _scratch_aux(self, n: int, settings: RasterizerSettings, device: torch.device) -> torch.Tensor:
        return _empty_bytes(self.lib.fgs_backward_aux_scratch_bytes(n, int(settings.width), int(settings.height)), device)

    def _scratch_pose(self, n: int, settings: RasterizerSettings, device: torch.device) -> torch.Tensor:
        return _empty_bytes(self.lib.fgs_backward_pose_scratch_bytes(n, int(settings.width), int(settings.height)), device)

    def _scratch_absgrad(self, n: int, settings: RasterizerSettings, device: torch.device) -> torch.Tensor:
        return _empty_bytes(self.lib.fgs_backward_absgrad_scratch_bytes(n, int(settings.width), int(settings.height)), device)

    def backward(self, densification_info, grad_image, image, means, scales, rotations, opacities, sh_rest, buffers, settings,
                 state, out: tuple | None = None, live_blocks: Optional[torch.Tensor] = None,
                 reached_blocks: Optional[torch.Tensor] = None, prior_blocks: Optional[torch.Tensor] = None) -> tuple:
        """`out`: optional six preallocated gradient tensors (e.g. views into one contiguous arena for a single RCCL call).
        `live_blocks`, `reached_blocks`: optional uint8 [ceil(N / 64)] on the device, filled with 1 / 0 per block of 64 Gaussians: some Gaussian of the
        block is visible / was reached by the backward blend pass. 0 = every gradient of the block is zero (still written) -- what
        adam_step_multi(live_blocks=...) needs to skip reading those zeros; `reached_blocks` flags a superset of the zero blocks.
        `prior_blocks` (with `out` and `reached_blocks`): the same kind of array going IN -- 0 = the caller promises that the block's rows of all six
        `out` tensors are zero already (the `reached_blocks` of the pass that last wrote them, untouched since); such a block is not written again
        if this pass reaches none of its Gaussians (fgs_backward_recycled)."""
        return self.backward_aux(densification_info, grad_image, None, None, image, None, means, scales, rotations, opacities, sh_rest, buffers, settings,
                                 state, out, live_blocks, reached_blocks, prior_blocks)

    def backward_aux(self, densification_info, grad_image, grad_alpha, grad_depth, image, depth, means, scales, rotations, opacities, sh_rest,
                     buffers, settings, state, out: tuple | None = None, live_blocks: Optional[torch.Tensor] = None,
                     reached_blocks: Optional[torch.Tensor] = None, prior_blocks: Optional[torch.Tensor] = None) -> tuple:
        """`backward` with upstream gradients of the maps of `forward_aux`: grad_alpha / grad_depth [H,W] or None (= zero). `depth` is the expected-depth
        map the forward pass returned (needed with grad_depth). Both None is `backward` exactly: no map is looked at, the scratch is `_scratch`'s and
        errors name fgs_backward; with a map gradient the scratch is `_scratch_aux`'s and errors name fgs_backward_aux."""
        return self._backward(densification_info, grad_image, grad_alpha, grad_depth, image, depth, means, scales, rotations, opacities, sh_rest, buffers,
                              settings, state, out, live_blocks, reached_blocks, prior_blocks)[:6]

    def backward_pose(self, densification_info, grad_image, grad_alpha, grad_depth, image, depth, means, scales, rotations, opacities, sh_rest,
                      buffers, settings, state, out: tuple | None = None, live_blocks: Optional[torch.Tensor] = None,
                      reached_blocks: Optional[torch.Tensor] = None, prior_blocks: Optional[torch.Tensor] = None,
                      w2c: bool = True, cam_position: bool = True) -> tuple:
        """`backward_aux` that also returns the gradient of the camera of `settings` (fgs_backward_pose): the six gradients, then grad_w2c [3,4] (rows
        0..2 of w2c; w2c and cam_position are independent inputs) and grad_cam_position [3] -- None for one that was not asked for. Neither asked for
        is `backward_aux` exactly. Map gradients may be None."""
        return self._backward(densification_info, grad_image, grad_alpha, grad_depth, image, depth, means, scales, rotations, opacities, sh_rest, buffers,
                              settings, state, out, live_blocks, reached_blocks, prior_blocks, (w2c, cam_position))

    def backward_absgrad(self, densification_info, abs_densification_info, grad_image, grad_alpha, grad_depth, image, depth, means, scales, rotations,
                         opacities, sh_rest, buffers, settings, state, out: tuple | None = None, live_blocks: Optional[torch.Tensor] = None,
                         reached_blocks: Optional[torch.Tensor] = None, prior_blocks: Optional[torch.Tensor] = None) -> tuple:
        """`backward_aux` that also accumulates the absolute-gradient densification statistic (fgs_backward_absgrad) into `abs_densification_info`,
        float32 [2, N] like `densification_info`: row 0 += 1 per visible Gaussian, row 1 += sqrt((0.5 W sum_p |gx_p|)^2 + (0.5 H sum_p |gy_p|)^2), the
        per-pixel shares of dL/dmean2d summed by magnitude instead of by sign. None or an empty tensor is `backward_aux` exactly. `densification_info` may be
        given as well or be None; the two may not be the same memory. Map gradients may be None."""
        return self._backward(densification_info, grad_image, grad_alpha, grad_depth, image, depth, means, scales, rotations, opacities, sh_rest, buffers,
                              settings, state, out, live_blocks, reached_blocks, prior_blocks, abs_info=abs_densification_info)[:6]

    def _backward(self, densification_info, grad_image, grad_alpha, grad_depth, image, depth, means, scales, rotations, opacities, sh_rest,
                  buffers, settings, state, out, live_blocks, reached_blocks, prior_blocks, camera: 'tuple | None' = None, abs_info=None) -> tuple:
        """The materialised-gradient backward pass behind backward / backward_aux (camera=None: fgs_backward_recycled), backward_pose
        (camera = which of (grad_w2c, grad_cam_position) are wanted: fgs_backward_pose) and backward_absgrad (abs_info: fgs_backward_absgrad): the six
        gradients + (grad_w2c, grad_cam_position)."""
        aux = grad_alpha is not None or grad_depth is not None
        want_w2c, want_cam = camera if camera is not None else (False, False)
        pose = want_w2c or want_cam
        device = self._check_params((means, scales, rotations, opacities, sh_rest), BACKWARD_PARAMETER_NAMES)
        keep: list = []
        n = means.shape[0]
        total_rest = total_sh_rest(sh_rest)
        S = self._settings(settings, total_rest, device, keep)
        grad_image = grad_image.to(dtype=torch.float32).contiguous()
        if aux:
            hw = (int(settings.height), int(settings.width))
            for name, t in (('grad_alpha', grad_alpha), ('grad_depth', grad_depth), ('depth', depth if grad_depth is not None else None)):
                if t is not None and (tuple(t.shape) != hw or t.device != device):
                    raise RuntimeError(f'{name} must be a [H,W] = {hw} tensor on the parameters\' device')
            if grad_depth is not None and depth is None:
                raise RuntimeError('backward_aux: grad_depth needs the expected-depth map of forward_aux')
            grad_alpha = grad_alpha.to(dtype=torch.float32).contiguous() if grad_alpha is not None else None
            grad_depth = grad_depth.to(dtype=torch.float32).contiguous() if grad_depth is not None else None
        depth = depth.to(dtype=torch.float32).contiguous() if grad_depth is not None else None
        grads = _gradients_out(out, gradient_shapes(n, total_rest), device)
        dens = _densification(densification_info, n, device, validate=True)
        try:
            absd = _densification(abs_info, n, device, validate=True)
        except RuntimeError as e:
            raise RuntimeError('abs_' + str(e)) from None
        _check_block_flags('live_blocks', live_blocks, n, device)
        _check_block_flags('reached_blocks', reached_blocks, n, device)
        _check_block_flags('prior_blocks', prior_blocks, n, device)
        scratch = (self._scratch_absgrad if absd is not None else self._scratch_pose if pose else self._scratch_aux if aux else self._scratch)(n, settings, device)
        st = _lib.ForwardState(*state)
        args = (_ptr(grad_image), _ptr(image), _ptr(grad_alpha), _ptr(grad_depth), _ptr(depth), _ptr(means), _ptr(scales),
                _ptr(rotations), _ptr(opacities), _ptr(sh_rest), _ptr(buffers[0]), _ptr(buffers[1]), _ptr(buffers[2]),
                _ptr(buffers[3]), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(grads[3]), _ptr(grads[4]), _ptr(grads[5]),
                _ptr(dens), scratch.data_ptr(), n, C.byref(S), C.byref(st), _ptr(live_blocks), _ptr(reached_blocks), _ptr(prior_blocks))
        if absd is not None:
            self._check(self.lib.fgs_backward_absgrad(*args, _ptr(absd), _stream_of(device)), 'fgs_backward_absgrad')
            return grads + (None, None)
        if camera is None:
            self._check(self.lib.fgs_backward_recycled(*args, _stream_of(device)), 'fgs_backward_aux' if aux else 'fgs_backward')
            return grads + (None, None)
        grad_w2c = torch.empty((3, 4), dtype=torch.float32, device=device) if want_w2c else None
        grad_cam = torch.empty(3, dtype=torch.float32, device=device) if want_cam else None
        self._check(self.lib.fgs_backward_pose(*args, _ptr(grad_w2c), _ptr(grad_cam), _stream_of(device)), 'fgs_backward_pose')
        return grads + (grad_w2c, grad_cam)

    @staticmethod
    def _check_features(features: torch.Tensor, n: int, device: torch.device) -> int:
        """The channel count F of a [N, F] feature tensor, 1..64 (an empty tensor has no address the library could be handed to refuse it itself)."""
        if features.dim() != 2 or features.shape[0] != n or features.dtype != torch.float32 or not features.is_contiguous() or features.device != device:
            raise RuntimeError(f'features must be a contiguous float32 [N, F] = [{n}, F] tensor on the parameters\' device, not '
                               f'{tuple(features.shape)} {features.dtype} on {features.device}')
        if not 1 <= features.shape[1] <= 64:
            raise RuntimeError(f'features has {features.shape[1]} channels: the feature render takes 1..64 channels')
        return int(features.shape[1])

    def blend_features(self, features: torch.Tensor, result, n_primitives: int, settings: RasterizerSettings) -> torch.Tensor:
        """fgs_blend_features: feature_map [F,H,W] = sum_i w_i features[i] over the pairs the training blend of `result` (a synchronous forward /
        forward_aux over `n_primitives` Gaussians with these settings) blended. features: float32 [N, F], any sign, 1 <= F <= 64."""
        device = result.image.device
        n = int(n_primitives)
        f = self._check_features(features, n, device)
        keep: list = []
        S = self._settings(settings, int(settings.active_sh_bases) - 1, device, keep)      # the blend reads no SH coefficient: any consistent count
        st = _lib.ForwardState(*result.state)
        fmap = torch.empty((f, int(settings.height), int(settings.width)), dtype=torch.float32, device=device)
        b = result.buffers
        self._check(self.lib.fgs_blend_features(_ptr(features), f, _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), n, C.byref(S), C.byref(st),
                                                fmap.data_ptr(), _stream_of(device)), 'fgs_blend_features')
        return fmap

    def backward_features(self, densification_info, grad_image, grad_feature_map, image, feature_map, features, means, scales, rotations, opacities,
                          sh_rest, buffers, settings, state, detach_geometry: bool = False, live_blocks: Optional[torch.Tensor] = None,
                          reached_blocks: Optional[torch.Tensor] = None) -> tuple:
        """fgs_backward_features: the six gradients of `backward` plus grad_features [N, F], for a loss that also depends on the map of
        `blend_features`. grad_feature_map [F,H,W] or None: None is `backward` exactly and the seventh result is None. detach_geometry: the feature
        term reaches grad_features only. Gradients come back in fresh tensors."""
        if grad_feature_map is None:
            return self.backward(densification_info, grad_image, image, means, scales, rotations, opacities, sh_rest, buffers, settings, state,
                                 live_blocks=live_blocks, reached_blocks=reached_blocks) + (None,)
        device = self._check_params((means, scales, rotations, opacities, sh_rest), BACKWARD_PARAMETER_NAMES)
        n = means.shape[0]
        f = self._check_features(features, n, device)
        shape = (f, int(settings.height), int(settings.width))
        for name, t in (('feature_map', feature_map), ('grad_feature_map', grad_feature_map)):
            if tuple(t.shape) != shape or t.device != device:
                raise RuntimeError(f'{name} must be a [F,H,W] = {shape} tensor on the parameters\' device')
        feature_map = feature_map.to(dtype=torch.float32).contiguous()
        grad_feature_map = grad_feature_map.to(dtype=torch.float32).contiguous()
        grad_image = grad_image.to(dtype=torch.float32).contiguous()
        keep: list = []
        total_rest = total_sh_rest(sh_rest)
        S = self._settings(settings, total_rest, device, keep)
        grads = _gradients_out(None, gradient_shapes(n, total_rest), device)
        grad_features = torch.empty((n, f), dtype=torch.float32, device=device)
        dens = _densification(densification_info, n, device, validate=True)
        _check_block_flags('live_blocks', live_blocks, n, device)
        _check_block_flags('reached_blocks', reached_blocks, n, device)
        scratch = self._scratch(n, settings, device)
        st = _lib.ForwardState(*state)
        self._check(self.lib.fgs_backward_features(
            _ptr(grad_image), _ptr(image), None, None, None, _ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh_rest),
            _ptr(buffers[0]), _ptr(buffers[1]), _ptr(buffers[2]), _ptr(buffers[3]), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(grads[3]),
            _ptr(grads[4]), _ptr(grads[5]), _ptr(dens), scratch.data_ptr(), n, C.byref(S), C.byref(st), _ptr(live_blocks), _ptr(reached_blocks),
            _ptr(features), f, _ptr(feature_map), grad_feature_map.data_ptr(), _ptr(grad_features),
            int(bool(detach_geometry)), _stream_of(device)), 'fgs_backward_features')
        return grads + (grad_features,)

    @staticmethod
    def _check_distortion_means(means: torch.Tensor, n: int, device: torch.device) -> None:
        if means.dim() != 2 or tuple(means.shape) != (n, 3) or means.dtype != torch.float32 or not means.is_contiguous() or means.device != device:
            raise RuntimeError(f'means must be a contiguous float32 [N, 3] = [{n}, 3] tensor on the device of the forward pass, not '
                               f'{tuple(means.shape)} {means.dtype} on {means.device}')

    def blend_distortion(self, means: torch.Tensor, result, n_primitives: int, settings: RasterizerSettings, normalized: bool = True) -> torch.Tensor:
        """fgs_blend_distortion: the depth-distortion state [3,H,W] of the pairs the training blend of `result` (a synchronous forward / forward_aux
        over `n_primitives` Gaussians with these means and settings) blended. Plane 0 is the map X = sum_ab w_a w_b |t_a - t_b|, t = the view-space
        depth (normalized=False) or its mapping onto [0, 1) with the settings' near and far planes; planes 1 and 2 are `backward_distortion`'s."""
        device = result.image.device
        n = int(n_primitives)
        self._check_distortion_means(means, n, device)
        keep: list = []
        S = self._settings(settings, int(settings.active_sh_bases) - 1, device, keep)      # the blend reads no SH coefficient: any consistent count
        st = _lib.ForwardState(*result.state)
        dstate = torch.empty((3, int(settings.height), int(settings.width)), dtype=torch.float32, device=device)
        b = result.buffers
        self._check(self.lib.fgs_blend_distortion(_ptr(means), _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), n, C.byref(S), C.byref(st),
                                                  _lib.DISTORTION_NORMALIZED if normalized else _lib.DISTORTION_LINEAR, dstate.data_ptr(),
                                                  _stream_of(device)), 'fgs_blend_distortion')
        return dstate

    def backward_distortion(self, densification_info, grad_image, grad_distortion, image, distortion_state, means, scales, rotations, opacities,
                            sh_rest, buffers, settings, state, normalized: bool = True, live_blocks: Optional[torch.Tensor] = None,
                            reached_blocks: Optional[torch.Tensor] = None) -> tuple:
        """fgs_backward_distortion: the six gradients of `backward` for a loss that also depends on plane 0 of `blend_distortion`'s state (same
        `normalized`). grad_distortion [H,W] or None: None is `backward` exactly. Gradients come back in fresh tensors."""
        if grad_distortion is None:
            return self.backward(densification_info, grad_image, image, means, scales, rotations, opacities, sh_rest, buffers, settings, state,
                                 live_blocks=live_blocks, reached_blocks=reached_blocks)
        device = self._check_params((means, scales, rotations, opacities, sh_rest), BACKWARD_PARAMETER_NAMES)
        n = means.shape[0]
        hw = (int(settings.height), int(settings.width))
        if tuple(grad_distortion.shape) != hw or grad_distortion.device != device:
            raise RuntimeError(f'grad_distortion must be a [H,W] = {hw} tensor on the parameters\' device')
        if tuple(distortion_state.shape) != (3,) + hw or distortion_state.device != device:
            raise RuntimeError(f'distortion_state must be the [3,H,W] = {(3,) + hw} tensor blend_distortion returned')
        distortion_state = distortion_state.to(dtype=torch.float32).contiguous()
        grad_distortion = grad_distortion.to(dtype=torch.float32).contiguous()
        grad_image = grad_image.to(dtype=torch.float32).contiguous()
        keep: list = []
        total_rest = total_sh_rest(sh_rest)
        S = self._settings(settings, total_rest, device, keep)
        grads = _gradients_out(None, gradient_shapes(n, total_rest), device)
        dens = _densification(densification_info, n, device, validate=True)
        _check_block_flags('live_blocks', live_blocks, n, device)
        _check_block_flags('reached_blocks', reached_blocks, n, device)
        scratch = self._scratch_aux(n, settings, device)                # dL/dz of the distortion term lives in the aux layout's acc_z
        st = _lib.ForwardState(*state)
        self._check(self.lib.fgs_backward_distortion(
            _ptr(grad_image), _ptr(image), None, None, None, _ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh_rest),
            _ptr(buffers[0]), _ptr(buffers[1]), _ptr(buffers[2]), _ptr(buffers[3]), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(grads[3]),
            _ptr(grads[4]), _ptr(grads[5]), _ptr(dens), scratch.data_ptr(), n, C.byref(S), C.byref(st), _ptr(live_blocks), _ptr(reached_blocks),
            _ptr(distortion_state), grad_distortion.data_ptr(), _lib.DISTORTION_NORMALIZED if normalized else _lib.DISTORTION_LINEAR,
            _stream_of(device)), 'fgs_backward_distortion')
        return grads

    @staticmethod
    def _check_surface_features(surface_features: torch.Tensor, n: int, device: torch.device) -> None:
        f = surface_features
        if f.dim() != 2 or tuple(f.shape) != (n, 5) or f.dtype != torch.float32 or not f.is_contiguous() or f.device != device:
            raise RuntimeError(f'surface_features must be a contiguous float32 [N, 5] = [{n}, 5] tensor on the device of the forward pass, not '
                               f'{tuple(f.shape)} {f.dtype} on {f.device}')

    def blend_geometry(self, means: torch.Tensor, surface_features: torch.Tensor, result, n_primitives: int, settings: RasterizerSettings,
                       normalized: bool = True) -> torch.Tensor:
        """fgs_blend_geometry: the state [8,H,W] of the one walk that carries the depth-distortion map and the blend of five per-Gaussian channels over
        the pairs the training blend of `result` (a synchronous forward / forward_aux over `n_primitives` Gaussians with these means and settings)
        blended. Plane 0 is `blend_distortion`'s map X (same `normalized`), state[2:7] is `blend_features`' map of `surface_features` [N, 5], a
        contiguous [5,H,W] that `normal_consistency` takes as it is; planes 1 and 7 are `backward_geometry`'s."""
        device = result.image.device
        n = int(n_primitives)
        self._check_distortion_means(means, n, device)
        self._check_surface_features(surface_features, n, device)
        keep: list = []
        S = self._settings(settings, int(settings.active_sh_bases) - 1, device, keep)      # the blend reads no SH coefficient: any consistent count
        st = _lib.ForwardState(*result.state)
        gstate = torch.empty((8, int(settings.height), int(settings.width)), dtype=torch.float32, device=device)
        b = result.buffers
        self._check(self.lib.fgs_blend_geometry(_ptr(means), _ptr(surface_features), _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), n, C.byref(S), C.byref(st),
                                                _lib.DISTORTION_NORMALIZED if normalized else _lib.DISTORTION_LINEAR, gstate.data_ptr(),
                                                _stream_of(device)), 'fgs_blend_geometry')
        return gstate

    def backward_geometry(self, densification_info, grad_image, grad_distortion, grad_surface_map, image, geometry_state, surface_features, means,
                          scales, rotations, opacities, sh_rest, buffers, settings, state, normalized: bool = True,
                          live_blocks: Optional[torch.Tensor] = None, reached_blocks: Optional[torch.Tensor] = None) -> tuple:
        """fgs_backward_geometry: the six gradients of `backward` plus grad_surface_features [N, 5], for a loss that also depends on plane 0 and / or
        planes 2..6 of `blend_geometry`'s state (same `normalized`, same features). grad_distortion [H,W] and grad_surface_map [5,H,W], either or
        both None: both None is `backward` exactly and the seventh result is None. Gradients come back in fresh tensors."""
        if grad_distortion is None and grad_surface_map is None:
            return self.backward(densification_info, grad_image, image, means, scales, rotations, opacities, sh_rest, buffers, settings, state,
                                 live_blocks=live_blocks, reached_blocks=reached_blocks) + (None,)
        device = self._check_params((means, scales, rotations, opacities, sh_rest), BACKWARD_PARAMETER_NAMES)
        n = means.shape[0]
        hw = (int(settings.height), int(settings.width))
        self._check_surface_features(surface_features, n, device)
        if grad_distortion is not None and (tuple(grad_distortion.shape) != hw or grad_distortion.device != device):
            raise RuntimeError(f'grad_distortion must be a [H,W] = {hw} tensor on the parameters\' device')
        if grad_surface_map is not None and (tuple(grad_surface_map.shape) != (5,) + hw or grad_surface_map.device != device):
            raise RuntimeError(f'grad_surface_map must be a [5,H,W] = {(5,) + hw} tensor on the parameters\' device')
        if tuple(geometry_state.shape) != (8,) + hw or geometry_state.device != device:
            raise RuntimeError(f'geometry_state must be the [8,H,W] = {(8,) + hw} tensor blend_geometry returned')
        geometry_state = geometry_state.to(dtype=torch.float32).contiguous()
        grad_distortion = grad_distortion.to(dtype=torch.float32).contiguous() if grad_distortion is not None else None
        grad_surface_map = grad_surface_map.to(dtype=torch.float32).contiguous() if grad_surface_map is not None else None
        grad_image = grad_image.to(dtype=torch.float32).contiguous()
        keep: list = []
        total_rest = total_sh_rest(sh_rest)
        S = self._settings(settings, total_rest, device, keep)
        grads = _gradients_out(None, gradient_shapes(n, total_rest), device)
        grad_features = torch.empty((n, 5), dtype=torch.float32, device=device)
        dens = _densification(densification_info, n, device, validate=True)
        _check_block_flags('live_blocks', live_blocks, n, device)
        _check_block_flags('reached_blocks', reached_blocks, n, device)
        scratch = self._scratch_aux(n, settings, device)                # dL/dz of the distortion term lives in the aux layout's acc_z
        st = _lib.ForwardState(*state)
        self._check(self.lib.fgs_backward_geometry(
            _ptr(grad_image), _ptr(image), None, None, None, _ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh_rest),
            _ptr(buffers[0]), _ptr(buffers[1]), _ptr(buffers[2]), _ptr(buffers[3]), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(grads[3]),
            _ptr(grads[4]), _ptr(grads[5]), _ptr(dens), scratch.data_ptr(), n, C.byref(S), C.byref(st), _ptr(live_blocks), _ptr(reached_blocks),
            _ptr(surface_features), _ptr(geometry_state), _ptr(grad_distortion), _ptr(grad_surface_map), _ptr(grad_features),
            _lib.DISTORTION_NORMALIZED if normalized else _lib.DISTORTION_LINEAR, _stream_of(device)), 'fgs_backward_geometry')
        return grads + (grad_features,)

    def backward_adam_fused(self, densification_info, grad_image, image, params: Sequence[torch.Tensor], exp_avgs, exp_avg_sqs,
                            buffers, settings, state, step: int, lrs: Sequence[float], betas=(0.9, 0.999), eps: float = 1e-15,
                            grad_alpha=None, grad_depth=None, grad_feature_map=None, grad_distortion=None, grad_geometry=None) -> None:
        """params / moments / lrs in optimizer-group order: means, sh0, sh_rest, opacities, scales, rotations (Model.py:238-245)."""
        if grad_alpha is not None or grad_depth is not None:
            raise RuntimeError('backward_adam_fused takes no alpha / depth gradients: use backward_aux and an optimizer step of its own')
        if grad_feature_map is not None:
            raise RuntimeError('backward_adam_fused takes no feature-map gradient: use backward_features and an optimizer step of its own')
        if grad_distortion is not None:
            raise RuntimeError('backward_adam_fused takes no distortion gradient: use backward_distortion and an optimizer step of its own')
        if grad_geometry is not None:
            raise RuntimeError('backward_adam_fused takes no geometry gradient: use backward_geometry and an optimizer step of its own')
        device = self._check_params(tuple(params) + tuple(exp_avgs) + tuple(exp_avg_sqs), ['param/moment'] * 18)
        keep: list = []
        n = params[0].shape[0]
        S = self._settings(settings, total_sh_rest(params[2]), device, keep)
        grad_image = grad_image.to(dtype=torch.float32).contiguous()
        dens = _densification(densification_info, n, device, validate=False)
        scratch = self._scratch(n, settings, device)
        st = _lib.ForwardState(*state)
        lr_arr = (C.c_double * 6)(*[float(x) for x in lrs])
        self._check(self.lib.fgs_backward_adam_fused(_ptr(grad_image), _ptr(image), _pointer_array(params, 6), _pointer_array(exp_avgs, 6),
                                                     _pointer_array(exp_avg_sqs, 6), _ptr(buffers[0]), _ptr(buffers[1]), _ptr(buffers[2]),
                                                     _ptr(buffers[3]), _ptr(dens), scratch.data_ptr(), n, C.byref(S), C.byref(st), int(step), lr_arr,
                                                     float(betas[0]), float(betas[1]), float(eps), _stream_of(device)),
                    'fgs_backward_adam_fused')

    def adam_step(self, grad, param, exp_avg, exp_avg_sq, step: int, lr: float, beta1: float, beta2: float, eps: float) -> None:
        device = self._check_params((grad, param, exp_avg, exp_avg_sq), ('param_grad', 'param', 'exp_avg', 'exp_avg_sq'))
        self._check(self.lib.fgs_adam_step(_ptr(grad), _ptr(param), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), int(step),
                                           float(lr), float(beta1), float(beta2), float(eps), _stream_of(device)), 'fgs_adam_step')

    def adam_step_multi(self, grads, params, exp_avgs, exp_avg_sqs, steps, lrs, beta1: float, beta2: float, eps: float,
                        live_blocks: Optional[torch.Tensor] = None, quiet_blocks: Optional[torch.Tensor] = None) -> None:
        """`live_blocks` (as filled by backward(live_blocks=...) for EXACTLY these gradient tensors, all of them [N, ...]): a promise that the
        gradient rows of blocks flagged 0 are zero; they are not read. The result is bit-identical either way.
        `quiet_blocks` (uint8 [ceil(N / 64)], the caller's own; fgs_adam_step_multi_quiet): 1 = a promise that both moments of the block are zero in
        every group. Blocks that are quiet and not live are neither read nor written (the identity); the call clears the flag of every block it
        reads a gradient for, and ALL flags if it cannot use them (no live_blocks, eps <= 0, a step size that is not finite)."""
        k = len(params)
        if k == 0:
            return
        device = self._check_params(tuple(grads) + tuple(params) + tuple(exp_avgs) + tuple(exp_avg_sqs), ['adam tensor'] * (4 * k))
        rows = None
        if live_blocks is not None or quiet_blocks is not None:
            n = params[0].shape[0]
            if any(p.dim() < 1 or p.shape[0] != n for p in params) or n == 0:
                raise RuntimeError('live_blocks / quiet_blocks need parameter tensors that all have one row per Gaussian')
            _check_block_flags('live_blocks', live_blocks, n, device)
            _check_block_flags('quiet_blocks', quiet_blocks, n, device)
            rows = (C.c_int32 * k)(*[p.numel() // n for p in params])
        self._check(self.lib.fgs_adam_step_multi_quiet(k, _pointer_array(grads, k), _pointer_array(params, k), _pointer_array(exp_avgs, k),
                                                       _pointer_array(exp_avg_sqs, k),
                                                       (C.c_int64 * k)(*[p.numel() for p in params]), (C.c_int32 * k)(*[int(s) for s in steps]),
                                                       (C.c_double * k)(*[float(x) for x in lrs]), float(beta1), float(beta2), float(eps),
                                                       _ptr(live_blocks), rows, _ptr(quiet_blocks), _stream_of(device)), 'fgs_adam_step_multi')

    def adam_quiet_scan(self, exp_avgs, exp_avg_sqs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [ceil(N / 64)]: 1 where every element of both moments of the block of 64 Gaussians is zero in every group (all [N, ...], one N):
        the `quiet_blocks` of adam_step_multi, from one streaming read of the moments (fgs_adam_quiet_scan)."""
        k = len(exp_avgs)
        device = self._check_params(tuple(exp_avgs) + tuple(exp_avg_sqs), ['adam moment'] * (2 * k))
        n = exp_avgs[0].shape[0]
        if any(t.dim() < 1 or t.shape[0] != n for t in tuple(exp_avgs) + tuple(exp_avg_sqs)) or n == 0 or any(
                m.shape != v.shape for m, v in zip(exp_avgs, exp_avg_sqs)):
            raise RuntimeError('adam_quiet_scan needs moment tensors that all have one row per Gaussian')
        if out is None:
            out = torch.empty((n + 63) // 64, dtype=torch.uint8, device=device)
        else:
            _check_block_flags('quiet_blocks', out, n, device, owner='moments')
        self._check(self.lib.fgs_adam_quiet_scan(k, _pointer_array(exp_avgs, k), _pointer_array(exp_avg_sqs, k),
                                                 (C.c_int64 * k)(*[t.numel() for t in exp_avgs]),
                                                 (C.c_int32 * k)(*[t.numel() // n for t in exp_avgs]), _ptr(out), _stream_of(device)),
                    'fgs_adam_quiet_scan')
        return out

    @staticmethod
    def _loss_weight(weight, image: torch.Tensor) -> torch.Tensor:
        """The [H,W] per-pixel weight of the weighted loss as the library takes it: float32, contiguous, on the image's device."""
        if not isinstance(weight, torch.Tensor) or weight.dim() != 2 or tuple(weight.shape) != tuple(image.shape[1:]):
            raise RuntimeError(f'l1_dssim: weight must be a [H,W] tensor matching the image ({tuple(image.shape[1:])}), got '
                               f'{tuple(weight.shape) if isinstance(weight, torch.Tensor) else type(weight).__name__}')
        if weight.device != image.device:
            raise RuntimeError(f'l1_dssim: weight lives on {weight.device}, the image on {image.device}')
        if weight.is_complex():
            raise RuntimeError('l1_dssim: weight must be real (float, integer or bool)')
        return weight.to(torch.float32).contiguous()

    def _l1_dssim(self, image: torch.Tensor, target: torch.Tensor, lambda_l1: float, lambda_dssim: float, with_grad: bool, weight=None) -> tuple:
        """fgs_l1_dssim_loss: (sums = (l1, ssim, loss) formed on the device by the reduce kernel, dloss/dimage or None, the scratch with the derivative maps).
        With a weight: fgs_l1_dssim_weighted_loss, the same triple of the weighted definition."""
        device = self._check_params((image, target), ('image', 'target'))
        if image.dim() != 3 or image.shape[0] != 3 or image.shape != target.shape:
            raise RuntimeError('l1_dssim expects two [3,H,W] tensors')
        _, h, w = image.shape
        if weight is not None:
            weight = self._loss_weight(weight, image)
        sums = torch.empty(3, dtype=torch.float32, device=device)
        grad = torch.empty_like(image) if with_grad else None
        if weight is None:
            scratch = torch.empty(int(self.lib.fgs_l1_dssim_scratch_bytes(w, h)), dtype=torch.uint8, device=device)
            self._check(self.lib.fgs_l1_dssim_loss(image.data_ptr(), target.data_ptr(), w, h, float(lambda_l1), float(lambda_dssim),
                                                   sums.data_ptr(), _ptr(grad), scratch.data_ptr(), _stream_of(device)), 'fgs_l1_dssim_loss')
        else:
            scratch = torch.empty(int(self.lib.fgs_l1_dssim_weighted_scratch_bytes(w, h)), dtype=torch.uint8, device=device)
            self._check(self.lib.fgs_l1_dssim_weighted_loss(image.data_ptr(), target.data_ptr(), weight.data_ptr(), w, h, float(lambda_l1), float(lambda_dssim),
                                                            sums.data_ptr(), _ptr(grad), scratch.data_ptr(), _stream_of(device)), 'fgs_l1_dssim_weighted_loss')
        return sums, grad, scratch

    def l1_dssim(self, image: torch.Tensor, target: torch.Tensor, lambda_l1: float = 0.8, lambda_dssim: float = 0.2,
                 with_grad: bool = True, weight: Optional[torch.Tensor] = None):
        """Fused photometric loss (Loss.py:15-16): returns (loss 0-dim tensor, dloss/dimage or None, (l1, ssim) tensor).
        `weight`: [H,W] per-pixel weights (masks, confidences) of the weighted loss of INTEGRATION.md -- w > 0 counts as w, anything else as 0, and a
        pixel that does not count is replaced by the target before the SSIM windows are formed; its gradient is exactly 0. None: the unweighted loss."""
        sums, grad, _ = self._l1_dssim(image, target, lambda_l1, lambda_dssim, with_grad, weight)
        return sums[2], grad, sums[:2]

    def l1_dssim_forward(self, image: torch.Tensor, target: torch.Tensor, lambda_l1: float = 0.8, lambda_dssim: float = 0.2,
                         weight: Optional[torch.Tensor] = None):
        """The loss value alone: returns (loss 0-dim tensor, (l1, ssim) tensor, scratch). `scratch` holds the derivative maps that
        l1_dssim_backward turns into dloss/dimage -- the shape of an autograd loss node (forward saves, backward launches one kernel).
        `weight` as in l1_dssim; hand the same one to l1_dssim_backward."""
        sums, _, scratch = self._l1_dssim(image, target, lambda_l1, lambda_dssim, False, weight)
        return sums[2], sums[:2], scratch

    def l1_dssim_backward(self, image: torch.Tensor, target: torch.Tensor, scratch: torch.Tensor, upstream: Optional[torch.Tensor] = None,
                          lambda_l1: float = 0.8, lambda_dssim: float = 0.2, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dloss/dimage * upstream from the maps of l1_dssim_forward (same image / target / weight). `upstream`: a float32 scalar tensor on the
        device (dL/dloss), folded into the kernel -- no `grad * upstream` pass over the image -- or None for 1. The weight itself gets no gradient."""
        device = self._check_params((image, target), ('image', 'target'))
        _, h, w = image.shape
        if weight is not None:
            weight = self._loss_weight(weight, image)
        need = self.lib.fgs_l1_dssim_scratch_bytes(w, h) if weight is None else self.lib.fgs_l1_dssim_weighted_scratch_bytes(w, h)
        if scratch.device != device or scratch.numel() < int(need):
            raise RuntimeError('l1_dssim_backward: scratch is not the buffer l1_dssim_forward returned for this image size')
        if upstream is not None:
            if upstream.device != device or upstream.dtype != torch.float32 or upstream.numel() != 1:
                raise RuntimeError('l1_dssim_backward: upstream must be one float32 on the device of the image')
            upstream = upstream.reshape(1).contiguous()
        grad = torch.empty_like(image)
        if weight is None:
            self._check(self.lib.fgs_l1_dssim_backward(image.data_ptr(), target.data_ptr(), w, h, float(lambda_l1), float(lambda_dssim),
                                                       _ptr(upstream), grad.data_ptr(), scratch.data_ptr(), _stream_of(device)), 'fgs_l1_dssim_backward')
        else:
            self._check(self.lib.fgs_l1_dssim_weighted_backward(image.data_ptr(), target.data_ptr(), weight.data_ptr(), w, h, float(lambda_l1),
                                                                float(lambda_dssim), _ptr(upstream), grad.data_ptr(), scratch.data_ptr(),
                                                                _stream_of(device)), 'fgs_l1_dssim_weighted_backward')
        return grad

    # -- per-view bilateral-grid colour correction (include/fgs_hip.h, csrc/bilagrid.hip) ------------------------------------------
    @staticmethod
    def _check_bilagrid(grid: torch.Tensor, image: Optional[torch.Tensor] = None, grad_out: Optional[torch.Tensor] = None) -> tuple:
        """(device, (Wg, Hg, L), (W, H)) of a [12, L, Hg, Wg] grid and, if given, a [3,H,W] image (and an upstream gradient of its shape)."""
        tensors, names = [grid], ['grid']
        if image is not None:
            tensors.append(image); names.append('image')
        if grad_out is not None:
            tensors.append(grad_out); names.append('grad_out')
        for t, n in zip(tensors, names):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != grid.device:
                raise RuntimeError(f"bilagrid: '{n}' must be a contiguous float32 tensor on {grid.device}")
        if grid.dim() != 4 or grid.shape[0] != 12 or min(grid.shape) < 1:
            raise RuntimeError(f'bilagrid: grid must be [12, L, Hg, Wg] with every extent >= 1, got {tuple(grid.shape)}')
        if image is not None and (image.dim() != 3 or image.shape[0] != 3 or image.numel() == 0):
            raise RuntimeError(f'bilagrid: image must be [3, H, W], got {tuple(image.shape)}')
        if grad_out is not None and grad_out.shape != image.shape:
            raise RuntimeError(f'bilagrid: grad_out must have the shape of the image {tuple(image.shape)}, got {tuple(grad_out.shape)}')
        _, gl, gh, gw = grid.shape
        return grid.device, (gw, gh, gl), (None if image is None else (image.shape[2], image.shape[1]))

    def _scratch_bilagrid(self, extents: tuple, device: torch.device) -> torch.Tensor:
        return _empty_bytes(self.lib.fgs_bilagrid_scratch_bytes(*extents), device)

    def bilagrid_staged(self, grid_shape: tuple, width: int, height: int) -> bool:
        """Whether the slice kernels stage the lattice points under a pixel tile in LDS for a [12, L, Hg, Wg] grid over a W x H image (else: global reads)."""
        _, gl, gh, gw = grid_shape
        st = self.lib.fgs_bilagrid_staged(int(gw), int(gh), int(gl), int(width), int(height))
        if st < 0:
            self._check(st, 'fgs_bilagrid_staged')
        return bool(st)

    def bilagrid_slice(self, image: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
        """image' = A(x, y, luma) image + b(x, y, luma) with the 3 x 4 matrix sliced out of `grid` per pixel: [3,H,W] -> [3,H,W]."""
        device, ext, (w, h) = self._check_bilagrid(grid, image)
        out = torch.empty_like(image)
        self._check(self.lib.fgs_bilagrid_slice(grid.data_ptr(), *ext, image.data_ptr(), w, h, out.data_ptr(), _stream_of(device)), 'fgs_bilagrid_slice')
        return out

    def bilagrid_slice_backward(self, image: torch.Tensor, grid: torch.Tensor, grad_out: torch.Tensor, need_grid: bool = True,
                                need_image: bool = True) -> tuple:
        """(dL/dgrid or None, dL/dimage or None) for the upstream gradient of bilagrid_slice's output; a gradient that is not needed is not computed."""
        device, ext, (w, h) = self._check_bilagrid(grid, image, grad_out)
        grad_grid = torch.empty_like(grid) if need_grid else None
        grad_image = torch.empty_like(image) if need_image else None
        scratch = self._scratch_bilagrid(ext, device) if need_grid else None
        self._check(self.lib.fgs_bilagrid_slice_backward(grid.data_ptr(), *ext, image.data_ptr(), grad_out.data_ptr(), w, h, _ptr(grad_grid), _ptr(grad_image),
                                                         _ptr(scratch), _stream_of(device)), 'fgs_bilagrid_slice_backward')
        return grad_grid, grad_image

    def bilagrid_tv(self, grid: torch.Tensor, with_grad: bool = True) -> tuple:
        """(tv(grid) as a 0-dim device tensor, d tv / d grid or None): the sum over the three axes of the mean squared difference of neighbours."""
        device, ext, _ = self._check_bilagrid(grid)
        loss = torch.empty((), dtype=torch.float32, device=device)
        grad = torch.empty_like(grid) if with_grad else None
        self._check(self.lib.fgs_bilagrid_tv(grid.data_ptr(), *ext, loss.data_ptr(), _ptr(grad), _stream_of(device)), 'fgs_bilagrid_tv')
        return loss, grad

    # -- normal-consistency regulariser (include/fgs_hip.h, csrc/normal_consistency.hip) ---------------------------------------------
    @staticmethod
    def _check_surface(means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, w2c: torch.Tensor, cam_position: torch.Tensor,
                       grad_features: Optional[torch.Tensor] = None) -> tuple:
        """(device, N, w2c, cam_position as contiguous float32 tensors on the device) of the [N,3] / [N,3] / [N,4] tensors of a Gaussian set and a camera."""
        tensors, names = [means, scales, rotations], ['means', 'scales', 'rotations']
        if grad_features is not None:
            tensors.append(grad_features); names.append('grad_features')
        for t, name in zip(tensors, names):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != means.device:
                raise RuntimeError(f"surface_features: '{name}' must be a contiguous float32 tensor on {means.device}")
        n = means.shape[0]
        if tuple(means.shape) != (n, 3) or tuple(scales.shape) != (n, 3) or tuple(rotations.shape) != (n, 4):
            raise RuntimeError(f'surface_features: means, scales, rotations must be [N,3], [N,3], [N,4], got {tuple(means.shape)}, {tuple(scales.shape)}, '
                               f'{tuple(rotations.shape)}')
        if grad_features is not None and tuple(grad_features.shape) != (n, 5):
            raise RuntimeError(f'surface_features: grad_features must be [N,5] = {(n, 5)}, got {tuple(grad_features.shape)}')
        w2c = w2c.detach().to(device=means.device, dtype=torch.float32).contiguous()
        cam = cam_position.detach().to(device=means.device, dtype=torch.float32).contiguous()
        if w2c.dim() != 2 or w2c.shape[0] < 3 or w2c.shape[1] != 4 or cam.numel() != 3:
            raise RuntimeError(f'surface_features: w2c must be [3,4] or [4,4] and cam_position have 3 entries, got {tuple(w2c.shape)}, {tuple(cam.shape)}')
        return means.device, n, w2c, cam

    def surface_features(self, means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, w2c: torch.Tensor, cam_position: torch.Tensor) -> torch.Tensor:
        """[N,5] rows (n_cam, z, 1): the camera-space normal of every Gaussian (the axis of its smallest scale, turned towards the camera), the
        view-space depth of its mean, and one -- the channels diff_rasterize_features blends into the map normal_consistency reads."""
        device, n, w2c, cam = self._check_surface(means, scales, rotations, w2c, cam_position)
        features = torch.empty((n, 5), dtype=torch.float32, device=device)
        self._check(self.lib.fgs_surface_features(_ptr(means), _ptr(scales), _ptr(rotations), n, w2c.data_ptr(), cam.data_ptr(), _ptr(features),
                                                  _stream_of(device)), 'fgs_surface_features')
        return features

    def surface_features_backward(self, means: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, w2c: torch.Tensor, cam_position: torch.Tensor,
                                  grad_features: torch.Tensor, need_rotations: bool = True, need_means: bool = True) -> tuple:
        """(dL/drotations [N,4] or None, dL/dmeans [N,3] or None) for the upstream gradient of surface_features' output; a gradient that is not needed
        is not computed. The scales get none (the choice of the axis and its sign are piecewise constant)."""
        device, n, w2c, cam = self._check_surface(means, scales, rotations, w2c, cam_position, grad_features)
        grad_rotations = torch.empty_like(rotations) if need_rotations else None
        grad_means = torch.empty_like(means) if need_means else None
        self._check(self.lib.fgs_surface_features_backward(_ptr(means), _ptr(scales), _ptr(rotations), n, w2c.data_ptr(), cam.data_ptr(), _ptr(grad_features),
                                                           int(need_rotations), int(need_means), _ptr(grad_rotations), _ptr(grad_means), _stream_of(device)),
                    'fgs_surface_features_backward')
        return grad_rotations, grad_means

    @staticmethod
    def _check_surface_map(surface_map: torch.Tensor, settings: RasterizerSettings, grad: Optional[torch.Tensor] = None) -> tuple:
        """(device, (W, H), (fx, fy, cx, cy)) of a [5,H,W] map of the settings' image size (and an upstream gradient [H,W])."""
        for t, name in ((surface_map, 'surface_map'),) + (((grad, 'grad_consistency'),) if grad is not None else ()):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != surface_map.device:
                raise RuntimeError(f"normal_consistency: '{name}' must be a contiguous float32 tensor on {surface_map.device}")
        w, h = int(settings.width), int(settings.height)
        if tuple(surface_map.shape) != (5, h, w) or surface_map.numel() == 0:
            raise RuntimeError(f'normal_consistency: surface_map must be [5, H, W] = {(5, h, w)}, got {tuple(surface_map.shape)}')
        if grad is not None and tuple(grad.shape) != (h, w):
            raise RuntimeError(f'normal_consistency: grad_consistency must be [H, W] = {(h, w)}, got {tuple(grad.shape)}')
        return surface_map.device, (w, h), (float(settings.focal_x), float(settings.focal_y), float(settings.center_x), float(settings.center_y))

    def normal_consistency(self, surface_map: torch.Tensor, settings: RasterizerSettings, min_alpha: float = 0.5, return_normals: bool = False) -> tuple:
        """(E [H,W], n_d [3,H,W] or None) of a blended map [5,H,W] = (N_r, D, A): E = A - N_r . n_d where the depth normal n_d exists, 0 elsewhere."""
        device, size, intrinsics = self._check_surface_map(surface_map, settings)
        E = torch.empty(surface_map.shape[1:], dtype=torch.float32, device=device)
        normals = torch.empty((3, *surface_map.shape[1:]), dtype=torch.float32, device=device) if return_normals else None
        self._check(self.lib.fgs_normal_consistency(surface_map.data_ptr(), *size, *intrinsics, float(min_alpha), E.data_ptr(), _ptr(normals),
                                                    _stream_of(device)), 'fgs_normal_consistency')
        return E, normals

    def normal_consistency_backward(self, surface_map: torch.Tensor, grad_consistency: torch.Tensor, settings: RasterizerSettings,
                                    min_alpha: float = 0.5) -> torch.Tensor:
        """dL/dsurface_map [5,H,W] for the upstream gradient of E; every element is written, bit-reproducibly (a gather, no float atomics)."""
        device, size, intrinsics = self._check_surface_map(surface_map, settings, grad_consistency)
        grad_map = torch.empty_like(surface_map)
        self._check(self.lib.fgs_normal_consistency_backward(surface_map.data_ptr(), grad_consistency.data_ptr(), *size, *intrinsics, float(min_alpha),
                                                             grad_map.data_ptr(), _stream_of(device)), 'fgs_normal_consistency_backward')
        return grad_map

    # -- TSDF fusion and mesh extraction (include/fgs_hip.h, csrc/tsdf.hip) ------------------------------------------------------
    @staticmethod
    def _check_volume(tsdf_weight: torch.Tensor, color: Optional[torch.Tensor]) -> tuple:
        """(device, (nx, ny, nz)) of a [nz,ny,nx,2] state tensor and, if given, its planar [3,nz,ny,nx] colour volume."""
        if not isinstance(tsdf_weight, torch.Tensor) or tsdf_weight.dtype != torch.float32 or not tsdf_weight.is_contiguous() or tsdf_weight.dim() != 4 \
                or tsdf_weight.shape[3] != 2:
            raise RuntimeError('tsdf: tsdf_weight must be a contiguous float32 [nz, ny, nx, 2] tensor')
        nz, ny, nx, _ = tsdf_weight.shape
        if color is not None and (color.dtype != torch.float32 or not color.is_contiguous() or color.device != tsdf_weight.device
                                  or tuple(color.shape) != (3, nz, ny, nx)):
            raise RuntimeError(f'tsdf: color must be a contiguous float32 [3, {nz}, {ny}, {nx}] tensor on {tsdf_weight.device}')
        return tsdf_weight.device, (int(nx), int(ny), int(nz))

    def tsdf_integrate(self, tsdf_weight: torch.Tensor, color: Optional[torch.Tensor], origin: Sequence[float], voxel_size: float, trunc: float,
                       settings_list: Sequence[RasterizerSettings], depths: Sequence[torch.Tensor], alphas: Optional[Sequence] = None,
                       colors: Optional[Sequence] = None, near: Optional[float] = None, depth_max: float = math.inf, min_alpha: float = 0.5,
                       max_weight: float = 65536.0) -> None:
        """Folds 1..8 views of one size into the volume IN PLACE, one launch (fgs_tsdf_integrate). near: None = the first view's near plane."""
        device, dims = self._check_volume(tsdf_weight, color)
        k = len(settings_list)
        if len(depths) != k or (alphas is not None and len(alphas) != k) or (colors is not None and len(colors) != k):
            raise RuntimeError('tsdf_integrate: one depth (and opacity / colour) map per view')
        if color is not None and colors is None:
            raise RuntimeError('tsdf_integrate: the volume has colour, the views have no colour maps')
        w, h = (int(settings_list[0].width), int(settings_list[0].height)) if k else (0, 0)
        views, keep = (_lib.TsdfView * max(k, 1))(), []
        for v, s in enumerate(settings_list):
            if (int(s.width), int(s.height)) != (w, h):
                raise RuntimeError('tsdf_integrate: the views of one call must have one image size')
            maps = {'depth': (depths[v], (h, w)), 'alpha': (None if alphas is None else alphas[v], (h, w)), 'color': (None if colors is None else colors[v], (3, h, w))}
            for name, (t, shape) in maps.items():
                if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != device or tuple(t.shape) != shape):
                    raise RuntimeError(f"tsdf_integrate: '{name}' of view {v} must be a contiguous float32 {shape} tensor on {device}")
            w2c = s.w2c.to(device=device, dtype=torch.float32).contiguous()
            if w2c.numel() < 12:
                raise ValueError('w2c needs >= 3x4 entries')
            keep.append(w2c)
            views[v] = _lib.TsdfView(w2c.data_ptr(), float(s.focal_x), float(s.focal_y), float(s.center_x), float(s.center_y), depths[v].data_ptr(),
                                     _ptr(maps['alpha'][0]), _ptr(maps['color'][0]))
        near = float(settings_list[0].near_plane) if near is None and k else float(near or 0.0)
        self._check(self.lib.fgs_tsdf_integrate(tsdf_weight.data_ptr(), _ptr(color), *dims, *[float(o) for o in origin], float(voxel_size), float(trunc),
                                                views, k, w, h, near, float(depth_max), float(min_alpha), float(max_weight), _stream_of(device)),
                    'fgs_tsdf_integrate')

    def tsdf_extract_mesh(self, tsdf_weight: torch.Tensor, color: Optional[torch.Tensor], origin: Sequence[float], voxel_size: float, iso: float = 0.0,
                          min_weight: float = 1.0) -> tuple:
        """(vertices [Nv,3] float32, faces [Nf,3] int32, colors [Nv,3] float32 or None) of the level set: count (one host synchronisation), allocate, emit."""
        device, dims = self._check_volume(tsdf_weight, color)
        scratch = _empty_bytes(self.lib.fgs_tsdf_mesh_scratch_bytes(*dims), device)
        counts = (C.c_int64 * 2)()
        stream = _stream_of(device)
        self._check(self.lib.fgs_tsdf_mesh_count(tsdf_weight.data_ptr(), *dims, float(iso), float(min_weight), scratch.data_ptr(), counts, stream),
                    'fgs_tsdf_mesh_count')
        nv, nf = int(counts[0]), int(counts[1])
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=device)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=device)
        colors = torch.empty((nv, 3), dtype=torch.float32, device=device) if color is not None else None
        self._check(self.lib.fgs_tsdf_mesh_emit(tsdf_weight.data_ptr(), _ptr(color), *dims, *[float(o) for o in origin], float(voxel_size), float(iso),
                                                float(min_weight), scratch.data_ptr(), nv, nf, _ptr(vertices), _ptr(colors), _ptr(faces), stream),
                    'fgs_tsdf_mesh_emit')
        return vertices, faces, colors

    # -- Gaussian-sharded multi-GPU path (include/fgs_hip.h, "Gaussian-sharded multi-GPU path") --------------------------------
    def _settings_array(self, views: Sequence[RasterizerSettings], total_sh_rest: int, device: torch.device, keep: list):
        arr = (_lib.Settings * len(views))()
        for i, v in enumerate(views):
            arr[i] = self._settings(v, total_sh_rest, device, keep)
        return arr

    def shard_preprocess(self, means, scales, rotations, opacities, sh0, sh_rest, views: Sequence[RasterizerSettings],
                         records: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
        """K1 over this rank's shard for all views of the step. `records`: uint8 [len(views), N, 56] (view v: the first
        counts[v, 0] records are filled), `counts`: int32 [len(views), 2] device tensor receiving (n_visible, n_instances).
        Returns the primitive buffer to hand to `shard_backward`."""
        device = self._check_params((means, scales, rotations, opacities, sh0, sh_rest), PARAMETER_NAMES)
        n, k = means.shape[0], len(views)
        if records.dtype != torch.uint8 or records.numel() < k * n * _lib.SPLAT_RECORD_BYTES or counts.dtype != torch.int32 \
                or counts.numel() < 2 * k or records.device != device or counts.device != device or not records.is_contiguous() \
                or not counts.is_contiguous():
            raise RuntimeError('records must be uint8 [views, N, 56] and counts int32 [views, 2] on the parameters\' device')
        keep: list = []
        S = self._settings_array(views, total_sh_rest(sh_rest), device, keep)
        buffers, cb = self._make_resizer(device, 4)
        self._check(self.lib.fgs_shard_preprocess(_ptr(means), _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh0), _ptr(sh_rest), n, k,
                                                  S, _ptr(records), counts.data_ptr(), cb, None, _stream_of(device)), 'fgs_shard_preprocess')
        return buffers[0]

    def forward_from_records(self, records: torch.Tensor, n_records: int, n_instances: int, settings: RasterizerSettings,
                             total_sh_rest: int, shard_counts: Sequence[int] | None = None) -> ForwardResult:
        """`shard_counts`: the records are the concatenation of that many records per shard; the renderer then places them interleaved (Morton
        neighbourhood of strided owners restored, include/fgs_hip.h). Pass the same counts to `backward_to_records`."""
        device = records.device
        if records.dtype != torch.uint8 or not records.is_contiguous() or records.numel() < n_records * _lib.SPLAT_RECORD_BYTES:
            raise RuntimeError('records must be a contiguous uint8 tensor of n_records * 56 bytes')
        S, keep, buffers, cb, st = self._forward_state(settings, total_sh_rest, device)
        image = torch.empty((3, settings.height, settings.width), dtype=torch.float32, device=device)
        counts, n_shards = _shard_counts(shard_counts)
        self._check(self.lib.fgs_forward_from_shard_records(_ptr(records), int(n_records), int(n_instances), counts, n_shards,
                                                            C.byref(S), image.data_ptr(), cb, None, C.byref(st), _stream_of(device)), 'fgs_forward_from_shard_records')
        return ForwardResult(image, tuple(buffers), _state_tuple(st))

    def backward_to_records(self, grad_image, image, buffers, settings: RasterizerSettings, state, total_sh_rest: int,
                            out: torch.Tensor | None = None, shard_counts: Sequence[int] | None = None, grad_alpha=None, grad_depth=None,
                            grad_feature_map=None, grad_distortion=None, grad_geometry=None) -> torch.Tensor:
        """K11 of a view rendered by `forward_from_records` -> float32 [n_records, 9] accumulator records."""
        if grad_alpha is not None or grad_depth is not None:
            raise RuntimeError('backward_to_records takes no alpha / depth gradients: the sharded and record paths render colour only')
        if grad_feature_map is not None:
            raise RuntimeError('backward_to_records takes no feature-map gradient: the sharded and record paths render colour only')
        if grad_distortion is not None:
            raise RuntimeError('backward_to_records takes no distortion gradient: the sharded and record paths render colour only')
        if grad_geometry is not None:
            raise RuntimeError('backward_to_records takes no geometry gradient: the sharded and record paths render colour only')
        device = image.device
        n = int(state[0])
        keep: list = []
        S = self._settings(settings, total_sh_rest, device, keep)
        grad_image = grad_image.to(dtype=torch.float32).contiguous()
        acc = out if out is not None else torch.empty((n, 9), dtype=torch.float32, device=device)
        if acc.dtype != torch.float32 or acc.numel() < 9 * n or not acc.is_contiguous() or acc.device != device:
            raise RuntimeError('accumulator records must be contiguous float32 [n_records, 9]')
        scratch = self._scratch(n, settings, device)
        st = _lib.ForwardState(*state)
        counts, n_shards = _shard_counts(shard_counts)
        self._check(self.lib.fgs_backward_to_shard_records(_ptr(grad_image), _ptr(image), _ptr(buffers[0]), _ptr(buffers[1]), _ptr(buffers[2]),
                                                           _ptr(buffers[3]), scratch.data_ptr(), _ptr(acc), n, counts, n_shards,
                                                           C.byref(S), C.byref(st), _stream_of(device)), 'fgs_backward_to_shard_records')
        return acc

    def shard_backward(self, acc_records: torch.Tensor, n_visible: Sequence[int], primitive_buffer: torch.Tensor, densification_info, means,
                       scales, rotations, opacities, sh_rest, views: Sequence[RasterizerSettings], out: tuple) -> tuple:
        """K12 on the shard, gradients summed over `views`; `acc_records`: float32 [sum(n_visible), 9] in view order;
        `out` = the six gradient tensors (means, scales, rotations, opacities, sh0, sh_rest), every element written."""
        device = self._check_params((means, scales, rotations, opacities, sh_rest) + tuple(out), BACKWARD_PARAMETER_NAMES + ('grad',) * 6)
        n, k = means.shape[0], len(views)
        total_rest = total_sh_rest(sh_rest)
        _gradients_out(out, gradient_shapes(n, total_rest), device, shapes_only=True)
        total = _check_acc_records(acc_records, n_visible, k, device)
        keep: list = []
        S = self._settings_array(views, total_rest, device, keep)
        dens = _densification(densification_info, n, device, validate=False)
        scratch = _empty_bytes(self.lib.fgs_shard_backward_scratch_bytes(n, k), device)
        counts = (C.c_int32 * k)(*[int(x) for x in n_visible])
        self._check(self.lib.fgs_shard_backward(_ptr(acc_records) if total > 0 else None, counts, _ptr(primitive_buffer), _ptr(means),
                                                _ptr(scales), _ptr(rotations), _ptr(opacities), _ptr(sh_rest), _ptr(out[0]), _ptr(out[1]),
                                                _ptr(out[2]), _ptr(out[3]), _ptr(out[4]), _ptr(out[5]), _ptr(dens), scratch.data_ptr(), n, k,
                                                S, _stream_of(device)), 'fgs_shard_backward')
        return out

    def shard_backward_adam_fused(self, acc_records: torch.Tensor, n_visible: Sequence[int], primitive_buffer: torch.Tensor, densification_info,
                                  params: Sequence[torch.Tensor], exp_avgs, exp_avg_sqs, views: Sequence[RasterizerSettings], step: int,
                                  lrs: Sequence[float], betas=(0.9, 0.999), eps: float = 1e-15) -> None:
        """`shard_backward` + Adam on the shard without materialising the gradients (<= 8 views). params / moments / lrs in
        optimizer-group order: means, sh0, sh_rest, opacities, scales, rotations."""
        device = self._check_params(tuple(params) + tuple(exp_avgs) + tuple(exp_avg_sqs), ['param/moment'] * 18)
        n, k = params[0].shape[0], len(views)
        total = _check_acc_records(acc_records, n_visible, k, device)
        keep: list = []
        S = self._settings_array(views, total_sh_rest(params[2]), device, keep)
        dens = _densification(densification_info, n, device, validate=False)
        scratch = _empty_bytes(self.lib.fgs_shard_backward_scratch_bytes(n, k), device)
        counts = (C.c_int32 * k)(*[int(x) for x in n_visible])
        self._check(self.lib.fgs_shard_backward_adam_fused(_ptr(acc_records) if total > 0 else None, counts, _ptr(primitive_buffer),
                                                           _pointer_array(params, 6), _pointer_array(exp_avgs, 6), _pointer_array(exp_avg_sqs, 6),
                                                           _ptr(dens), scratch.data_ptr(), n, k, S, int(step),
                                                           (C.c_double * 6)(*[float(x) for x in lrs]), float(betas[0]), float(betas[1]),
                                                           float(eps), _stream_of(device)), 'fgs_shard_backward_adam_fused')

    # -- the remaining exported operators (reference torch_bindings/filter3d.py, densification.py) ---------------------------
    def update_3d_filter(self, positions, w2c, filter_3d, visibility_mask, width, height, focal_x, focal_y, center_x, center_y,
                         near_plane, clipping_tolerance, distance2filter) -> None:
        device = self._check_params((positions, filter_3d), ('positions', 'filter_3d'))
        if visibility_mask.dtype != torch.bool or not visibility_mask.is_contiguous() or visibility_mask.device != device:
            raise RuntimeError('visibility_mask must be a contiguous bool tensor on the same device')
        w = w2c.to(device=device, dtype=torch.float32).contiguous()
        self._check(self.lib.fgs_update_3d_filter(_ptr(positions), w.data_ptr(), _ptr(filter_3d), _ptr(visibility_mask), positions.shape[0],
                                                  int(width), int(height), float(focal_x), float(focal_y), float(center_x), float(center_y),
                                                  float(near_plane), float(clipping_tolerance), float(distance2filter), _stream_of(device)),
                    'fgs_update_3d_filter')

    def relocation_adjustment(self, old_opacities, old_scales, n_samples_per_primitive):
        device = old_opacities.device
        op = old_opacities.to(torch.float32).contiguous()
        sc = old_scales.to(torch.float32).contiguous()
        ns = n_samples_per_primitive.to(device=device, dtype=torch.int64).contiguous()
        table = self._relocation_table.get(device)
        if table is None:
            host = (C.c_float * 2500)()
            self._check(self.lib.fgs_relocation_table(host), 'fgs_relocation_table')
            table = torch.tensor(list(host), dtype=torch.float32, device=device)
            self._relocation_table[device] = table
        n = op.shape[0]
        new_op = torch.empty((n, 1), dtype=torch.float32, device=device)
        new_sc = torch.empty((n, 3), dtype=torch.float32, device=device)
        self._check(self.lib.fgs_relocation_adjustment(_ptr(op), _ptr(sc), _ptr(ns), table.data_ptr(), _ptr(new_op), _ptr(new_sc), n,
                                                       _stream_of(device)), 'fgs_relocation_adjustment')
        return new_op, new_sc

    def add_noise(self, raw_scales, raw_rotations, raw_opacities, random_samples, means, current_lr: float) -> None:
        device = self._check_params((raw_scales, raw_rotations, raw_opacities, random_samples, means),
                                    ('raw_scales', 'raw_rotations', 'raw_opacities', 'random_samples', 'means'))
        self._check(self.lib.fgs_add_noise(_ptr(raw_scales), _ptr(raw_rotations), _ptr(raw_opacities), _ptr(random_samples), _ptr(means),
                                           means.shape[0], float(current_lr), _stream_of(device)), 'fgs_add_noise')

    # -- maintenance of the Gaussian set with the Adam moments (include/fgs_hip.h, "Next" row rank 1; Model.py:275-366, 459-463) -------
    def adaptive_density_control(self, densification_info, params: Sequence[torch.Tensor], exp_avgs, exp_avg_sqs, grad_threshold: float,
                                 min_opacity: float, prune_large_gaussians: bool, percent_dense: float, extent: float, noise_fn=None):
        """params (and optionally the two moment lists) in optimizer-group order: means, sh0, sh_rest, opacities, scales, rotations.
        Returns (new_params, new_exp_avgs or None, new_exp_avg_sqs or None, counts) with counts = (survivors, clones, children per
        copy, split). `noise_fn(n_rows)` supplies the [n_rows, 3] N(0,1) samples of the split (default torch.randn on the device)."""
        device = self._check_params(tuple(params) + (densification_info,), ['parameter'] * 6 + ['densification_info'])
        n = params[0].shape[0]
        total_rest = total_sh_rest(params[2])
        scratch = _empty_bytes(self.lib.fgs_adc_scratch_bytes(n), device)
        counts = (C.c_int32 * 4)()
        # the reference's thresholds (Model.py:315, 360, 363): formed in double from the Python scalars and rounded to float32 once, at the comparison
        if not (0.0 < min_opacity < 1.0) or not (percent_dense * extent > 0.0):
            raise RuntimeError('adaptive_density_control: min_opacity / percent_dense * extent out of range')
        log_small, log_large = math.log(percent_dense * extent), math.log(0.1 * extent)
        min_opacity_logit = math.log(min_opacity / (1 - min_opacity))
        self._check(self.lib.fgs_adc_plan_thresholds(_ptr(densification_info), _ptr(params[4]), _ptr(params[5]), _ptr(params[3]), n, float(grad_threshold),
                                                     min_opacity_logit, int(bool(prune_large_gaussians)), log_small, log_large,
                                                     scratch.data_ptr(), counts, _stream_of(device)), 'fgs_adc_plan_thresholds')
        kept, clones, children, split = (int(c) for c in counts)
        n_new = kept + clones + 2 * children
        noise = (noise_fn(2 * split) if noise_fn is not None else torch.randn((2 * split, 3), device=device)).to(device=device, dtype=torch.float32).contiguous()
        make = lambda t: torch.empty((n_new,) + tuple(t.shape[1:]), dtype=torch.float32, device=device)
        out_p = [make(t) for t in params]
        have_state = exp_avgs is not None
        if have_state:
            self._check_params(tuple(exp_avgs) + tuple(exp_avg_sqs), ['moment'] * 12)
        out_m = [make(t) for t in params] if have_state else None
        out_v = [make(t) for t in params] if have_state else None
        arr = lambda ts: _pointer_array(ts, 6) if ts is not None else None
        if n_new == 0:                     # everything pruned: nothing to write, and empty tensors have no address to hand over
            return out_p, out_m, out_v, (kept, clones, children, split)
        self._check(self.lib.fgs_adc_apply(arr(params), arr(exp_avgs), arr(exp_avg_sqs), arr(out_p), arr(out_m), arr(out_v), _ptr(noise),
                                           scratch.data_ptr(), n, total_rest, _stream_of(device)), 'fgs_adc_apply')
        return out_p, out_m, out_v, (kept, clones, children, split)

    def gather_rows(self, tensors: Sequence[torch.Tensor], index: torch.Tensor) -> list:
        """[t[index] for t in tensors] (float32, row-major) in one launch per 18 tensors: prune / sort of parameters and moments."""
        if not tensors:
            return []
        device = self._check_params(tuple(tensors), ['tensor'] * len(tensors))
        index = index.to(device=device, dtype=torch.int64).contiguous()
        rows = index.shape[0]
        outs = [torch.empty((rows,) + tuple(t.shape[1:]), dtype=torch.float32, device=device) for t in tensors]
        for first in range(0, len(tensors), 18):
            chunk, oc = tensors[first:first + 18], outs[first:first + 18]
            k = len(chunk)
            widths = [int(t.numel() // max(t.shape[0], 1)) if t.shape[0] > 0 else 0 for t in chunk]
            self._check(self.lib.fgs_gather_rows(k, _pointer_array(chunk, k), _pointer_array(oc, k),
                                                 (C.c_int32 * k)(*widths), _ptr(index), rows, _stream_of(device)), 'fgs_gather_rows')
        return outs

    def morton_order(self, means: torch.Tensor) -> torch.Tensor:
        """int64 permutation that sorts the points along a 30-bit Z-curve over their bounding box (Model.py:459-463), stable."""
        device = self._check_params((means,), ('means',))
        n = means.shape[0]
        order = torch.empty(n, dtype=torch.int64, device=device)
        if n == 0:
            return order
        lo, hi = means.min(dim=0).values.contiguous(), means.max(dim=0).values.contiguous()      # stay on the device: no host sync
        nbytes = int(self.lib.fgs_morton_order_temp_bytes(n))
        temp = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self._check(self.lib.fgs_morton_order(_ptr(means), lo.data_ptr(), hi.data_ptr(), order.data_ptr(), n, temp.data_ptr(), nbytes,
                                              _stream_of(device)), 'fgs_morton_order')
        return order

    def profile_enable(self, enable, only: str | None = None) -> None:
        """enable=True: HIP events around every stage; only='adam': around that one stage (far less intrusive); False: off."""
        if enable and only is not None:
            names = list(self.profile_read().keys())
            self._check(self.lib.fgs_profile_enable(2 + names.index(only)), 'fgs_profile_enable')
        else:
            self.lib.fgs_profile_enable(int(bool(enable)))

    def profile_read(self) -> dict:
        """{stage: (total_ms, calls)} accumulated since the last read (HIP events on the launch stream)."""
        arr = (_lib.StageTime * 32)()
        k = self.lib.fgs_profile_read(arr, 32)
        return {arr[i].name.decode(): (arr[i].total_ms, arr[i].calls) for i in range(max(k, 0))}

    # -- introspection (tests / bench only) ------------------------------------------------------------------------------
    def blob_layout(self, which: int, n: int, width: int, height: int, n_instances: int, n_buckets: int) -> dict:
        entries = (_lib.BlobEntry * 32)()
        k = self.lib.fgs_blob_layout(which, n, width, height, n_instances, n_buckets, entries, 32)
        if k < 0:
            raise RuntimeError(self.lib.fgs_last_error().decode())
        return {entries[i].name.decode(): (entries[i].offset, entries[i].bytes) for i in range(k)}

    def view(self, blob: torch.Tensor, layout: dict, name: str, dtype: torch.dtype) -> torch.Tensor:
        off, nbytes = layout[name]
        return blob[off:off + nbytes].view(dtype)


_DEFAULT: Backend | None = None


def default_backend() -> Backend:
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Backend(_lib.library())
    return _DEFAULT
