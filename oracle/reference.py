"""ctypes front end of the reference's own rasterizer run on the CPU (oracle/build_ref.py -> oracle/_ref/libfgs_ref_cpu.so).  TEST INFRASTRUCTURE ONLY.

forward / backward / inference / pruning_scores / relocation_adjustment / add_noise call the reference's host functions through oracle/ref_driver.cpp
and return what they computed under the keys of oracle.forward / oracle.backward, so a test compares the two dictionaries field by field. The
intermediates are decoded from the reference's four byte blobs through the offsets its own from_blob layouts give (ref_layout in the driver).

Fields the reference leaves undefined are returned as it left them (the driver fills fresh blobs with 0xA5): per-Gaussian records of Gaussians with
n_touched == 0, and bucket checkpoints of pixels that were done when the bucket began (`ckpt_written` tells which are defined).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import build_ref
from .oracle import BLOCK_BLEND, Settings, _f32, _p, grid_of

_LIB = None


def available() -> bool:
    """A library exists or can be built (a reference tree is present)."""
    return build_ref.LIB.exists() or build_ref.reference_tree() is not None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        path = build_ref.build()
        if path is None:
            raise RuntimeError('no reference tree and no oracle/_ref/libfgs_ref_cpu.so')
        _LIB = C.CDLL(str(path))
        _LIB.ref_blob.restype = C.c_void_p
        _LIB.ref_extract_end_bit.restype = C.c_int
    return _LIB


def _blob(which: int) -> np.ndarray:
    size = C.c_size_t(0)
    ptr = lib().ref_blob(which, C.byref(size))
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(size.value, 1),))[:size.value].copy() if ptr else np.zeros(0, np.uint8)


def _take(blob: np.ndarray, offset: int, dtype, count: int) -> np.ndarray:
    nbytes = np.dtype(dtype).itemsize * count
    assert offset + nbytes <= blob.size, (offset, nbytes, blob.size)
    return blob[offset:offset + nbytes].view(dtype).copy()


def _inputs(means, scales, rotations, opacities, sh0, sh_rest):
    means, scales, rotations = _f32(means).reshape(-1, 3), _f32(scales).reshape(-1, 3), _f32(rotations).reshape(-1, 4)
    opacities, sh0 = _f32(opacities).reshape(-1), _f32(sh0).reshape(-1, 3)
    N = means.shape[0]
    sh_rest = _f32(sh_rest)
    total_rest = sh_rest.shape[1] if sh_rest.ndim == 3 else (sh_rest.size // (3 * N) if N else 0)
    return (means, scales, rotations, opacities, sh0, sh_rest.reshape(N, total_rest, 3)), N, total_rest


def _view_args(s: Settings):
    w2c = np.ascontiguousarray(np.asarray(s.w2c, np.float32).reshape(-1)[:12])
    cam = np.ascontiguousarray(np.asarray(s.cam_position, np.float32).reshape(3))
    bg = np.ascontiguousarray(np.asarray(s.bg_color, np.float32).reshape(3))
    return w2c, cam, bg


def _scalars(s: Settings, planes: bool = True):
    out = [C.c_float(s.focal_x), C.c_float(s.focal_y), C.c_float(s.center_x), C.c_float(s.center_y)]
    if planes:
        out += [C.c_float(s.near_plane), C.c_float(s.far_plane)]
    return out + [int(bool(s.proper_antialiasing))]


def _decode(N: int, W: int, H: int, I: int | None, B: int | None, selector: int | None) -> dict:
    """The intermediates of the latest call. B None: a pass without buckets (inference, pruning scores); selector None: take the half CUB's sort
    leaves current (the stand-in flips once per 8-bit pass)."""
    L = lib()
    gw, gh, T = grid_of(W, H)
    end_bit = int(L.ref_extract_end_bit(C.c_uint(T - 1)))
    po, to, io, bo = (C.c_size_t * 13)(), (C.c_size_t * 7)(), (C.c_size_t * 5)(), (C.c_size_t * 3)()
    pb, tb, ib = _blob(0), _blob(1), _blob(2)
    if I is None:          # a pass that returns no counts: the primitive layout does not depend on them
        L.ref_layout(N, T, 0, 0, end_bit, po, to, io, bo)
        I = int(_take(pb, po[11], np.uint32, 1)[0])
    L.ref_layout(N, T, I, B or 0, end_bit, po, to, io, bo)
    assert pb.size == po[12] and tb.size == to[6] and ib.size == io[4], 'blob sizes differ from required<>()'
    V = int(_take(pb, po[10], np.uint32, 1)[0])
    assert int(_take(pb, po[11], np.uint32, 1)[0]) == I
    out = {'N': N, 'grid': (gw, gh), 'T': T, 'end_bit': end_bit, 'bucket_size': 32, 'V': V, 'I': I}
    depth_sel = 0          # 32 key bits: four passes, back in the first half
    out['depth_keys'] = _take(pb, po[0 + depth_sel], np.uint32, N)[:V]
    out['prim_idx'] = _take(pb, po[2 + depth_sel], np.uint32, N)[:V]
    out['n_touched'] = _take(pb, po[4], np.uint32, N)
    out['offsets'] = _take(pb, po[5], np.uint32, N)[:V]
    out['screen_bounds'] = _take(pb, po[6], np.uint16, 4 * N).reshape(N, 4)
    out['mean2d'] = _take(pb, po[7], np.float32, 2 * N).reshape(N, 2)
    out['conic_opacity'] = _take(pb, po[8], np.float32, 4 * N).reshape(N, 4)
    out['color'] = _take(pb, po[9], np.float32, 3 * N).reshape(N, 3)
    key_t = np.uint16 if end_bit <= 16 else np.uint32
    sel = ((end_bit + 7) // 8) & 1 if selector is None else selector
    out['selector'] = sel
    out['inst_keys'] = _take(ib, io[0 + sel], key_t, I).astype(np.uint32)
    out['inst_prims'] = _take(ib, io[2 + sel], np.uint32, I)
    out['ranges'] = _take(tb, to[0], np.uint32, 2 * T).reshape(T, 2)
    out['n_buckets'] = _take(tb, to[2], np.uint32, T)
    out['bucket_offsets'] = _take(tb, to[3], np.uint32, T)
    if B is None:
        # the inference / pruning-scores preprocess does not zero n_touched first (the training one does): rows outside the visible list are
        # whatever the blob held. Returned as 0, which is what a reader of the list can know about them.
        listed = np.zeros(N, bool)
        listed[out['prim_idx']] = True
        out['n_touched'] = np.where(listed, out['n_touched'], 0).astype(np.uint32)
        return out
    P = W * H
    bb = _blob(3)
    assert bb.size == bo[2]
    out['B'] = B
    out['final_T'] = _take(tb, to[1], np.float32, T * BLOCK_BLEND)[:P]            # indexed by pixel, width * y + x
    out['max_n_processed'] = _take(tb, to[4], np.uint32, T)
    out['n_processed'] = _take(tb, to[5], np.uint32, T * BLOCK_BLEND)[:P]
    out['bucket_tile_index'] = _take(bb, bo[0], np.uint32, B)
    out['bucket_ckpt'] = _take(bb, bo[1], np.float32, B * BLOCK_BLEND * 4).reshape(B, BLOCK_BLEND, 4)
    # a pixel stores its checkpoint at the start of every 32-entry chunk it is not yet done at: pixels inside the image, until the entry that
    # brought their transmittance under 1e-4 (n_processed names it; a pixel that never terminated has final_T >= 1e-4)
    written = np.zeros((B, BLOCK_BLEND), bool)
    if B:
        tile = out['bucket_tile_index'].astype(np.int64)
        first = np.where(tile == 0, 0, out['bucket_offsets'][np.maximum(tile - 1, 0)]).astype(np.int64)
        k = np.arange(B) - first
        local = np.arange(BLOCK_BLEND)
        px = (tile % gw)[:, None] * 16 + local[None, :] % 16
        py = (tile // gw)[:, None] * 12 + local[None, :] // 16
        inside = (px < W) & (py < H)
        pix = np.where(inside, py * W + px, 0)
        terminated = out['final_T'][pix] < np.float32(1e-4)
        written = inside & (~terminated | (k[:, None] * 32 < out['n_processed'][pix]))
    # ... and that rule names exactly the written set: every other entry still holds the fill the driver gave the fresh blob
    raw = out['bucket_ckpt'].view(np.uint32)
    assert np.all(raw[~written] == 0xA5A5A5A5) and not np.any(np.all(raw[written] == 0xA5A5A5A5, axis=-1)), 'ckpt_written is not the set of stored checkpoints'
    out['ckpt_written'] = written
    return out


def forward(means, scales, rotations, opacities, sh0, sh_rest, settings: Settings) -> dict:
    """faster_gs::rasterization::forward as forward_wrapper calls it; every intermediate under oracle.forward's keys (bucket size 32)."""
    L = lib()
    a, N, total_rest = _inputs(means, scales, rotations, opacities, sh0, sh_rest)
    w2c, cam, bg = _view_args(settings)
    W, H = settings.width, settings.height
    image = np.zeros((3, H, W), np.float32)
    out3 = (C.c_int * 3)()
    L.ref_forward(*[_p(x) for x in a], _p(w2c), _p(cam), _p(bg), _p(image), N, int(settings.active_sh_bases), total_rest, W, H, *_scalars(settings), out3)
    out = _decode(N, W, H, int(out3[0]), int(out3[1]), int(out3[2]))
    out.update(image=image, _inputs=a, _state=tuple(int(v) for v in out3), _view=(w2c, cam, bg), _total_rest=total_rest)
    return out


def backward(fwd: dict, settings: Settings, grad_image, densification_info: np.ndarray | None = None) -> dict:
    """faster_gs::rasterization::backward as backward_wrapper calls it, on the blobs of the forward that returned `fwd` -- which must be the latest
    forward call. Zero-filled gradients and helpers, as the wrapper's torch::zeros."""
    L = lib()
    means, scales, rotations, opacities, sh0, sh_rest = fwd['_inputs']
    N, total_rest = fwd['N'], fwd['_total_rest']
    w2c, cam, bg = fwd['_view']
    W, H = settings.width, settings.height
    grad_image = np.ascontiguousarray(_f32(grad_image).reshape(3, H, W))
    g = {'means': np.zeros((N, 3), np.float32), 'scales': np.zeros((N, 3), np.float32), 'rotations': np.zeros((N, 4), np.float32),
         'opacities': np.zeros((N, 1), np.float32), 'sh0': np.zeros((N, 1, 3), np.float32), 'sh_rest': np.zeros((N, total_rest, 3), np.float32)}
    grad_mean2d, grad_conic = np.zeros((N, 2), np.float32), np.zeros((3, N), np.float32)
    dens = None
    if densification_info is not None and densification_info.size > 0:
        assert densification_info.dtype == np.float32 and densification_info.flags['C_CONTIGUOUS']
        dens = _p(densification_info)
    n_inst, n_buckets, selector = fwd['_state']
    L.ref_backward(_p(grad_image), _p(fwd['image']), _p(means), _p(scales), _p(rotations), _p(opacities), _p(sh_rest), _p(w2c), _p(cam), _p(bg),
                   _p(g['means']), _p(g['scales']), _p(g['rotations']), _p(g['opacities']), _p(g['sh0']), _p(g['sh_rest']), _p(grad_mean2d), _p(grad_conic),
                   dens, N, n_inst, n_buckets, selector, int(settings.active_sh_bases), total_rest, W, H, *_scalars(settings, planes=False))
    g['_grad_mean2d'], g['_grad_conic'] = grad_mean2d, grad_conic
    return g


def inference(means, scales, rotations, opacities, sh0, sh_rest, settings: Settings, to_chw: bool = True, clamp_output: bool = True) -> dict:
    L = lib()
    a, N, total_rest = _inputs(means, scales, rotations, opacities, sh0, sh_rest)
    w2c, cam, bg = _view_args(settings)
    W, H = settings.width, settings.height
    image = np.zeros((3, H, W) if to_chw else (H, W, 3), np.float32)
    L.ref_inference(*[_p(x) for x in a], _p(w2c), _p(cam), _p(bg), _p(image), N, int(settings.active_sh_bases), total_rest, W, H, *_scalars(settings),
                    int(to_chw), int(clamp_output))
    out = _decode(N, W, H, None, None, None)
    out['image'] = image
    return out


def pruning_scores(scores: np.ndarray, means, scales, rotations, opacities, sh0, sh_rest, settings: Settings) -> dict:
    """faster_gs::rasterization::pruning_scores: accumulates into `scores` [N] in place."""
    assert scores.dtype == np.float32 and scores.flags['C_CONTIGUOUS']
    L = lib()
    a, N, total_rest = _inputs(means, scales, rotations, opacities, sh0, sh_rest)
    w2c, cam, bg = _view_args(settings)
    W, H = settings.width, settings.height
    L.ref_pruning_scores(_p(scores), *[_p(x) for x in a], _p(w2c), _p(cam), _p(bg), N, int(settings.active_sh_bases), total_rest, W, H, *_scalars(settings))
    return _decode(N, W, H, None, None, None)


def relocation_adjustment(old_opacities, old_scales, n_samples_per_primitive):
    op, sc = np.ascontiguousarray(_f32(old_opacities).reshape(-1)), np.ascontiguousarray(_f32(old_scales).reshape(-1, 3))
    ns = np.ascontiguousarray(np.asarray(n_samples_per_primitive).astype(np.int64).reshape(-1))
    new_op, new_sc = np.zeros_like(op), np.zeros_like(sc)
    lib().ref_relocation_adjustment(_p(op), _p(sc), _p(ns), _p(new_op), _p(new_sc), op.shape[0])
    return new_op.reshape(-1, 1), new_sc


def add_noise(raw_scales, raw_rotations, raw_opacities, random_samples, means, current_lr) -> None:
    """`means` [N,3] float32 is updated in place."""
    assert means.dtype == np.float32 and means.flags['C_CONTIGUOUS']
    s, q = np.ascontiguousarray(_f32(raw_scales).reshape(-1, 3)), np.ascontiguousarray(_f32(raw_rotations).reshape(-1, 4))
    o, r = np.ascontiguousarray(_f32(raw_opacities).reshape(-1)), np.ascontiguousarray(_f32(random_samples).reshape(-1, 3))
    lib().ref_add_noise(_p(s), _p(q), _p(o), _p(r), _p(means), means.shape[0], C.c_float(current_lr))


def dump_scene(path, means, scales, rotations, opacities, sh0, sh_rest, settings: Settings, grad_image) -> None:
    """The input file of the driver's stand-alone main (oracle/build_ref.py: build_sanitized_program)."""
    a, N, total_rest = _inputs(means, scales, rotations, opacities, sh0, sh_rest)
    w2c, cam, bg = _view_args(settings)
    W, H = settings.width, settings.height
    with open(path, 'wb') as fh:
        fh.write(np.array([N, total_rest, W, H, int(settings.active_sh_bases), int(bool(settings.proper_antialiasing))], np.int32).tobytes())
        fh.write(np.array([settings.focal_x, settings.focal_y, settings.center_x, settings.center_y, settings.near_plane, settings.far_plane], np.float32).tobytes())
        for x in (*a, w2c, cam, bg, _f32(grad_image).reshape(3, H, W)):
            fh.write(np.ascontiguousarray(x, np.float32).tobytes())
