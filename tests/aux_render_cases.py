"""Scenes, reference arithmetic and comparisons shared by tests/test_aux_render.py (CPU simulation) and tests/test_gpu_aux_render.py (MI355X):
the per-pixel maps of fgs_inference_aux -- accumulated opacity, expected depth, median depth -- against references built from the oracle.

  alpha          : 1 - final_T of oracle.forward.
  expected depth : oracle.reblend with the colour (z, 1, 0) on a black background: channel 0 is sum_i w_i z_i in the oracle's own summation order,
                   channel 1 is sum_i w_i = 1 - final_T (cross-check). z = the float behind K1's depth key of the Gaussian.
  median depth   : reference_walk() below -- a per-tile fp32 walk in list order with the oracle's sub-tile cull and thresholds. It is trusted for the
                   median only after it has reproduced the oracle's final_T and n_processed on EVERY pixel (checked in reference()).

Bars (they hold on the simulation and on the device alike):
  alpha, expected depth : rel_inf < 1e-4 outside the flip pixels (helpers.flip_masks: a pair within 5e-6 of the alpha cut or a T within 1e-5 of the
                          termination test), which may be at most 0.1 % of the image;
  median depth          : |a - ref| <= 1e-6 |ref| outside the flip pixels and the pixels whose reference walk has a T_before within 1e-5 of 0.5
                          (there one ulp of exp picks the neighbour), at most 1 % of the image.
The scene seeds were chosen so that the reference side alone stays inside both caps (asserted, not assumed)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

import helpers
from harness.scenes import View, make_s0

ALPHA_DEPTH_TOL = 1e-4
MEDIAN_RTOL = 1e-6
HALF_BAND = 1e-5
MAX_EXCLUDED = 1e-3            # alpha / expected depth
MAX_EXCLUDED_MEDIAN = 1e-2

_libm = ctypes.CDLL('libm.so.6')
_libm.expf.restype, _libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
_expf = np.frompyfunc(lambda x: _libm.expf(float(x)), 1, 1)      # the oracle's own expf (numpy's float32 exp is another implementation)


def _logit(p):
    return torch.log(p) - torch.log1p(-p)


def stacked_scene(seed: int = 3):
    """128 x 96 (8 x 8 tiles). ~700 faint Gaussians (opacity 0.01 - 0.02) over one 32 x 24 px region in the middle: the lists of its tiles exceed three
    192-entry batches and are walked to their end (the fourth batch comes from the read-ahead registers, its indices from the stage before); T crosses 0.5
    some 70 entries in. Top left, three nearly opaque Gaussians stacked in front of twenty faint ones: early termination, median = the first Gaussian.
    An empty border all around: every map is 0 there."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    n_stack, n_front, n_behind = 700, 3, 20
    n = n_stack + n_front + n_behind
    means = torch.empty(n, 3)
    means[:n_stack] = (u(n_stack, 3) * 2.0 - 1.0) * torch.tensor([0.5, 0.35, 0.8])
    ray = lambda depth: torch.stack([-0.3 * depth, -0.2 * depth, depth - 4.0], dim=1)        # the camera sits at z = -4 and looks down +z
    means[n_stack:n_stack + n_front] = ray(torch.tensor([3.0, 3.3, 3.6])) + 0.01 * (u(n_front, 3) - 0.5)
    means[n_stack + n_front:] = ray(4.1 + 0.8 * u(n_behind)) + 0.2 * (u(n_behind, 3) - 0.5) * torch.tensor([1.0, 1.0, 0.0])
    scales = torch.log(torch.cat([0.2 + 0.1 * u(n_stack, 3), 0.08 + 0.02 * u(n_front, 3), 0.08 + 0.04 * u(n_behind, 3)]))
    opac = torch.cat([0.01 + 0.01 * u(n_stack, 1), 0.985 + 0.01 * u(n_front, 1), 0.05 + 0.1 * u(n_behind, 1)])
    rot = torch.randn(n, 4, generator=g)
    params = {'means': means.contiguous(), 'scales': scales.contiguous(), 'rotations': rot, 'opacities': _logit(opac),
              'sh_coefficients_0': 0.5 * torch.randn(n, 1, 3, generator=g), 'sh_coefficients_rest': 0.1 * torch.randn(n, 15, 3, generator=g)}
    w2c = torch.eye(4)
    w2c[2, 3] = 4.0
    return params, View(w2c, torch.tensor([0.0, 0.0, -4.0]), 128, 96, 128.0, 128.0, 64.0, 48.0, 0.2, 1.0e4, torch.zeros(3))


def partial_tiles_scene(seed: int = 4):
    """70 x 50: 4 full tiles + 6 px across, 4 full tiles + 2 px down -- live tiles with pixels outside the image on both axes."""
    p, v = make_s0(seed=seed, n=400)
    return p, View(v.w2c, v.position, 70, 50, 150.0, 150.0, 35.0, 25.0, 0.2, 1.0e4, torch.zeros(3))


SCENES = {'s0': lambda: make_s0(n=1000), 'partial_tiles': partial_tiles_scene, 'stacked': stacked_scene}


def reference_walk(f: dict, z: np.ndarray, width: int, height: int) -> dict:
    """K10's per-pixel walk restated per tile in numpy, fp32, in list order (fgs_oracle.c: orc_blend_forward): sub-tile bounding-box cull, alpha >= 1/255,
    stop once T < 1e-4. Returns final_T, n_processed, the median depth (z of the last blended Gaussian met with T > 0.5) and `near_half`: pixels where a
    blended Gaussian met a T within HALF_BAND of 0.5."""
    f32 = np.float32
    gw, gh = (width + 15) // 16, (height + 11) // 12
    final_T, n_proc = np.ones((height, width), f32), np.zeros((height, width), np.uint32)
    median, near_half = np.zeros((height, width), f32), np.zeros((height, width), bool)
    mean2d, conic, bounds = f['mean2d'], f['conic_opacity'], f['screen_bounds'].astype(np.int64)
    for tile in range(gw * gh):
        r0, r1 = (int(x) for x in f['ranges'][tile])
        ty, tx = divmod(tile, gw)
        lx, ly = np.tile(np.arange(16), 12), np.repeat(np.arange(12), 16)
        px, py = tx * 16 + lx, ty * 12 + ly
        inside = (px < width) & (py < height)
        sx0, sy0 = tx * 16 + (lx // 8) * 8, ty * 12 + (ly // 4) * 4
        pxf, pyf = px.astype(f32) + f32(0.5), py.astype(f32) + f32(0.5)
        T, used, med, near, done = np.ones(192, f32), np.zeros(192, np.uint32), np.zeros(192, f32), np.zeros(192, bool), ~inside
        for j in range(r1 - r0):
            if done.all():
                break
            p = int(f['inst_prims'][r0 + j])
            sb = bounds[p]
            idx = np.nonzero(~done & (sb[0] < sx0 + 8) & (sx0 < sb[1]) & (sb[2] < sy0 + 4) & (sy0 < sb[3]))[0]
            if not idx.size:
                continue
            co = conic[p]
            dx, dy = mean2d[p, 0] - pxf[idx], mean2d[p, 1] - pyf[idx]
            expo = f32(-0.5) * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy
            alpha = co[3] * _expf(np.minimum(expo, f32(0.0))).astype(f32)
            blend = alpha >= f32(1.0) / f32(255.0)
            idx, alpha = idx[blend], alpha[blend]
            before = T[idx]
            near[idx] |= np.abs(before.astype(np.float64) - 0.5) <= HALF_BAND
            med[idx] = np.where(before > f32(0.5), z[p], med[idx])
            T[idx] = before * (f32(1.0) - alpha)
            used[idx] = j + 1
            done[idx] |= T[idx] < f32(1e-4)
        ys, xs = py[inside], px[inside]
        final_T[ys, xs], n_proc[ys, xs], median[ys, xs], near_half[ys, xs] = T[inside], used[inside], med[inside], near[inside]
    return {'final_T': final_T, 'n_processed': n_proc, 'median': median, 'near_half': near_half}


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """Scene `name` and its reference maps, computed once per process and shared (treat as read-only)."""
    from oracle import oracle as O
    O.build()
    params, view = SCENES[name]()
    assert float(view.background_color.abs().max()) == 0.0             # channel 0 of the re-blend is sum w z only on black
    S, _ = helpers.settings_pair(view)
    f = O.forward(*helpers.np_params(params), S, bucket_size=64)
    H, W, N = view.height, view.width, f['N']
    z = np.zeros(N, np.float32)
    z[f['prim_idx_unsorted']] = f['depth_keys_unsorted'].view(np.float32)
    colour = np.stack([z, np.ones(N, np.float32), np.zeros(N, np.float32)], axis=1)
    f2 = O.reblend(f, S, f['mean2d'], f['conic_opacity'], colour)
    alpha = (np.float32(1.0) - f['final_T']).reshape(H, W)
    assert np.array_equal(f2['final_T'], f['final_T']) and np.array_equal(f2['n_processed'], f['n_processed'])
    assert np.abs(f2['image'][1] - alpha).max() < 1e-5                                     # sum of the weights = accumulated opacity
    walk = reference_walk(f, z, W, H)
    assert np.array_equal(walk['final_T'].reshape(-1), f['final_T']), 'the numpy walk must reproduce the final transmittance of every pixel'
    assert np.array_equal(walk['n_processed'].reshape(-1), f['n_processed']), 'the numpy walk must reproduce the last contributor of every pixel'
    flips = helpers.flip_masks(O, f, S)['pixel']
    excluded_median = flips | walk['near_half']
    assert float(flips.mean()) <= MAX_EXCLUDED, (name, 'flip pixels', float(flips.mean()))
    assert float(excluded_median.mean()) <= MAX_EXCLUDED_MEDIAN, (name, 'pixels excluded from the median', float(excluded_median.mean()))
    return {'params': params, 'view': view, 'f': f, 'z': z, 'alpha': alpha, 'depth': f2['image'][0].copy(), 'median': walk['median'],
            'n_processed': f['n_processed'].reshape(H, W), 'keep': ~flips, 'keep_median': ~excluded_median}


def render(be, ref: dict, device='cpu', to_chw=True, clamp=True, alpha=True, depth_expected=True, depth_median=True, bg=None) -> dict:
    _, RS = helpers.settings_pair(ref['view'], bg=bg, device=device)
    out = be.inference_aux(*[ref['params'][k].to(device) for k in helpers.NAMES], RS, to_chw, clamp, alpha, depth_expected, depth_median)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_maps(out: dict, ref: dict, label: str = '') -> dict:
    """The three maps of one fgs_inference_aux run against the references; every figure is printed before it is held to its bar."""
    keep, keep_m = ref['keep'], ref['keep_median']
    report = {'excluded': float((~keep).mean()), 'excluded_median': float((~keep_m).mean())}
    report['alpha'] = helpers.rel_inf(out['alpha'][keep], ref['alpha'][keep])
    report['depth'] = helpers.rel_inf(out['depth'][keep], ref['depth'][keep])
    a, r = out['depth_median'][keep_m].astype(np.float64), ref['median'][keep_m].astype(np.float64)
    report['median_worst_rel'] = float((np.abs(a - r)[r != 0] / np.abs(r[r != 0])).max()) if (r != 0).any() else 0.0
    report['median_mismatches'] = int((np.abs(a - r) > MEDIAN_RTOL * np.abs(r)).sum())
    print(label, report)
    assert report['excluded'] <= MAX_EXCLUDED and report['excluded_median'] <= MAX_EXCLUDED_MEDIAN, (label, report)
    assert report['alpha'] < ALPHA_DEPTH_TOL, (label, 'alpha', report)
    assert report['depth'] < ALPHA_DEPTH_TOL, (label, 'expected depth', report)
    assert report['median_mismatches'] == 0, (label, 'median depth', report)
    nothing = ref['n_processed'] == 0                       # nothing was blended: all three maps are exactly 0, whatever the masks say
    assert not out['alpha'][nothing].any() and not out['depth'][nothing].any() and not out['depth_median'][nothing].any(), label
    return report
