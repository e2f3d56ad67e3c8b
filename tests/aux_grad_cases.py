"""Scenes, fp64 reference and comparisons shared by tests/test_aux_grad.py (CPU simulation) and tests/test_gpu_aux_grad.py (MI355X): the training render
that returns accumulated opacity A = 1 - T_final and expected depth D = sum_i w_i z_i differentiably (fgs_forward_aux / fgs_backward_aux,
diff_rasterize_aux).

Reference: aux_autograd_reference() -- the fp64 torch.autograd restatement of the image formation model of oracle/torch_check.py: autograd_reference
(discrete structure from oracle.forward(..., bucket_size=64), everything differentiable recomputed in double) with two more outputs of the same
compositing weights, A = sum_i w_i and D = sum_i w_i z_i, z_i = row 2 of w2c applied to the mean. With gA = gD = 0 it must give autograd_reference's
gradients (asserted in test_aux_grad.py), which pins it to the reference the project already trusts.

Upstream gradients: seeded random gC [3,H,W], gA, gD [H,W], set to ZERO on the reference's flip pixels (helpers.flip_masks(...)['pixel']): a pair
blended by one side and skipped by the other only affects its own pixel, so zeroing the pixel removes the flip from both sides. At most 0.1 % of a
scene's pixels may be zeroed (asserted per scene; the seeds were chosen so that the reference alone stays inside it).

Bars: forward maps -- aux_render_cases.check_maps' alpha / depth bar (1e-4 rel_inf outside the flip pixels); image -- diff_rasterize's (bit-identical on
the simulation, 1e-4 on the device: equal-depth compaction order is the only licence); each of the six gradient tensors -- helpers.rel_inf < 1e-4
against the fp64 reference, the project's bar, with the plain RGB path's figure on the same scene and gC printed next to it."""
from __future__ import annotations

import functools

import numpy as np
import torch

import aux_render_cases as render_cases
import helpers
from harness.scenes import View, make_s0
from oracle.torch_check import _sh_color

GRAD_TOL = 1e-4
MAP_TOL = render_cases.ALPHA_DEPTH_TOL
MAX_ZEROED = 1e-3
HOT_FOOTPRINT = 256                     # csrc/fgs_config.h: kHotFootprint (candidate tiles)


def hot_scene(seed: int = 7):
    """120 large Gaussians at 336 x 252 (21 x 21 tiles): several have boxes of more than 256 candidate tiles -- K11 adds their sums into the 16 replicas of
    their hot slot, and dL/dz into the replicas of acc_z -- in front of and behind ordinary ones. Small enough for the dense fp64 reference."""
    p, v = make_s0(seed=seed, n=120)
    p['scales'] = p['scales'] + 2.2
    p['opacities'] = p['opacities'] - 2.0
    return p, View(v.w2c, v.position, 336, 252, 300.0, 300.0, 168.0, 126.0, 0.2, 1e4, torch.zeros(3))


# name -> (scene, active_sh_bases, proper_antialiasing)
CASES = {
    's0': (render_cases.SCENES['s0'], 16, False),
    'partial_tiles': (render_cases.SCENES['partial_tiles'], 16, True),         # the proper-antialiasing case
    'stacked': (render_cases.SCENES['stacked'], 1, False),                     # the active_sh_bases = 1 case
    'hot': (hot_scene, 16, False),
}


def aux_autograd_reference(params: dict, S, fwd: dict, gC, gA, gD) -> dict:
    """fp64 image, A, D and the six gradients of sum(gC image) + sum(gA A) + sum(gD D). `params`: numpy arrays named as in oracle.forward
    (means, scales, rotations, opacities, sh0, sh_rest); `S` an oracle.Settings; `fwd` = oracle.forward(..., bucket_size=64)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    P = {k: t(v).requires_grad_(True) for k, v in params.items()}
    means, scales, rots, opac = P['means'], P['scales'], P['rotations'], P['opacities'].reshape(-1)
    N = means.shape[0]
    sh0, sh_rest = P['sh0'].reshape(-1, 1, 3), P['sh_rest'].reshape(N, -1, 3)
    W, H = S.width, S.height
    w2c, cam, bg = t(S.w2c)[:3, :4], t(S.cam_position).reshape(1, 3), t(S.bg_color).reshape(3)

    order = torch.tensor(fwd['prim_idx'].astype(np.int64))
    V = order.numel()
    m = means[order]
    cam_pts = m @ w2c[:, :3].T + w2c[:, 3]
    depth = cam_pts[:, 2]
    x, y = cam_pts[:, 0] / depth, cam_pts[:, 1] / depth
    q = rots[order]
    qn = q / q.norm(dim=1, keepdim=True)
    r, qx, qy, qz = qn[:, 0], qn[:, 1], qn[:, 2], qn[:, 3]
    R = torch.stack([
        1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r * qz), 2 * (qx * qz + r * qy),
        2 * (qx * qy + r * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r * qx),
        2 * (qx * qz - r * qy), 2 * (qy * qz + r * qx), 1 - 2 * (qx * qx + qy * qy)], dim=1).reshape(V, 3, 3)
    cov3d = R @ torch.diag_embed(torch.exp(2.0 * scales[order])) @ R.transpose(1, 2)
    clip_l, clip_r = (-0.15 * W - S.center_x) / S.focal_x, (1.15 * W - S.center_x) / S.focal_x
    clip_t, clip_b = (-0.15 * H - S.center_y) / S.focal_y, (1.15 * H - S.center_y) / S.focal_y
    xc, yc = x.clamp(clip_l, clip_r), y.clamp(clip_t, clip_b)
    j11, j22 = S.focal_x / depth, S.focal_y / depth
    zero = torch.zeros_like(depth)
    J = torch.stack([j11, zero, -j11 * xc, zero, j22, -j22 * yc], dim=1).reshape(V, 2, 3)
    JW = J @ w2c[:, :3]
    cov2d = JW @ cov3d @ JW.transpose(1, 2)
    ks = 0.1 if S.proper_antialiasing else 0.3
    a_raw, b, c_raw = cov2d[:, 0, 0], cov2d[:, 0, 1], cov2d[:, 1, 1]
    a, c = a_raw + ks, c_raw + ks
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], dim=1)
    opacity = torch.sigmoid(opac[order])
    if S.proper_antialiasing:
        opacity = opacity * torch.sqrt(((a_raw * c_raw - b * b) / det).clamp_min(0.0)).detach()
    mean2d = torch.stack([x * S.focal_x + S.center_x, y * S.focal_y + S.center_y], dim=1)
    color = _sh_color(sh0[order], sh_rest[order], m, cam, S.active_sh_bases).clamp_min(0.0)

    gw, gh = fwd['grid']
    rank = torch.full((N,), -1, dtype=torch.int64)
    rank[order] = torch.arange(V)
    member = torch.zeros((gw * gh, V), dtype=torch.bool)
    member[torch.tensor(fwd['inst_keys'].astype(np.int64)), rank[torch.tensor(fwd['inst_prims'].astype(np.int64))]] = True
    sb = torch.tensor(fwd['screen_bounds'].astype(np.int64))[order]
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    tile = (ys // 12) * gw + (xs // 16)
    sx0, sy0 = (xs // 8) * 8, (ys // 4) * 4
    overlap = (sb[None, :, 0] < (sx0 + 8)[:, None]) & (sx0[:, None] < sb[None, :, 1]) \
        & (sb[None, :, 2] < (sy0 + 4)[:, None]) & (sy0[:, None] < sb[None, :, 3])
    dx = mean2d[None, :, 0] - (xs.double() + 0.5)[:, None]
    dy = mean2d[None, :, 1] - (ys.double() + 0.5)[:, None]
    expo = -0.5 * (conic[None, :, 0] * dx * dx + conic[None, :, 2] * dy * dy) - conic[None, :, 1] * dx * dy
    alpha = opacity[None, :] * torch.exp(expo.clamp_max(0.0))
    use = member[tile] & overlap & (alpha >= 1.0 / 255.0)
    alpha = torch.where(use, alpha, torch.zeros_like(alpha))
    T_after = torch.cumprod(1.0 - alpha, dim=1)
    T_before = torch.cat([torch.ones_like(T_after[:, :1]), T_after[:, :-1]], dim=1)
    alpha = torch.where((T_before >= 1e-4).detach(), alpha, torch.zeros_like(alpha))
    T_after = torch.cumprod(1.0 - alpha, dim=1)
    T_before = torch.cat([torch.ones_like(T_after[:, :1]), T_after[:, :-1]], dim=1)
    w = T_before * alpha
    image = (w @ color + T_after[:, -1:] * bg[None, :]).T.reshape(3, H, W)
    A = w.sum(dim=1).reshape(H, W)                        # = 1 - T_final; the background is no part of it
    D = (w @ depth).reshape(H, W)
    loss = (image * t(gC).reshape(3, H, W)).sum() + (A * t(gA).reshape(H, W)).sum() + (D * t(gD).reshape(H, W)).sum()
    loss.backward()
    out = {'image': image.detach().numpy(), 'alpha': A.detach().numpy(), 'depth': D.detach().numpy()}
    for k, v in P.items():
        out[k] = v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))
    return out


def named_params(params: dict) -> dict:
    a = helpers.np_params(params)
    return dict(means=a[0], scales=a[1], rotations=a[2], opacities=a[3], sh0=a[4], sh_rest=a[5])


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """Scene, settings, oracle forward pass, flip mask and the seeded upstream gradients (zero on the flip pixels) of case `name`: once per process."""
    from oracle import oracle as O
    O.build()
    make, K, aa = CASES[name]
    params, view = make()
    S, _ = helpers.settings_pair(view, K, aa)
    f = O.forward(*helpers.np_params(params), S, bucket_size=64)
    H, W = view.height, view.width
    flips = helpers.flip_masks(O, f, S)['pixel']
    assert float(flips.mean()) <= MAX_ZEROED, (name, 'zeroed pixels', float(flips.mean()))
    rng = np.random.default_rng(11)
    gC = (rng.standard_normal((3, H, W)) / (3 * H * W)).astype(np.float32)
    gA = (rng.standard_normal((H, W)) / (H * W)).astype(np.float32)
    gD = (rng.standard_normal((H, W)) / (H * W)).astype(np.float32)
    gC[:, flips] = 0.0
    gA[flips] = 0.0
    gD[flips] = 0.0
    return {'name': name, 'params': params, 'view': view, 'K': K, 'aa': aa, 'S': S, 'f': f, 'keep': ~flips, 'gC': gC, 'gA': gA, 'gD': gD}


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """The fp64 reference of case `name` for its (gC, gA, gD): once per process, shared, read-only."""
    c = case(name)
    return aux_autograd_reference(named_params(c['params']), c['S'], c['f'], c['gC'], c['gA'], c['gD'])


@functools.lru_cache(maxsize=None)
def reference_rgb(name: str) -> dict:
    """... and for gC alone: what the plain RGB path is compared with (the figure printed beside the depth path's)."""
    c = case(name)
    return aux_autograd_reference(named_params(c['params']), c['S'], c['f'], c['gC'], 0.0 * c['gA'], 0.0 * c['gD'])


def settings_of(c: dict, device='cpu'):
    return helpers.settings_pair(c['view'], c['K'], c['aa'], device=device)[1]


def run(be, c: dict, gC, gA, gD, device='cpu', res=None) -> dict:
    """forward_aux + backward_aux through the backend: numpy image, alpha, depth and the six gradients under helpers.GRAD_KEYS."""
    RS = settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    res = be.forward_aux(*p, RS) if res is None else res
    dev = lambda g: None if g is None else torch.as_tensor(g).to(device)
    grads = be.backward_aux(None, dev(gC), dev(gA), dev(gD), res.image, res.depth, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
    out = {'image': res.image.cpu().numpy(), 'alpha': res.alpha.cpu().numpy(), 'depth': res.depth.cpu().numpy(), 'res': res}
    out.update({k: g.cpu().numpy() for k, g in zip(helpers.GRAD_KEYS, grads)})
    return out


def run_plain(be, c: dict, gC, device='cpu') -> dict:
    RS = settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    res = be.forward(*p, RS)
    grads = be.backward(None, torch.as_tensor(gC).to(device), res.image, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
    out = {'image': res.image.cpu().numpy()}
    out.update({k: g.cpu().numpy() for k, g in zip(helpers.GRAD_KEYS, grads)})
    return out


def check_against_reference(be, name: str, device='cpu', exact_image: bool = True) -> dict:
    """One case end to end: maps, image and the six gradients against the fp64 reference; every figure is printed before it is held to its bar."""
    c, ref = case(name), reference(name)
    out = run(be, c, c['gC'], c['gA'], c['gD'], device)
    plain = run_plain(be, c, c['gC'], device)
    ref_rgb = reference_rgb(name)
    keep = c['keep']
    report = {'zeroed': float((~keep).mean()),
              'alpha': helpers.rel_inf(out['alpha'][keep], ref['alpha'][keep]), 'depth': helpers.rel_inf(out['depth'][keep], ref['depth'][keep]),
              'image_vs_plain': float(np.abs(out['image'] - plain['image']).max())}
    for k in helpers.GRAD_KEYS:
        report[k] = helpers.rel_inf(out[k], np.asarray(ref[k]).reshape(out[k].shape))
        report[k + '_plain_rgb'] = helpers.rel_inf(plain[k], np.asarray(ref_rgb[k]).reshape(plain[k].shape))
    print(name, device, report)
    nothing = c['f']['n_processed'].reshape(keep.shape) == 0
    assert not out['alpha'][nothing].any() and not out['depth'][nothing].any(), name
    assert report['alpha'] < MAP_TOL and report['depth'] < MAP_TOL, (name, report)
    if exact_image:
        assert np.array_equal(out['image'], plain['image']), name
    else:
        assert helpers.rel_inf(out['image'], plain['image']) < MAP_TOL, (name, report)
    for k in helpers.GRAD_KEYS:
        assert report[k] < GRAD_TOL, (name, k, report)
    return report
