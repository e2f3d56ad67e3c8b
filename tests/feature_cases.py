"""Scenes, fp64 reference and comparisons shared by tests/test_feature_render.py (CPU simulation) and tests/test_gpu_feature_render.py (MI355X): the
training render that also blends F per-Gaussian feature channels, M_c = sum_i w_i f_{i,c}, differentiably (fgs_blend_features / fgs_backward_features,
diff_rasterize_features).

Scenes: aux_grad_cases.case(name), all four (their path conditions and the cap on zeroed flip pixels are asserted there and in test_aux_grad.py).
Reference: aux_grad_cases.aux_autograd_reference's construction with one more output of the same compositing weights, M = (w @ F).T.reshape(F,H,W), and
its term in the loss; the graph of a case is built once and differentiated per channel count. With gF = 0 it must give aux_grad_cases.reference_rgb.
Features: seeded standard normal (both signs). Upstream gradients: aux_grad_cases' gC, and a seeded normal gF / (F H W), zero on the flip pixels like gC.
Bars: aux_grad_cases.MAP_TOL for maps, GRAD_TOL for each gradient tensor (rel_inf against fp64), 1e-5 between two runs of the same pass (the order
of the float atomics is the only difference)."""
from __future__ import annotations

import functools

import numpy as np
import torch

import aux_grad_cases as aux
import helpers
from oracle.torch_check import _sh_color

MAP_TOL, GRAD_TOL = aux.MAP_TOL, aux.GRAD_TOL
RERUN_TOL = 1e-5
CHANNELS = (1, 5, 16, 35)              # one narrow walk, a ragged one, one full line, three walks with a ragged last one
WIDE_CASES = ('partial_tiles', 'hot')  # where F = 35 runs
SH_C0 = 0.28209479177387814
PARITY = [(name, f) for name in aux.CASES for f in CHANNELS if f != 35 or name in WIDE_CASES]


def features(name: str, n_channels: int) -> np.ndarray:
    """[N, F] float32, the first F columns of one seeded draw per case."""
    n = aux.case(name)['params']['means'].shape[0]
    return np.ascontiguousarray(np.random.default_rng(23).standard_normal((n, 64)).astype(np.float32)[:, :n_channels])


def grad_map(name: str, n_channels: int) -> np.ndarray:
    """gF [F,H,W] float32: seeded normal / (F H W), zero on the flip pixels."""
    c = aux.case(name)
    H, W = c['view'].height, c['view'].width
    g = (np.random.default_rng(29 + n_channels).standard_normal((n_channels, H, W)) / (n_channels * H * W)).astype(np.float32)
    g[:, ~c['keep']] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def _graph(name: str) -> dict:
    """The fp64 autograd graph of case `name` up to the image and the compositing weights (aux_grad_cases.aux_autograd_reference, restated)."""
    c = aux.case(name)
    params, S, fwd = aux.named_params(c['params']), c['S'], c['f']
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
    a, cc = a_raw + ks, c_raw + ks
    det = a * cc - b * b
    conic = torch.stack([cc / det, -b / det, a / det], dim=1)
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
    return {'P': P, 'order': order, 'w': w, 'image': image, 'H': H, 'W': W, 'N': N}


def feature_autograd_reference(name: str, feats: np.ndarray, gC: np.ndarray, gF: np.ndarray) -> dict:
    """fp64 image, feature map, the six gradients and grad_features of sum(gC image) + sum(gF M)."""
    G = _graph(name)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    Fe = t(feats).requires_grad_(True)
    n_channels, H, W = Fe.shape[1], G['H'], G['W']
    M = (G['w'] @ Fe[G['order']]).T.reshape(n_channels, H, W)
    loss = (G['image'] * t(gC).reshape(3, H, W)).sum() + (M * t(gF).reshape(n_channels, H, W)).sum()
    leaves = list(G['P'].values()) + [Fe]
    grads = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    out = {'image': G['image'].detach().numpy(), 'map': M.detach().numpy()}
    for (k, v), g in zip(list(G['P'].items()) + [('features', Fe)], grads):
        out[k] = g.numpy() if g is not None else np.zeros(tuple(v.shape))
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str, n_channels: int) -> dict:
    """The fp64 reference of (case, F) for aux_grad_cases' gC and this module's features and gF: once per process, shared, read-only."""
    return feature_autograd_reference(name, features(name, n_channels), aux.case(name)['gC'], grad_map(name, n_channels))


def run(be, c: dict, feats, gC, gF, device='cpu', detach: bool = False, res=None, RS=None, params=None) -> dict:
    """forward + blend_features + backward_features through the backend: numpy image, map, the six gradients under helpers.GRAD_KEYS, 'features'."""
    RS = aux.settings_of(c, device) if RS is None else RS
    p = [(c['params'] if params is None else params)[k].to(device) for k in helpers.NAMES]
    res = be.forward(*p, RS) if res is None else res
    fe = torch.as_tensor(feats).to(device)
    fmap = be.blend_features(fe, res, p[0].shape[0], RS)
    dev = lambda g: None if g is None else torch.as_tensor(g).to(device)
    grads = be.backward_features(None, dev(gC), dev(gF), res.image, fmap, fe, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state, detach)
    out = {'image': res.image.cpu().numpy(), 'map': fmap.cpu().numpy(), 'res': res, 'fmap': fmap}
    out.update({k: g.cpu().numpy() for k, g in zip(helpers.GRAD_KEYS, grads[:6])})
    out['features'] = None if grads[6] is None else grads[6].cpu().numpy()
    return out


def check_against_reference(be, name: str, n_channels: int, device='cpu', exact_image: bool = True) -> dict:
    """One (case, F) end to end: map, image, the six gradients and grad_features against fp64; every figure is printed before it is held to its bar."""
    c, ref = aux.case(name), reference(name, n_channels)
    out = run(be, c, features(name, n_channels), c['gC'], grad_map(name, n_channels), device)
    plain = aux.run_plain(be, c, c['gC'], device)
    keep = c['keep']
    report = {'zeroed': float((~keep).mean()), 'map': helpers.rel_inf(out['map'][:, keep], ref['map'][:, keep]),
              'image_vs_plain': float(np.abs(out['image'] - plain['image']).max())}
    for k in helpers.GRAD_KEYS + ('features',):
        report[k] = helpers.rel_inf(out[k], np.asarray(ref[k]).reshape(out[k].shape))
    print(name, n_channels, device, report)
    nothing = c['f']['n_processed'].reshape(keep.shape) == 0
    assert not out['map'][:, nothing].any(), name
    assert report['map'] < MAP_TOL, (name, n_channels, report)
    if exact_image:
        assert np.array_equal(out['image'], plain['image']), name
    else:
        assert helpers.rel_inf(out['image'], plain['image']) < MAP_TOL, (name, report)
    for k in helpers.GRAD_KEYS + ('features',):
        assert report[k] < GRAD_TOL, (name, n_channels, k, report)
    return report


def check_reference_without_feature_gradient(name: str) -> None:
    """gF = 0: the reference IS aux_grad_cases.reference_rgb (image and all six gradients), which pins it to the reference the project trusts."""
    c = aux.case(name)
    mine = feature_autograd_reference(name, features(name, 5), c['gC'], 0.0 * grad_map(name, 5))
    theirs = aux.reference_rgb(name)
    assert np.abs(mine['image'] - theirs['image']).max() < 1e-12
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(mine[k], np.asarray(theirs[k]).reshape(mine[k].shape)) < 1e-12, (name, k)
    assert not mine['features'].any()


def view_depths(c: dict, means: torch.Tensor) -> torch.Tensor:
    """z_i = row 2 of w2c applied to the mean, in torch (differentiable in the means)."""
    w2c = c['view'].w2c.to(means.device, means.dtype)
    return means @ w2c[2, :3] + w2c[2, 3]


def check_identities(be, device='cpu') -> None:
    """A ones channel is forward_aux's alpha, a channel of z_i its depth map; on `stacked` with a black background three channels max(0, 0.5 + C0 sh0)
    are the image; the six gradients of a depth-channel loss are backward_aux's for the same gD once autograd has added z's own dependence on the mean."""
    name = 'partial_tiles'
    c = aux.case(name)
    RS = aux.settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    n, keep = p[0].shape[0], c['keep']
    res = be.forward_aux(*p, RS)                                     # its buffers serve the feature blend as well
    means = p[0].clone().requires_grad_(True)
    z = view_depths(c, means)
    two = torch.stack([torch.ones_like(z), z], dim=1).detach().contiguous()
    fmap = be.blend_features(two, res, n, RS).cpu().numpy()
    report = {'ones_vs_alpha': helpers.rel_inf(fmap[0][keep], res.alpha.cpu().numpy()[keep]), 'z_vs_depth': helpers.rel_inf(fmap[1][keep], res.depth.cpu().numpy()[keep])}
    print('identities', device, report)
    assert report['ones_vs_alpha'] < MAP_TOL and report['z_vs_depth'] < MAP_TOL, report

    gD = torch.as_tensor(c['gD']).to(device)
    zero_image = torch.zeros_like(res.image)
    want = be.backward_aux(None, zero_image, None, gD, res.image, res.depth, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
    zf = z.detach().reshape(n, 1).contiguous()
    zmap = be.blend_features(zf, res, n, RS)
    got = be.backward_features(None, zero_image, gD[None].contiguous(), res.image, zmap, zf, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
    (through_z,) = torch.autograd.grad((z * got[6].reshape(-1)).sum(), means)
    got = (got[0] + through_z,) + tuple(got[1:6])
    for k, g, w in zip(helpers.GRAD_KEYS, got, want):
        figure = helpers.rel_inf(g.cpu().numpy(), w.cpu().numpy())
        print('depth channel', device, k, figure)
        assert figure < GRAD_TOL, (k, figure)

    st = aux.case('stacked')
    assert st['K'] == 1
    _, RS0 = helpers.settings_pair(st['view'], 1, st['aa'], bg=(0.0, 0.0, 0.0), device=device)
    ps = [st['params'][k].to(device) for k in helpers.NAMES]
    plain = be.forward(*ps, RS0)
    colour = (0.5 + SH_C0 * ps[4].reshape(-1, 3)).clamp_min(0.0).contiguous()
    cmap = be.blend_features(colour, plain, ps[0].shape[0], RS0).cpu().numpy()
    figure = helpers.rel_inf(cmap[:, st['keep']], plain.image.cpu().numpy()[:, st['keep']])
    print('colour channels vs image', device, figure)
    assert figure < MAP_TOL, figure


def check_workaround_parity(be, device='cpu') -> None:
    """Non-negative features pushed through the colour path as sh0 = (f - 0.5) / C0 with active_sh_bases = 1: grad_features = grad_sh0 / C0."""
    c = aux.case('stacked')
    gF = grad_map('stacked', 3)
    f = np.abs(features('stacked', 3))
    _, RS0 = helpers.settings_pair(c['view'], 1, c['aa'], bg=(0.0, 0.0, 0.0), device=device)
    mine = run(be, c, f, np.zeros_like(c['gC']), gF, device, RS=RS0)
    params = dict(c['params'])
    params['sh_coefficients_0'] = ((torch.as_tensor(f) - 0.5) / SH_C0).reshape(-1, 1, 3).contiguous()
    p = [params[k].to(device) for k in helpers.NAMES]
    res = be.forward(*p, RS0)
    grads = be.backward(None, torch.as_tensor(gF).to(device), res.image, p[0], p[1], p[2], p[3], p[5], res.buffers, RS0, res.state)
    figure = helpers.rel_inf(mine['features'], grads[4].cpu().numpy().reshape(-1, 3) / SH_C0)
    print('workaround parity', device, figure, 'map', helpers.rel_inf(mine['map'][:, c['keep']], res.image.cpu().numpy()[:, c['keep']]))
    assert figure < GRAD_TOL, figure


def check_detached_and_retained(be, device='cpu') -> None:
    """detach_geometry: grad_features unchanged, the six gradients the plain RGB pass's; no feature gradient: `backward`; a second pass over retained
    buffers equals the first."""
    name, n_channels = 'hot', 5
    c = aux.case(name)
    f, gF = features(name, n_channels), grad_map(name, n_channels)
    first = run(be, c, f, c['gC'], gF, device)
    plain = aux.run_plain(be, c, c['gC'], device)
    detached = run(be, c, f, c['gC'], gF, device, detach=True)
    assert helpers.rel_inf(detached['features'], first['features']) < RERUN_TOL
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(detached[k], plain[k]) < RERUN_TOL, ('detached', k)
    none = run(be, c, f, c['gC'], None, device)
    assert none['features'] is None
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(none[k], plain[k]) < RERUN_TOL, ('no feature gradient', k)
    second = run(be, c, f, c['gC'], gF, device, res=first['res'])
    for k in helpers.GRAD_KEYS + ('features',):
        assert helpers.rel_inf(second[k], first[k]) < RERUN_TOL, ('second pass', k)
    assert max(float(np.abs(first[k] - plain[k]).max()) for k in ('means', 'scales', 'rotations', 'opacities')) > 0       # the feature term is there


def check_errors_and_empty(be, device='cpu') -> None:
    """Every refusal with its text, and n = 0."""
    import pytest
    c = aux.case('partial_tiles')
    RS = aux.settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    n, H, W = p[0].shape[0], c['view'].height, c['view'].width
    total_rest = p[5].shape[1]
    res = be.forward(*p, RS)
    f = torch.as_tensor(features('partial_tiles', 5)).to(device)
    gi = torch.as_tensor(c['gC']).to(device)
    fmap = be.blend_features(f, res, n, RS)
    back = lambda feats, fm, gm, r=res: be.backward_features(None, gi, gm, r.image, fm, feats, p[0], p[1], p[2], p[3], p[5], r.buffers, RS, r.state)
    for bad in (0, 65):
        wide = torch.zeros((n, bad), device=device)
        with pytest.raises(RuntimeError, match='1..64 channels'):
            be.blend_features(wide, res, n, RS)
        with pytest.raises(RuntimeError, match='1..64 channels'):
            back(wide, torch.zeros((bad, H, W), device=device), torch.zeros((bad, H, W), device=device))
    with pytest.raises(RuntimeError, match=r'features must be a contiguous float32 \[N, F\]'):
        be.blend_features(f[:-1].contiguous(), res, n, RS)
    with pytest.raises(RuntimeError, match=r'features must be a contiguous float32 \[N, F\]'):
        back(f[:-1].contiguous(), fmap, fmap)
    with pytest.raises(RuntimeError, match=r'features must be a contiguous float32 \[N, F\]'):
        be.blend_features(f.t().contiguous().t(), res, n, RS)
    with pytest.raises(RuntimeError, match='grad_feature_map must be'):
        back(f, fmap, fmap[:3])
    asynchronous = be.forward(*p, RS, instance_capacity=1 << 20)
    with pytest.raises(RuntimeError, match='fgs_forward_async'):
        be.blend_features(f, asynchronous, n, RS)
    with pytest.raises(RuntimeError, match='fgs_forward_async'):
        back(f, fmap, fmap, asynchronous)
    # the record path for real: one owner's K1, then the render from its splat records -- the state that pass returns is refused
    rec = torch.zeros((1, n, 56), dtype=torch.uint8, device=device)
    counts = torch.zeros((1, 2), dtype=torch.int32, device=device)
    be.shard_preprocess(*p, [RS], rec, counts)
    n_visible, n_instances = (int(x) for x in counts[0].cpu())
    assert n_visible > 0
    records = be.forward_from_records(rec.view(-1), n_visible, n_instances, RS, total_rest)
    with pytest.raises(RuntimeError, match='record'):
        be.blend_features(f[:n_visible].contiguous(), records, n_visible, RS)
    with pytest.raises(RuntimeError, match='record'):
        be.backward_features(None, gi, fmap, records.image, fmap, f[:n_visible].contiguous(), p[0][:n_visible].contiguous(), p[1][:n_visible].contiguous(),
                             p[2][:n_visible].contiguous(), p[3][:n_visible].contiguous(), p[5][:n_visible].contiguous(), records.buffers, RS, records.state)
    with pytest.raises(RuntimeError, match='takes no feature-map gradient'):
        be.backward_adam_fused(None, gi, res.image, [], [], [], res.buffers, RS, res.state, 1, [], grad_feature_map=fmap)
    with pytest.raises(RuntimeError, match='takes no feature-map gradient'):
        be.backward_to_records(gi, res.image, res.buffers, RS, res.state, 15, grad_feature_map=fmap)
    # n = 0: a zero map, empty gradients
    empty = [t[:0].contiguous() for t in p]
    r0 = be.forward(*empty, RS)
    f0 = torch.zeros((0, 5), device=device)
    m0 = be.blend_features(f0, r0, 0, RS)
    assert m0.shape == (5, H, W) and not m0.any()
    g0 = be.backward_features(None, torch.ones_like(r0.image), torch.ones_like(m0), r0.image, m0, f0, empty[0], empty[1], empty[2], empty[3], empty[5],
                              r0.buffers, RS, r0.state)
    assert all(g.shape[0] == 0 for g in g0) and g0[6].shape == (0, 5)


def check_operator(B, be, name: str, device='cpu') -> None:
    """The public operator B.diff_rasterize_features against the backend `be` it runs on: outputs and the seven gradients equal to the backend's, a second
    backward over the retained graph, a non-contiguous gF, features that do not require grad, an unused map = the plain pass, detach_geometry,
    torch.no_grad()."""
    n_channels = 5
    c = aux.case(name)
    RS = aux.settings_of(c, device)
    gC = torch.as_tensor(c['gC']).to(device)
    gF = torch.as_tensor(grad_map(name, n_channels)).to(device)
    f = features(name, n_channels)
    leaves_of = lambda: [c['params'][k].to(device).clone().requires_grad_(True) for k in helpers.NAMES]
    feats_of = lambda grad: torch.as_tensor(f).to(device).clone().requires_grad_(grad)
    none = torch.empty(0)
    direct = run(be, c, f, c['gC'], gF, device)

    leaves, fe = leaves_of(), feats_of(True)
    image, fmap = B.diff_rasterize_features(*leaves, none, RS, fe)
    assert image.shape == (3, c['view'].height, c['view'].width) and fmap.shape == (n_channels,) + image.shape[1:]
    assert torch.equal(fmap.detach().cpu(), torch.as_tensor(direct['map'])) and torch.equal(image.detach().cpu(), torch.as_tensor(direct['image']))
    loss = (image * gC).sum() + (fmap * gF).sum()
    first = torch.autograd.grad(loss, leaves + [fe], retain_graph=True)
    second = torch.autograd.grad(loss, leaves + [fe])
    for k, g1, g2 in zip(helpers.GRAD_KEYS + ('features',), first, second):
        assert helpers.rel_inf(g1.cpu().numpy(), direct[k]) < RERUN_TOL, k
        assert helpers.rel_inf(g2.cpu().numpy(), g1.cpu().numpy()) < RERUN_TOL, k

    # a non-contiguous incoming gradient is made contiguous; features without requires_grad get no gradient and raise nothing
    leaves, fe = leaves_of(), feats_of(False)
    image, fmap = B.diff_rasterize_features(*leaves, none, RS, fe)
    gF_t = gF.transpose(1, 2).contiguous().transpose(1, 2)
    assert not gF_t.is_contiguous()
    strided = torch.autograd.grad((image * gC).sum() + (fmap * gF_t).sum(), leaves)
    for k, g in zip(helpers.GRAD_KEYS, strided):
        assert helpers.rel_inf(g.cpu().numpy(), direct[k]) < RERUN_TOL, k

    # the map is not part of the loss: the pass is the plain one and the features get no gradient
    leaves, fe = leaves_of(), feats_of(True)
    image, _ = B.diff_rasterize_features(*leaves, none, RS, fe)
    unused = torch.autograd.grad((image * gC).sum(), leaves + [fe], allow_unused=True)
    assert unused[6] is None
    leaves = leaves_of()
    plain = torch.autograd.grad((B.diff_rasterize(*leaves, none, RS) * gC).sum(), leaves)
    for k, g, q in zip(helpers.GRAD_KEYS, unused, plain):
        assert helpers.rel_inf(g.cpu().numpy(), q.cpu().numpy()) < RERUN_TOL, k

    # the image is not part of the loss: its gradient arrives as None and is passed on as zeros; with detach_geometry the Gaussians then get exact zeros
    leaves, fe = leaves_of(), feats_of(True)
    _, fmap = B.diff_rasterize_features(*leaves, none, RS, fe, detach_geometry=True)
    only = torch.autograd.grad((fmap * gF).sum(), leaves + [fe])
    assert all(not g.any() for g in only[:6])
    assert helpers.rel_inf(only[6].cpu().numpy(), direct['features']) < RERUN_TOL
    leaves, fe = leaves_of(), feats_of(True)
    _, fmap = B.diff_rasterize_features(*leaves, none, RS, fe)
    attached = torch.autograd.grad((fmap * gF).sum(), leaves + [fe])
    want = run(be, c, f, np.zeros_like(c['gC']), gF, device)
    for k, g in zip(helpers.GRAD_KEYS + ('features',), attached):
        assert helpers.rel_inf(g.cpu().numpy(), want[k]) < RERUN_TOL, k
    assert float(attached[0].abs().max()) > 0

    with torch.no_grad():
        image, fmap = B.diff_rasterize_features(*leaves_of(), none, RS, feats_of(False))
    assert not fmap.requires_grad and torch.equal(fmap.cpu(), torch.as_tensor(direct['map']))
    # a wrong row count is the backend's refusal, with its text
    import pytest
    with pytest.raises(RuntimeError, match=r'features must be a contiguous float32 \[N, F\]'):
        B.diff_rasterize_features(*leaves_of(), none, RS, feats_of(False)[:-1])
