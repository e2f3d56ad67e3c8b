"""Scenes, fp64 reference and comparisons shared by tests/test_absgrad.py (CPU simulation) and tests/test_gpu_absgrad.py (MI355X): the absolute-gradient
densification statistic of the training render (fgs_backward_absgrad, Backend.backward_absgrad, diff_rasterize_absgrad).

Definition: for every (pixel p, Gaussian i) pair the backward blend lets contribute, the pair's share of dL/dmean2d is (gx_p, gy_p); the signed statistic
densification_info[1] accumulates sqrt((0.5 W sum_p gx_p)^2 + (0.5 H sum_p gy_p)^2), the absolute one sqrt((0.5 W sum_p |gx_p|)^2 + (0.5 H sum_p |gy_p|)^2).
Row 0 of both counts the passes in which the Gaussian was visible (n_touched != 0).

Reference: abs_reference() -- aux_grad_cases.aux_autograd_reference restated in fp64 torch with dx = mean2d.x - pixel centre and dy kept as retained dense
[P, V] tensors. They are the only places mean2d enters the image formation model, so dx.grad[p, i] IS gx_p of Gaussian i and sum_p |dx.grad[p, i]| is ax_i.
Its six gradients must equal aux_autograd_reference's to 1e-12 (asserted first, for every case), which pins it to the reference the project trusts; the
column sums of dx.grad, dy.grad must reproduce the signed statistic the library writes.

Cases: the four of aux_grad_cases.CASES with their seeded upstream gradients (zero on the reference's flip pixels, at most 0.1 % of a scene: asserted there)
and `lone`, one isotropic Gaussian whose projected mean lies on a pixel corner of a 32 x 24 image, with a constant dL/dC: every pixel's share is cancelled
by its mirror image's, the signed statistic is (nearly) zero and the absolute one is not.

Bars: row 1 against the reference -- helpers.rel_inf < aux_grad_cases.GRAD_TOL (1e-4): an absolute sum has no cancellation, so the project's gradient bar
applies unchanged; the signed statistic of the same pass against the reference's column sums at the same bar -- except on `lone`, where that statistic
is the rounding residue of sums that cancel (3e-19 in fp64) and is held to 1e-4 of the ABSOLUTE statistic, the scale of the terms it is the difference
of; row 0 exact; everything a plain / aux backward pass writes -- bit-identical on the simulation, within 1e-5 on the device (two runs that
differ by the order of the blend's float atomics: the bar of tests/test_gpu_aux_grad.py)."""
from __future__ import annotations

import functools

import numpy as np
import torch

import aux_grad_cases as aux
import helpers
from harness.scenes import View
from oracle.torch_check import _sh_color

GRAD_TOL = aux.GRAD_TOL
CASE_NAMES = tuple(aux.CASES) + ('lone',)
LONE_RATIO = 0.01                       # signed / absolute statistic of `lone`, on the reference


def lone_scene():
    """One isotropic Gaussian (sigma 1.2 px + the 0.3 px^2 blur) at the world origin, 4 units in front of a camera whose principal point (16, 12) is a
    pixel corner of the 32 x 24 image: two tiles across, two down, the footprint symmetric about the corner and well inside the image."""
    params = {
        'means': torch.zeros(1, 3), 'scales': torch.full((1, 3), float(np.log(0.15))), 'rotations': torch.tensor([[1.0, 0.0, 0.0, 0.0]]),
        'opacities': torch.tensor([[float(np.log(0.6 / 0.4))]]), 'sh_coefficients_0': torch.tensor([[[0.9, 0.2, -0.4]]]),
        'sh_coefficients_rest': torch.zeros(1, 15, 3),
    }
    w2c = torch.eye(4)
    w2c[2, 3] = 4.0
    return params, View(w2c, torch.tensor([0.0, 0.0, -4.0]), 32, 24, 32.0, 32.0, 16.0, 12.0, 0.2, 1.0e4, torch.zeros(3))


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """aux_grad_cases.case(name) for its four cases; `lone` built the same way with a constant gC and zero map gradients."""
    if name != 'lone':
        return aux.case(name)
    from oracle import oracle as O
    O.build()
    params, view = lone_scene()
    S, _ = helpers.settings_pair(view, 16, False)
    f = O.forward(*helpers.np_params(params), S, bucket_size=64)
    H, W = view.height, view.width
    flips = helpers.flip_masks(O, f, S)['pixel']
    assert float(flips.mean()) <= aux.MAX_ZEROED, ('lone', 'zeroed pixels', float(flips.mean()))
    gC = np.full((3, H, W), 1.0 / (3 * H * W), np.float32)
    gC[:, flips] = 0.0
    return {'name': name, 'params': params, 'view': view, 'K': 16, 'aa': False, 'S': S, 'f': f, 'keep': ~flips, 'gC': gC,
            'gA': np.zeros((H, W), np.float32), 'gD': np.zeros((H, W), np.float32)}


def abs_reference(params: dict, S, fwd: dict, gC, gA, gD) -> dict:
    """aux_grad_cases.aux_autograd_reference, statement for statement, with dx and dy retained: the six gradients under their oracle names plus, per
    Gaussian [N], 'sx', 'sy' = sum_p dx.grad, dy.grad (what the record's words 0 and 1 hold) and 'ax', 'ay' = sum_p |dx.grad|, |dy.grad|."""
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
    dx = mean2d[None, :, 0] - (xs.double() + 0.5)[:, None]              # [P, V]: retained, the only places mean2d enters below
    dy = mean2d[None, :, 1] - (ys.double() + 0.5)[:, None]
    dx.retain_grad()
    dy.retain_grad()
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
    A = w.sum(dim=1).reshape(H, W)
    D = (w @ depth).reshape(H, W)
    loss = (image * t(gC).reshape(3, H, W)).sum() + (A * t(gA).reshape(H, W)).sum() + (D * t(gD).reshape(H, W)).sum()
    loss.backward()
    out = {'image': image.detach().numpy()}
    for k, v in P.items():
        out[k] = v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))
    gx = dx.grad if dx.grad is not None else torch.zeros_like(dx)
    gy = dy.grad if dy.grad is not None else torch.zeros_like(dy)
    idx = order.numpy()
    for key, col in (('sx', gx.sum(dim=0)), ('sy', gy.sum(dim=0)), ('ax', gx.abs().sum(dim=0)), ('ay', gy.abs().sum(dim=0))):
        full = np.zeros(N)
        full[idx] = col.numpy()
        out[key] = full
    return out


def statistic(sum_x: np.ndarray, sum_y: np.ndarray, width: int, height: int) -> np.ndarray:
    """Row 1 of a densification tensor from the two per-Gaussian sums, in fp64."""
    return np.sqrt((0.5 * width * np.asarray(sum_x, np.float64)) ** 2 + (0.5 * height * np.asarray(sum_y, np.float64)) ** 2)


@functools.lru_cache(maxsize=None)
def reference(name: str, maps: bool) -> dict:
    """The fp64 reference of case `name` for (gC, gA, gD) or, maps=False, for gC alone: once per process, shared, read-only. Adds 'abs' and 'signed', the
    two statistics' row 1."""
    c = case(name)
    zero = 0.0 * c['gA']
    ref = abs_reference(aux.named_params(c['params']), c['S'], c['f'], c['gC'], c['gA'] if maps else zero, c['gD'] if maps else zero)
    W, H = c['view'].width, c['view'].height
    ref['abs'], ref['signed'] = statistic(ref['ax'], ref['ay'], W, H), statistic(ref['sx'], ref['sy'], W, H)
    return ref


def trusted_reference(name: str, maps: bool) -> dict:
    """aux_grad_cases' own reference for the same upstream gradients (cached there for its four cases)."""
    if name != 'lone':
        return aux.reference(name) if maps else aux.reference_rgb(name)
    c = case(name)
    zero = 0.0 * c['gA']
    return aux.aux_autograd_reference(aux.named_params(c['params']), c['S'], c['f'], c['gC'], c['gA'] if maps else zero, c['gD'] if maps else zero)


def check_reference_is_the_trusted_one(name: str) -> None:
    for maps in (False, True):
        mine, theirs = reference(name, maps), trusted_reference(name, maps)
        assert np.abs(mine['image'] - theirs['image']).max() < 1e-12, (name, maps)
        for k in ('means', 'scales', 'rotations', 'opacities', 'sh0', 'sh_rest'):
            assert helpers.rel_inf(mine[k], theirs[k]) < 1e-12, (name, maps, k)
        assert (mine['ax'] >= np.abs(mine['sx'])).all() and (mine['ay'] >= np.abs(mine['sy'])).all(), (name, maps)


def settings_of(c: dict, device='cpu'):
    return helpers.settings_pair(c['view'], c['K'], c['aa'], device=device)[1]


def forward(be, c: dict, maps: bool, device='cpu'):
    RS = settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    return be.forward_aux(*p, RS) if maps else be.forward(*p, RS)


def visible(be, c: dict, res) -> np.ndarray:
    """n_touched != 0 per Gaussian, read from the primitive blob of the forward pass."""
    n, v = c['params']['means'].shape[0], c['view']
    layout = be.blob_layout(0, n, v.width, v.height, res.state[1], res.state[2])
    return be.view(res.buffers[0].cpu(), layout, 'n_touched', torch.int32).numpy() != 0


def run(be, c: dict, maps: bool, device='cpu', res=None, absgrad: bool = True, dens=None, abs_info=None, signed: bool = True) -> dict:
    """One backward pass over (new or retained) forward buffers: backward_absgrad, or -- absgrad=False -- backward_aux / backward on the same arguments.
    Returns numpy gradients under helpers.GRAD_KEYS, 'dens' and 'abs' [2, N] (accumulated into `dens` / `abs_info` if given), both flag arrays, 'res'."""
    RS = settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    n = p[0].shape[0]
    res = forward(be, c, maps, device) if res is None else res
    dev = lambda g: torch.as_tensor(g).to(device)
    gA, gD, depth = (dev(c['gA']), dev(c['gD']), res.depth) if maps else (None, None, None)
    dens = (torch.zeros(2, n, device=device) if dens is None else dens) if signed else None
    abs_info = torch.zeros(2, n, device=device) if abs_info is None else abs_info
    live, reached = torch.zeros((2, (n + 63) // 64), dtype=torch.uint8, device=device)
    tail = (res.image, depth, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
    if absgrad:
        grads = be.backward_absgrad(dens, abs_info, dev(c['gC']), gA, gD, *tail, live_blocks=live, reached_blocks=reached)
    else:
        grads = be.backward_aux(dens, dev(c['gC']), gA, gD, *tail, live_blocks=live, reached_blocks=reached)
    out = {k: g.cpu().numpy() for k, g in zip(helpers.GRAD_KEYS, grads)}
    out.update(dens=None if dens is None else dens.cpu().numpy(), abs=abs_info.cpu().numpy(), live=live.cpu().numpy(), reached=reached.cpu().numpy(), res=res)
    return out


_RUNS: dict = {}


def run_once(be, name: str, maps: bool, device='cpu') -> dict:
    """run() with zeroed statistics tensors on fresh forward buffers, once per (backend, case, maps, device): shared, read-only (its 'res' may be walked
    again by a retained-buffer pass, which leaves the forward buffers as valid as it found them)."""
    key = (id(be.lib), name, maps, str(device))
    if key not in _RUNS:
        _RUNS[key] = run(be, case(name), maps, device)
    return _RUNS[key]


def check_parity(be, name: str, maps: bool, device='cpu') -> dict:
    """1. Row 1 against the fp64 reference, row 0 exactly the visibility; the signed statistic of the same pass against the reference's column sums."""
    c, ref = case(name), reference(name, maps)
    out = run_once(be, name, maps, device)
    vis = visible(be, c, out['res'])
    report = {'abs': helpers.rel_inf(out['abs'][1], ref['abs']), 'signed': helpers.rel_inf(out['dens'][1], ref['signed']),
              'signed_vs_abs_scale': float(np.abs(out['dens'][1] - ref['signed']).max() / (ref['abs'].max() + 1e-30)),
              'max_abs': float(ref['abs'].max()), 'max_signed': float(ref['signed'].max())}
    print(name, 'maps' if maps else 'rgb', device, report)
    assert np.array_equal(out['abs'][0], vis.astype(np.float32)), name
    assert np.array_equal(out['dens'][0], vis.astype(np.float32)), name
    assert ref['abs'].max() > 0 and report['abs'] < GRAD_TOL, (name, maps, report)
    if name == 'lone':          # the signed statistic cancels to (nearly) nothing there: held at the scale of the sums it is the difference of
        assert report['signed_vs_abs_scale'] < GRAD_TOL, (name, maps, report)
    else:
        assert report['signed'] < GRAD_TOL, (name, maps, report)
    return out


def check_nothing_else_moves(be, name: str, maps: bool, device='cpu', exact: bool = True) -> None:
    """2. The six gradients, densification_info and the block flags of a backward_absgrad call against backward_aux / backward on the same forward buffers."""
    c = case(name)
    with_abs = run_once(be, name, maps, device)
    without = run(be, c, maps, device, res=with_abs['res'], absgrad=False)
    assert np.array_equal(with_abs['live'], without['live']) and np.array_equal(with_abs['reached'], without['reached']), name
    for k in helpers.GRAD_KEYS + ('dens',):
        if exact:
            assert np.array_equal(with_abs[k], without[k]), (name, maps, k)
        else:
            assert helpers.rel_inf(with_abs[k], without[k]) < 1e-5, (name, maps, k)
    assert not without['abs'].any()


def check_identities(be, device='cpu') -> None:
    """3. abs >= signed per Gaussian (within 1e-6 abs) in every case; on `lone` the REFERENCE's signed / abs ratio is below LONE_RATIO -- a property of the
    scene -- and the library matches the reference on both statistics (check_parity)."""
    for name in CASE_NAMES:
        out = run_once(be, name, True, device)
        assert (out['abs'][1] >= out['dens'][1] - 1e-6 * out['abs'][1]).all(), name
    for maps in (False, True):
        ref = reference('lone', maps)
        assert ref['abs'][0] > 0 and ref['signed'][0] / ref['abs'][0] < LONE_RATIO, (maps, ref['signed'], ref['abs'])
        out = check_parity(be, 'lone', maps, device)
        assert out['dens'][1][0] < LONE_RATIO * out['abs'][1][0]


def check_accumulation(be, name: str = 'hot', device='cpu', tol: float = 1e-6) -> None:
    """4. A second backward call over the retained buffers of the first, into the tensors the first one filled, doubles both rows (the pass clears its
    own sums, replicas included, and adds to what it finds); a tensor that arrives non-zero is added to, not overwritten, with no signed tensor given."""
    c = case(name)
    once = run_once(be, name, True, device)
    dens, info = torch.as_tensor(once['dens']).to(device).clone(), torch.as_tensor(once['abs']).to(device).clone()
    twice = run(be, c, True, device, res=once['res'], dens=dens, abs_info=info)
    assert np.array_equal(twice['abs'][0], 2.0 * once['abs'][0]) and helpers.rel_inf(twice['abs'][1], 2.0 * once['abs'][1]) < tol
    assert np.array_equal(twice['dens'][0], 2.0 * once['dens'][0]) and helpers.rel_inf(twice['dens'][1], 2.0 * once['dens'][1]) < tol
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(twice[k], once[k]) < max(tol, 1e-6), k
    small, first = case('partial_tiles'), run_once(be, 'partial_tiles', False, device)
    seeded = torch.full((2, small['params']['means'].shape[0]), 3.0, device=device)
    added = run(be, small, False, device, res=first['res'], abs_info=seeded, signed=False)
    assert added['dens'] is None and helpers.rel_inf(added['abs'], 3.0 + first['abs']) < tol


def check_operator(B, be, name: str = 'partial_tiles', device='cpu', tol: float = 1e-6) -> None:
    """6. diff_rasterize_absgrad: outputs, gradients and statistic equal the backend's; torch.empty(0) gives diff_rasterize's gradients."""
    c = case(name)
    RS = settings_of(c, device)
    n = c['params']['means'].shape[0]
    gC, gA, gD = (torch.as_tensor(c[k]).to(device) for k in ('gC', 'gA', 'gD'))
    leaves = lambda: [c['params'][k].to(device).requires_grad_(True) for k in helpers.NAMES]
    direct = run_once(be, name, True, device)
    lv, info, dens = leaves(), torch.zeros(2, n, device=device), torch.zeros(2, n, device=device)
    image, alpha, depth = B.diff_rasterize_absgrad(*lv, dens, RS, info, alpha=True, depth=True)
    assert image.shape == (3, c['view'].height, c['view'].width) and alpha.shape == depth.shape == image.shape[1:]
    grads = torch.autograd.grad((image * gC).sum() + (alpha * gA).sum() + (depth * gD).sum(), lv)
    for k, g in zip(helpers.GRAD_KEYS, grads):
        assert helpers.rel_inf(g.cpu().numpy(), direct[k]) < tol, k
    assert helpers.rel_inf(info.cpu().numpy(), direct['abs']) < tol and helpers.rel_inf(dens.cpu().numpy(), direct['dens']) < tol
    assert not info.requires_grad

    plain_direct = run_once(be, name, False, device)
    lv, info = leaves(), torch.zeros(2, n, device=device)
    image, alpha, depth = B.diff_rasterize_absgrad(*lv, torch.empty(0), RS, info)
    assert alpha is None and depth is None
    grads = torch.autograd.grad((image * gC).sum(), lv)
    assert helpers.rel_inf(info.cpu().numpy(), plain_direct['abs']) < tol
    lv2 = leaves()
    empty = torch.autograd.grad((B.diff_rasterize_absgrad(*lv2, torch.empty(0), RS, torch.empty(0))[0] * gC).sum(), lv2)
    lv3 = leaves()
    plain = torch.autograd.grad((B.diff_rasterize(*lv3, torch.empty(0), RS) * gC).sum(), lv3)
    for k, g, e, p in zip(helpers.GRAD_KEYS, grads, empty, plain):
        assert helpers.rel_inf(e.cpu().numpy(), p.cpu().numpy()) < tol and helpers.rel_inf(g.cpu().numpy(), p.cpu().numpy()) < tol, k
