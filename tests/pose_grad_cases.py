"""Scenes, fp64 reference, upstream gradients and comparisons shared by tests/test_pose_grad.py (CPU simulation) and tests/test_gpu_pose_grad.py (MI355X):
the camera-pose gradients of the training render (fgs_backward_pose, Backend.backward_pose, diff_rasterize_pose).

Definitions (include/fgs_hip.h): W = w2c[:3,:3], t = w2c[:3,3], c = cam_position are INDEPENDENT inputs; p_i = W m_i + t, J_i W the
projected Jacobian with the clipped x/z, y/z, the colour a function of m_i - c; L = <gC, image> + <gA, A> + <gD, D>.

Reference: pose_autograd_reference() -- tests/aux_grad_cases.py: aux_autograd_reference restated line for line with w2c[:3,:4] and cam_position as
fp64 autograd leaves beside the six parameter tensors. It is pinned twice in test_pose_grad.py: with the camera leaves detached it gives
aux_autograd_reference's six gradients, and its 15 camera gradients agree with fp64 central differences of oracle/torch_check.py: autograd_reference.

Upstream gradients: NOT noise -- a random-sign gC makes each of the 15 sums over all Gaussians pure cancellation. gC = image - target with the target the
fp64 reference image of the same scene from a camera moved by a small seeded rigid motion (what pose refinement backpropagates), gA and gD likewise from
that camera's maps; all three ZERO on the reference's flip pixels (helpers.flip_masks(...)['pixel']), at most 0.1 % of a scene's pixels.

Bar: helpers.rel_inf < 1e-4 against fp64, separately for grad_w2c (12 entries) and grad_cam_position (3). Precondition (test_pose_grad.py): the same
torch graph evaluated in float32 stays inside the bar on every scene -- else the scene is ill-conditioned and gets another seed, never a wider bar."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import aux_grad_cases as aux
import helpers
from harness.scenes import View, make_s0
from oracle.torch_check import _sh_color

GRAD_TOL = aux.GRAD_TOL                 # 1e-4, the project's bar
MAX_ZEROED = aux.MAX_ZEROED             # 1e-3 of a scene's pixels
CAMERA_KEYS = ('w2c', 'cam')


def ragged_scene(seed: int = 5):
    """150 Gaussians at 96 x 72: one workgroup of K12 whose third wave is partial (22 lanes in range)."""
    p, v = make_s0(seed=seed, n=150)
    return p, View(v.w2c, v.position, 96, 72, 96.0, 96.0, 48.0, 36.0, 0.2, 1e4, torch.zeros(3))


def clipped_scene(seed: int = 9):
    """200 large Gaussians spread to three times the image's width at 96 x 72: some whose centre projects beyond the +-15 % clip range in x still reach
    pixels -- K12's valid_x branch (and, spread less, in y: valid_y)."""
    p, v = make_s0(seed=seed, n=200)
    p['means'][:, 0] = p['means'][:, 0] * 3.2
    p['means'][:, 1] = p['means'][:, 1] * 2.0
    p['scales'] = p['scales'] + 1.3
    p['opacities'] = p['opacities'] - 1.0
    return p, View(v.w2c, v.position, 96, 72, 96.0, 96.0, 48.0, 36.0, 0.2, 1e4, torch.zeros(3))


# name -> (scene, active_sh_bases, proper_antialiasing, seed of the target camera's motion)
CASES = {name: (make, K, aa, 101 + i) for i, (name, (make, K, aa)) in enumerate(aux.CASES.items())}
CASES['ragged'] = (ragged_scene, 16, False, 111)
CASES['clipped'] = (clipped_scene, 16, True, 112)


def rigid_motion(seed: int, angle: float, shift: float) -> np.ndarray:
    """fp64 [4,4] rigid motion: a rotation by `angle` radians about a seeded axis and a translation of length `shift` in a seeded direction."""
    rng = np.random.default_rng(seed)
    axis, d = rng.standard_normal(3), rng.standard_normal(3)
    axis, d = axis / np.linalg.norm(axis), d / np.linalg.norm(d)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
    M[:3, 3] = shift * d
    return M


def moved(S, M: np.ndarray):
    """oracle.Settings of the camera M o w2c (camera-frame motion), its position recomputed; fp64 arrays (the fp32 paths round them)."""
    w = np.eye(4)
    w[:3, :4] = np.asarray(S.w2c, np.float64)[:3, :4]
    w = M @ w
    return dataclasses.replace(S, w2c=w, cam_position=-w[:3, :3].T @ w[:3, 3])


def pose_autograd_reference(params: dict, S, fwd: dict, gC, gA, gD, dtype=torch.float64, camera_leaves: bool = True, forward_only: bool = False) -> dict:
    """aux_autograd_reference with w2c[:3,:4] and cam_position as leaves: image, A, D, the six gradients and 'w2c' [3,4], 'cam' [3] of
    sum(gC image) + sum(gA A) + sum(gD D); `reached` [N]: Gaussians with a non-zero compositing weight somewhere; `xy` [N,2]: x/z, y/z of the means.
    dtype=torch.float32 evaluates the same graph in single precision (the conditioning precondition)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    P = {k: t(v).requires_grad_(True) for k, v in params.items()}
    means, scales, rots, opac = P['means'], P['scales'], P['rotations'], P['opacities'].reshape(-1)
    N = means.shape[0]
    sh0, sh_rest = P['sh0'].reshape(-1, 1, 3), P['sh_rest'].reshape(N, -1, 3)
    W, H = S.width, S.height
    w2c, cam, bg = t(S.w2c)[:3, :4].clone(), t(S.cam_position).reshape(1, 3).clone(), t(S.bg_color).reshape(3)
    if camera_leaves:
        w2c.requires_grad_(True)
        cam.requires_grad_(True)

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
    dx = mean2d[None, :, 0] - (xs.to(dtype) + 0.5)[:, None]
    dy = mean2d[None, :, 1] - (ys.to(dtype) + 0.5)[:, None]
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
    out = {'image': image.detach().numpy(), 'alpha': A.detach().numpy(), 'depth': D.detach().numpy()}
    reached = np.zeros(N, bool)
    reached[order.numpy()] = (w.detach() > 0).any(dim=0).numpy()
    xy = np.zeros((N, 2))
    xy[order.numpy()] = torch.stack([x, y], dim=1).detach().double().numpy()
    out.update(reached=reached, xy=xy, clip=(clip_l, clip_r, clip_t, clip_b))
    if forward_only:
        return out
    loss = (image * t(gC).reshape(3, H, W)).sum() + (A * t(gA).reshape(H, W)).sum() + (D * t(gD).reshape(H, W)).sum()
    loss.backward()
    for k, v in P.items():
        out[k] = v.grad.double().numpy() if v.grad is not None else np.zeros(tuple(v.shape))
    if camera_leaves:
        out['w2c'] = w2c.grad.double().numpy() if w2c.grad is not None else np.zeros((3, 4))
        out['cam'] = cam.grad.double().numpy().reshape(3) if cam.grad is not None else np.zeros(3)
    return out


def motion_of(name: str) -> np.ndarray:
    """The target camera of case `name`: the case's own, moved by 0.3 degrees and 0.2 % of the camera's distance to the scene (4 units)."""
    return rigid_motion(CASES[name][3], np.deg2rad(0.3), 0.008)


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """Scene, settings, oracle forward pass, flip mask and the upstream gradients of case `name` (zero on the flip pixels): once per process."""
    from oracle import oracle as O
    O.build()
    make, K, aa, _ = CASES[name]
    params, view = make()
    S, _ = helpers.settings_pair(view, K, aa)
    named = aux.named_params(params)
    f = O.forward(*helpers.np_params(params), S, bucket_size=64)
    H, W = view.height, view.width
    flips = helpers.flip_masks(O, f, S)['pixel']
    assert float(flips.mean()) <= MAX_ZEROED, (name, 'zeroed pixels', float(flips.mean()))
    here = pose_autograd_reference(named, S, f, None, None, None, forward_only=True)
    S2 = moved(S, motion_of(name))
    f2 = O.forward(*helpers.np_params(params), S2, bucket_size=64)
    there = pose_autograd_reference(named, S2, f2, None, None, None, forward_only=True)
    gC = ((here['image'] - there['image']) / (3 * H * W)).astype(np.float32)
    gA = ((here['alpha'] - there['alpha']) / (H * W)).astype(np.float32)
    gD = ((here['depth'] - there['depth']) / (H * W)).astype(np.float32)
    gC[:, flips] = 0.0
    gA[flips] = 0.0
    gD[flips] = 0.0
    assert np.abs(gC).max() > 0 and np.abs(gA).max() > 0 and np.abs(gD).max() > 0, name
    return {'name': name, 'params': params, 'named': named, 'view': view, 'K': K, 'aa': aa, 'S': S, 'f': f, 'keep': ~flips, 'gC': gC, 'gA': gA, 'gD': gD,
            'reached': here['reached'], 'xy': here['xy'], 'clip': here['clip']}


@functools.lru_cache(maxsize=None)
def reference(name: str, maps: bool = True, dtype=torch.float64) -> dict:
    """The reference of case `name` for (gC, gA, gD) (maps=True) or for gC alone: once per process, shared, read-only."""
    c = case(name)
    z = 0.0 if not maps else 1.0
    return pose_autograd_reference(c['named'], c['S'], c['f'], c['gC'], z * c['gA'], z * c['gD'], dtype=dtype)


def settings_of(c: dict, device='cpu'):
    return helpers.settings_pair(c['view'], c['K'], c['aa'], device=device)[1]


def run(be, c: dict, gC, gA, gD, device='cpu', res=None, entry: str = 'pose', **kw) -> dict:
    """forward (forward_aux when a map gradient is given) + one backward entry of the backend -- 'pose': backward_pose, 'aux': backward_aux -- numpy
    gradients under helpers.GRAD_KEYS and, for 'pose', 'w2c' [3,4] / 'cam' [3] (None if not asked for). kw: out, the block flag arrays, w2c=, cam_position=."""
    RS = settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    if res is None:
        res = be.forward_aux(*p, RS) if (gA is not None or gD is not None) else be.forward(*p, RS)
    dev = lambda g: None if g is None else torch.as_tensor(g).to(device)
    depth = getattr(res, 'depth', None)
    fn = be.backward_pose if entry == 'pose' else be.backward_aux
    got = fn(None, dev(gC), dev(gA), dev(gD), res.image, depth, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state, **kw)
    out = {'res': res, 'tensors': got}
    out.update({k: g.cpu().numpy() for k, g in zip(helpers.GRAD_KEYS, got[:6])})
    if entry == 'pose':
        out.update({k: (g.cpu().numpy() if g is not None else None) for k, g in zip(CAMERA_KEYS, got[6:])})
    return out


def check_camera_gradients(be, name: str, device='cpu') -> dict:
    """Check 1 for one case: the 15 camera gradients against fp64, with gA = gD = 0 and with all three upstream gradients; printed, then held to the bar."""
    c = case(name)
    report = {'zeroed': float((~c['keep']).mean())}
    for maps in (False, True):
        ref = reference(name, maps)
        out = run(be, c, c['gC'], c['gA'] if maps else None, c['gD'] if maps else None, device)
        for k in CAMERA_KEYS:
            report[f'{k}{"_maps" if maps else ""}'] = helpers.rel_inf(out[k], ref[k])
    print('pose', name, device, report)
    assert report['zeroed'] <= MAX_ZEROED, (name, report)
    for k, v in report.items():
        assert k == 'zeroed' or v < GRAD_TOL, (name, k, report)
    return report


def garden_60k():
    """The 60 001-Gaussian garden-like configuration of tests/test_sim_parity.py (640 x 360), at active_sh_bases = 1: 938 wave partials, 235 workgroups."""
    from harness.scenes import make_garden_like, orbit_views
    params = make_garden_like(60_001)
    params['scales'] = params['scales'] + 0.7
    return params, orbit_views(8, width=640, height=360, focal=473.0)[1]


def check_translation_identity(be, device='cpu') -> dict:
    """Check 6, reference-free: with one SH basis the colour does not see the camera position, so grad_means[i] = W^T dL/dp_i and
    grad_w2c[:,3] = sum_i dL/dp_i = W sum_i grad_means[i] (W a rotation). Allowed error per component: 1e-5 * sum_i |grad_means[i]|_1 -- a rounding
    bound, not a measurement: a 64-term fp32 wave sum in any order plus the 3 x 3 product is under 80 unit roundoffs of 2^-24 = 4.8e-6 of the absolute
    sum (the sum over the waves and the right-hand side are fp64), rounded up."""
    params, view = garden_60k()
    _, RS = helpers.settings_pair(view, 1, False, device=device)
    p = [params[k].to(device) for k in helpers.NAMES]
    res = be.forward(*p, RS)
    H, W = view.height, view.width
    gC = ((res.image - 0.5) / (3 * H * W)).contiguous()            # smooth and deterministic; the identity holds for any upstream gradient
    got = be.backward_pose(None, gC, None, None, res.image, None, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
    gm = got[0].double().cpu().numpy()
    Wr = view.w2c.double().numpy()[:3, :3]
    assert np.abs(Wr @ Wr.T - np.eye(3)).max() < 1e-6
    rhs = Wr @ gm.sum(axis=0)
    lhs = got[6].double().cpu().numpy()[:, 3]
    allowed = 1e-5 * np.abs(gm).sum()
    report = {'lines': (gm.shape[0] + 63) // 64, 'lhs': lhs.tolist(), 'rhs': rhs.tolist(), 'error': np.abs(lhs - rhs).tolist(), 'allowed': float(allowed),
              'cam': got[7].cpu().numpy().tolist()}
    print('pose identity', device, report)
    assert report['lines'] > 900 and np.abs(rhs).max() > 0
    assert np.all(np.abs(lhs - rhs) <= allowed), report
    assert not got[7].any()                                         # one SH basis: exactly zero
    return report


def same(a, b, exact: bool, tol: float = 1e-5) -> bool:
    """Bit for bit on the simulation (one thread order), rel_inf < 1e-5 on the device, where only the order of K11's atomics differs between two runs."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.array_equal(a, b)) if exact else helpers.rel_inf(a, b) < tol


def check_parameter_gradients_unchanged(be, name: str, device='cpu', exact: bool = True) -> None:
    """Check 2: on the same buffers the six gradients (and both flag arrays) of fgs_backward_pose are fgs_backward_reached's; with both camera outputs
    NULL the entry is fgs_backward_recycled."""
    c = case(name)
    n = c['f']['N']
    flags = lambda: {k: torch.full(((n + 63) // 64,), 7, dtype=torch.uint8, device=device) for k in ('live_blocks', 'reached_blocks')}
    fa, fp, fn = flags(), flags(), flags()
    plain = run(be, c, c['gC'], c['gA'], c['gD'], device, entry='aux', **fa)
    pose = run(be, c, c['gC'], c['gA'], c['gD'], device, res=plain['res'], **fp)
    none = run(be, c, c['gC'], c['gA'], c['gD'], device, res=plain['res'], w2c=False, cam_position=False, **fn)
    assert none['w2c'] is None and none['cam'] is None and pose['w2c'].shape == (3, 4) and pose['cam'].shape == (3,)
    only_cam = run(be, c, c['gC'], c['gA'], c['gD'], device, res=plain['res'], w2c=False)
    assert only_cam['w2c'] is None and same(only_cam['cam'], pose['cam'], exact), name
    for k in helpers.GRAD_KEYS:
        assert same(pose[k], plain[k], exact), (name, k, helpers.rel_inf(pose[k], plain[k]))
        assert same(none[k], plain[k], exact), (name, k)
    for k in fa:
        assert torch.equal(fa[k], fp[k]) and torch.equal(fa[k], fn[k]) and int(fa[k].max()) <= 1, (name, k)


def hidden_blocks_case() -> dict:
    """s0 with its first 128 Gaussians behind the camera: two blocks of K12 that reach nothing (the recycled path's early return) in front of 14 that do."""
    c = dict(case('s0'))
    c['params'] = {k: v.clone() for k, v in c['params'].items()}
    c['params']['means'][:128, 2] = -10.0
    return c


def check_recycled_path(be, device='cpu', exact: bool = True) -> None:
    """Check 3: with valid prior_blocks -- the gradient tensors and reached flags of an earlier pass -- the camera gradients are those of the unrecycled
    call; the two unreached blocks take K12's early return behind the store of their (zero) partials."""
    c = hidden_blocks_case()
    n = c['params']['means'].shape[0]
    flag = lambda: torch.full(((n + 63) // 64,), 7, dtype=torch.uint8, device=device)
    fresh = run(be, c, c['gC'], None, None, device)
    first_flags, second_flags = flag(), flag()
    first = run(be, c, c['gC'], None, None, device, reached_blocks=first_flags)
    assert first_flags[:2].tolist() == [0, 0] and int(first_flags[2:].min()) == 1
    again = run(be, c, 2.0 * c['gC'], None, None, device, out=first['tensors'][:6], reached_blocks=second_flags, prior_blocks=first_flags)
    twice = run(be, c, 2.0 * c['gC'], None, None, device)
    assert torch.equal(first_flags, second_flags)
    for k in CAMERA_KEYS:
        assert same(first[k], fresh[k], exact) and same(again[k], twice[k], exact), k
        assert np.abs(fresh[k]).max() > 0
    for k in helpers.GRAD_KEYS:
        assert same(again[k], twice[k], exact), k


def persistent_scratch(be, fill=None):
    """A Backend whose pose scratch is ONE buffer that survives the calls (and starts as `fill` bytes)."""
    _lib, _backend = helpers.backend_modules()

    class Persistent(_backend.Backend):
        kept = None

        def _scratch_pose(self, n, settings, device):
            t = super()._scratch_pose(n, settings, device)
            if self.kept is None or self.kept.numel() != t.numel() or self.kept.device != t.device:
                self.kept = t if fill is None else t.fill_(fill)
            return self.kept
    return Persistent(be.lib)


def check_scratch_independence(be, name: str = 'partial_tiles', device='cpu', exact: bool = True) -> None:
    """Check 4: a pass on scratch full of 0xFF bytes gives the clean result, and a second pass on the SAME scratch with all upstream gradients zero
    returns 15 values equal to 0.0f (every line of the partials is rewritten, a wave that reached nothing writes zeros)."""
    c = case(name)
    clean = run(be, c, c['gC'], c['gA'], c['gD'], device)
    kept = persistent_scratch(be, fill=255)
    dirty = run(kept, c, c['gC'], c['gA'], c['gD'], device)
    for k in CAMERA_KEYS:
        assert same(dirty[k], clean[k], exact), k
    scratch = kept.kept
    zero = run(kept, c, 0.0 * c['gC'], 0.0 * c['gA'], 0.0 * c['gD'], device, res=dirty['res'])
    assert kept.kept is scratch
    assert zero['w2c'].shape == (3, 4) and not zero['w2c'].any() and not zero['cam'].any()


def check_degenerate_inputs(be, device='cpu') -> None:
    """Check 5: n = 0 -> 15 zeros; one SH basis -> grad_cam_position exactly 0; a depth-only loss -> grad_cam_position exactly 0, row 2 of grad_w2c not."""
    c = case('partial_tiles')
    RS = settings_of(c, device)
    empty = [c['params'][k][:0].contiguous().to(device) for k in helpers.NAMES]
    for aux_forward in (False, True):
        res = be.forward_aux(*empty, RS) if aux_forward else be.forward(*empty, RS)
        ones = torch.ones_like(res.image)
        maps = (torch.ones_like(res.alpha), torch.ones_like(res.depth)) if aux_forward else (None, None)
        got = be.backward_pose(None, ones, *maps, res.image, getattr(res, 'depth', None), empty[0], empty[1], empty[2], empty[3], empty[5], res.buffers, RS, res.state)
        assert all(g.shape[0] == 0 for g in got[:6]) and got[6].shape == (3, 4) and got[7].shape == (3,)
        assert not got[6].any() and not got[7].any()
    st = case('stacked')
    assert st['K'] == 1
    one_basis = run(be, st, st['gC'], st['gA'], st['gD'], device)
    assert not one_basis['cam'].any() and np.abs(one_basis['w2c']).max() > 0
    depth_only = run(be, c, 0.0 * c['gC'], None, c['gD'], device)
    assert not depth_only['cam'].any() and np.abs(depth_only['w2c'][2]).max() > 0
    ref = pose_autograd_reference(c['named'], c['S'], c['f'], 0.0 * c['gC'], 0.0 * c['gA'], c['gD'])
    assert helpers.rel_inf(depth_only['w2c'], ref['w2c']) < GRAD_TOL and not ref['cam'].any()


def check_public_operator(B, be, device) -> None:
    """Check 7: diff_rasterize_pose against the backend (`be` is the backend the operator runs on) -- leaf w2c / cam_position, the composed chain with
    cam_position=None, a [4,4] w2c, camera inputs without requires_grad, a second backward over a retained graph."""
    c = case('partial_tiles')
    RS = settings_of(c, device)
    gC, gA, gD = (torch.as_tensor(c[k]).to(device) for k in ('gC', 'gA', 'gD'))
    leaves = lambda: [c['params'][k].to(device).requires_grad_(True) for k in helpers.NAMES]
    direct = run(be, c, c['gC'], c['gA'], c['gD'], device)
    direct_rgb = run(be, c, c['gC'], None, None, device)
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    near = lambda a, b: helpers.rel_inf(host(a), host(b)) < 1e-5        # two runs differ by the order of K11's atomics only
    w34 = RS.w2c[:3, :4].clone().requires_grad_(True)
    cam = RS.cam_position.clone().requires_grad_(True)

    # leaves, all three outputs; a retained graph differentiated twice
    p = leaves()
    image, alpha, depth = B.diff_rasterize_pose(*p, torch.empty(0), RS, w2c=w34, cam_position=cam, alpha=True, depth=True)
    assert image.shape == (3, c['view'].height, c['view'].width) and alpha.shape == depth.shape == image.shape[1:]
    loss = (image * gC).sum() + (alpha * gA).sum() + (depth * gD).sum()
    first = torch.autograd.grad(loss, p + [w34, cam], retain_graph=True)
    second = torch.autograd.grad(loss, p + [w34, cam])
    for k, g1, g2 in zip(helpers.GRAD_KEYS + CAMERA_KEYS, first, second):
        assert near(g1, direct[k]) and near(g2, g1), k
    assert first[6].shape == (3, 4) and first[7].shape == (3,)

    # colour only, a [4,4] w2c: no map is requested, the last row gets zeros
    w44 = torch.eye(4, device=device)
    w44[:3] = RS.w2c[:3, :4]
    w44.requires_grad_(True)
    p = leaves()
    image, alpha, depth = B.diff_rasterize_pose(*p, torch.empty(0), RS, w2c=w44, cam_position=cam)
    assert alpha is None and depth is None
    g44, gcam = torch.autograd.grad((image * gC).sum(), [w44, cam])
    assert g44.shape == (4, 4) and not g44[3].any() and near(g44[:3], direct_rgb['w2c']) and near(gcam, direct_rgb['cam'])

    # cam_position=None: derived as -W^T t, the chain is autograd's. dc/dW[i,j] = -t_i e_j, dc/dt = -W: grad_W -= t gc^T, grad_t -= W gc
    w = w44.detach().clone().requires_grad_(True)
    image, _, _ = B.diff_rasterize_pose(*leaves(), torch.empty(0), RS, w2c=w)
    (composed,) = torch.autograd.grad((image * gC).sum(), [w])
    derived = settings_of(c, device)._replace(cam_position=(-w.detach()[:3, :3].T @ w.detach()[:3, 3]))
    split = be.backward_pose(None, gC, None, None, *_forward_for(be, c, derived, device))
    gw, gc = split[6].double().cpu(), split[7].double().cpu()
    W_, t_ = w.detach().double().cpu()[:3, :3], w.detach().double().cpu()[:3, 3]
    by_hand = gw.clone()
    by_hand[:, :3] -= t_[:, None] * gc[None, :]
    by_hand[:, 3] -= W_ @ gc
    assert near(composed[:3], by_hand.numpy()) and not composed[3].any()

    # camera inputs that do not require grad: diff_rasterize's (diff_rasterize_aux's) gradients, no camera gradient, no POSE kernel
    p = leaves()
    image, _, _ = B.diff_rasterize_pose(*p, torch.empty(0), RS, w2c=RS.w2c, cam_position=RS.cam_position)
    quiet = torch.autograd.grad((image * gC).sum(), p)
    p = leaves()
    plain = torch.autograd.grad((B.diff_rasterize(*p, torch.empty(0), RS) * gC).sum(), p)
    for k, g, q in zip(helpers.GRAD_KEYS, quiet, plain):
        assert helpers.rel_inf(g.cpu().numpy(), q.cpu().numpy()) < 1e-6, k
    p = leaves()
    image, alpha, depth = B.diff_rasterize_pose(*p, torch.empty(0), RS, alpha=True, depth=True)
    quiet = torch.autograd.grad((image * gC).sum() + (alpha * gA).sum() + (depth * gD).sum(), p)
    p = leaves()
    image, alpha, depth = B.diff_rasterize_aux(*p, torch.empty(0), RS)
    plain = torch.autograd.grad((image * gC).sum() + (alpha * gA).sum() + (depth * gD).sum(), p)
    for k, g, q in zip(helpers.GRAD_KEYS, quiet, plain):
        assert helpers.rel_inf(g.cpu().numpy(), q.cpu().numpy()) < 1e-5, k
    with torch.no_grad():
        assert not B.diff_rasterize_pose(*leaves(), torch.empty(0), RS, w2c=w34, cam_position=cam)[0].requires_grad


def _forward_for(be, c: dict, RS, device) -> tuple:
    """The positional tail of backward_pose behind the map gradients for a plain forward pass of case `c` under settings RS."""
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    res = be.forward(*p, RS)
    return (res.image, None, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)


def check_refinement(device, steps: int, lr: float = 2e-3) -> dict:
    """Check 8: make_s0(n=1000) at its own size, the target rendered at the true camera; refine_pose starts a degree and 1 % of the camera's distance
    (0.04 of 4 units) off and must lower the rotation error, the translation error and the image L1. (steps, lr) were picked on the simulation:
    30 steps at 2e-3 take the angle from 1.0 to 0.3 degrees, the position error from 0.040 to 0.016 and the L1 from 0.043 to 0.003."""
    import FasterGSCudaBackend as B
    from harness import pose as P_
    from harness import trainer as T
    params, view = make_s0(n=1000)
    view = view.to(device)
    g = T.Gaussians(params, device)
    settings = T.extract_settings(view, g.active_sh_bases, view.background_color)
    with torch.no_grad():
        target = B.diff_rasterize_pose(*[t.detach() for t in g.tensors()], torch.empty(0), settings)[0]
    w0 = torch.tensor(rigid_motion(3, np.deg2rad(1.0), 0.04) @ view.w2c.double().cpu().numpy(), dtype=torch.float32, device=device)
    start = dataclasses.replace(view, w2c=w0, position=-w0[:3, :3].T @ w0[:3, 3])
    delta, losses = P_.refine_pose(g, start, target, steps=steps, lr=lr)
    with torch.no_grad():
        w1, c1 = delta(start.w2c)
        final = float((B.diff_rasterize_pose(*[t.detach() for t in g.tensors()], torch.empty(0), settings, w2c=w1, cam_position=c1)[0] - target).abs().mean())
    before, after = P_.pose_error(start.w2c, view.w2c), P_.pose_error(w1, view.w2c)
    report = {'angle': (before[0], after[0]), 'position': (before[1], after[1]), 'l1': (losses[0], final), 'steps': steps, 'lr': lr}
    print('pose refinement', device, report)
    assert all(np.isfinite(losses))
    assert after[0] < before[0] and after[1] < before[1] and final < losses[0], report
    return report
