"""Scenes and checks shared by tests/test_unreached.py (CPU simulation) and tests/test_gpu_unreached.py (MI355X): the backward gradients kernel and the
fused backward + Adam kernel skip VISIBLE Gaussians whose accumulator record K11 never added to (csrc/preprocess_backward.hip: gaussian_backward).

wall_scene(): 1 483 Gaussians (23 blocks of 64 + 11) at 128 x 128 behind the s0 camera. Indices 0 .. 719 are a wall of five layers of 12 x 12 nearly opaque
Gaussians two units in front of the camera: every pixel's transmittance falls below 1e-4 inside it. Index-contiguous runs around it:
  768 ..  831  a whole block behind the wall, inside the frustum: visible, unreached
  832 ..  895  a block alternating small Gaussians in FRONT of the wall (reached) and Gaussians behind it (unreached)
  896 ..  959  a block behind the camera (invisible)
  960 .. 1199  small faint Gaussians in front of the wall
 1200 .. 1482  behind the wall; the ragged last wave (1472 .. 1482) is visible and unreached
"Reached" is read off the oracle: any of the nine per-Gaussian sums of oracle.backward non-zero. case() asserts that the scene produces every one of
these situations and fails otherwise."""
from __future__ import annotations

import functools

import numpy as np
import torch

import helpers
from harness.scenes import View, make_s0

N_WALL, N = 720, 1483
UNREACHED_BLOCK, MIXED_BLOCK, BEHIND_CAMERA_BLOCK = 12, 13, 14
ORDER = ('means', 'sh_coefficients_0', 'sh_coefficients_rest', 'opacities', 'scales', 'rotations')      # optimizer-group order (Model.py:238-245)
GRAD_OF = {'means': 'means', 'sh_coefficients_0': 'sh0', 'sh_coefficients_rest': 'sh_rest', 'opacities': 'opacities', 'scales': 'scales', 'rotations': 'rotations'}
LRS = [1.6e-4, 2.5e-3, 1.25e-4, 2.5e-2, 5e-3, 1e-3]
TOL = 1e-4                               # the suite's bar: max-abs error relative to the tensor's max-abs value


def _logit(x):
    return torch.log(x) - torch.log1p(-x)


def wall_scene(seed: int = 41):
    p, view = make_s0(seed=seed, n=N)                       # camera at z = -4 looking down +z, focal 128: the frustum is |x|, |y| < depth / 2
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    idx = torch.arange(N)
    # the wall: layer l at depth 2 + 0.05 l, a 12 x 12 grid over [-1.15, 1.15]^2 (the frustum there is [-1, 1]^2), sigma 0.16 = 10 px at a pitch of 13 px
    w = idx[:N_WALL]
    layer, cell = w // 144, w % 144
    grid = torch.linspace(-1.15, 1.15, 12)
    p['means'][:N_WALL, 0] = grid[cell % 12] + 0.02 * (layer % 2)
    p['means'][:N_WALL, 1] = grid[cell // 12] + 0.02 * (layer % 2)
    p['means'][:N_WALL, 2] = -2.0 + 0.05 * layer + 1e-4 * cell                     # distinct depth keys
    p['scales'][:N_WALL] = float(np.log(0.16))
    p['opacities'][:N_WALL] = 5.0
    front = torch.zeros(N, dtype=torch.bool)
    front[MIXED_BLOCK * 64:(MIXED_BLOCK + 1) * 64:2] = True
    front[960:1200] = True
    behind = ~front
    behind[:N_WALL] = False
    nf, nb = int(front.sum()), int(behind.sum())
    p['means'][front] = torch.stack([0.9 * u(nf) - 0.45, 0.9 * u(nf) - 0.45, -3.0 + 0.3 * u(nf)], 1)       # depth 1 .. 1.3
    p['scales'][front] = torch.log(0.015 + 0.02 * u(nf, 3))
    p['opacities'][front] = _logit(0.2 + 0.5 * u(nf, 1))
    p['means'][behind] = torch.stack([3.0 * u(nb) - 1.5, 3.0 * u(nb) - 1.5, 0.2 + 0.8 * u(nb)], 1)         # depth 4.2 .. 5
    p['means'][BEHIND_CAMERA_BLOCK * 64:(BEHIND_CAMERA_BLOCK + 1) * 64, 2] = -10.0
    return {k: v.contiguous() for k, v in p.items()}, view


def hot_scene(seed: int = 43):
    """288 x 204 (18 x 17 tiles): Gaussian 0 is large and semi-transparent, its footprint covers more than 256 tiles -- K11 adds its sums into the replicas of a
    hot slot and the fold in front of K12 completes its record; six small Gaussians sit in front of it."""
    p, v = make_s0(seed=seed, n=7)
    p['means'][0] = torch.tensor([0.03, -0.02, 0.0])
    p['scales'][0] = torch.log(torch.tensor([1.6, 1.2, 1.4]))          # anisotropic: an isotropic Gaussian's rotation gradient is zero up to rounding
    p['opacities'][0] = float(_logit(torch.tensor(0.4)))
    p['means'][1:, 2] = -1.0 - 0.1 * torch.arange(6)
    p['means'][1:, :2] *= 0.8
    return p, View(v.w2c, v.position, 288, 204, 200.0, 200.0, 144.0, 102.0, 0.2, 1e4, torch.zeros(3))


def records_of(g: dict, n: int) -> np.ndarray:
    """The nine sums K11 leaves per Gaussian, from oracle.backward: mean2d 2, conic 3, opacity 1, colour 3."""
    return np.concatenate([g['_grad_mean2d'].reshape(n, 2), g['_grad_conic'].T.reshape(n, 3), g['_grad_opacity_acc'].reshape(n, 1),
                           g['_grad_color_acc'].reshape(n, 3)], axis=1)


def blocks_of(mask: np.ndarray) -> np.ndarray:
    return np.concatenate([mask, np.zeros((-mask.size) % 64, bool)]).reshape(-1, 64)


@functools.lru_cache(maxsize=None)
def case() -> dict:
    """The wall scene, its oracle forward / backward pass and the classes of its Gaussians: once per process, shared, read-only."""
    from oracle import oracle as O
    O.build()
    params, view = wall_scene()
    S, _ = helpers.settings_pair(view)
    f = O.forward(*helpers.np_params(params), S, bucket_size=64)
    gi = (np.random.default_rng(5).standard_normal(f['image'].shape) / f['image'].size).astype(np.float32)
    dens = np.zeros((2, N), np.float32)
    g = O.backward(f, S, gi, dens)
    visible = f['n_touched'] > 0
    reached = visible & (records_of(g, N) != 0).any(axis=1)
    unreached = visible & ~reached
    # ---- the scene's premises ----
    assert N % 64 != 0
    assert float(f['final_T'].max()) < 1e-4, 'some pixel is not closed'
    idx = np.arange(N)
    front = ((idx // 64 == MIXED_BLOCK) & (idx % 2 == 0)) | ((idx >= 960) & (idx < 1200))
    assert not reached[(idx >= N_WALL) & ~front].any(), 'a Gaussian behind the wall was reached: the wall does not close every pixel'
    vb, rb = blocks_of(visible), blocks_of(reached)
    assert vb[UNREACHED_BLOCK].all() and not rb[UNREACHED_BLOCK].any(), 'no block that is entirely visible and unreached'
    lanes = np.arange(64)
    assert vb[MIXED_BLOCK].all() and rb[MIXED_BLOCK][lanes % 2 == 0].sum() >= 16 and not rb[MIXED_BLOCK][lanes % 2 == 1].any(), 'no mixed block'
    assert not vb[BEHIND_CAMERA_BLOCK].any(), 'no invisible block'
    assert rb[:288 // 64].all(), 'the front two layers of the wall (whole blocks 0 .. 3) are not all reached'        # deeper layers: reached where the front left light
    assert vb[-1][:N % 64].all() and not rb[-1].any(), 'the ragged last wave is not visible and unreached'
    assert unreached.sum() > 300 and reached.sum() > 300
    return {'params': params, 'view': view, 'S': S, 'f': f, 'gi': gi, 'g': g, 'dens': dens, 'visible': visible, 'reached': reached, 'unreached': unreached}


def may_flip(c: dict, dec: dict | None) -> tuple[np.ndarray, int]:
    """Hardware only: the Gaussians whose "reached" state may legitimately differ between the device and the oracle, and the number of pixels that can cause it.
    A pixel whose transmittance lands within 1e-5 (relative) of the 1e-4 termination test, or that owns a pair within 5e-6 of the alpha test, may be walked a
    Gaussian or two further (or less far) on the device than in the oracle. The oracle names such pixels (helpers.flip_masks); every Gaussian whose screen box
    contains one is a candidate. In this scene every pixel lies inside the boxes of some fifty unreached Gaussians, so the candidates are many even for two or
    three pixels; what is bounded is the number of Gaussians that really differ (check_backward), not the number of candidates."""
    from oracle import oracle as O
    out = np.zeros(N, bool)
    if dec is None:
        return out, 0
    risk = helpers.flip_masks(O, c['f'], c['S'], dec)
    out |= risk['prim']
    sb = c['f']['screen_bounds'].astype(np.int64)
    for y, x in zip(*np.nonzero(risk['pixel'])):
        out |= (sb[:, 0] <= x) & (x < sb[:, 1]) & (sb[:, 2] <= y) & (y < sb[:, 3])
    return out, int(risk['pixel'].sum())


def check_backward(be, device: str) -> dict:
    """Gradients against the oracle at the suite's bar, exact zeros for unreached Gaussians, both densification statistics, the live-block flags.
    "Unreached" is checked in two steps, so that no Gaussian escapes the `== 0` check: (1) K11's records are read back from the primitive blob; every visible
    Gaussian whose record is all +-0 there must have gradient rows that are exactly zero and an unchanged second statistic -- no exclusions; (2) the set the
    device reached equals the oracle's. On hardware it may differ by the Gaussians a borderline pixel walks further or less far (may_flip): each one that
    differs must be such a candidate, and there may be at most three per borderline pixel (a walk that continues past a transmittance of 1e-4 ends again with
    the next one or two contributors). In the simulation the two sets are equal."""
    c = case()
    view, f, g = c['view'], c['f'], c['g']
    _, RS = helpers.settings_pair(view, device=device)
    dp = {k: v.to(device) for k, v in c['params'].items()}
    res = be.forward(*[dp[k] for k in helpers.NAMES], RS)
    dec = helpers.decode_forward(be, res, N, view.width, view.height)
    assert np.array_equal(dec['n_touched'] > 0, c['visible'])
    dens0 = torch.stack([torch.full((N,), 3.0), torch.full((N,), 0.25)]).to(device)
    dens = dens0.clone()
    flags = torch.full(((N + 63) // 64,), 7, dtype=torch.uint8, device=device)
    grads = be.backward(dens, torch.from_numpy(c['gi']).to(device), res.image, dp['means'], dp['scales'], dp['rotations'], dp['opacities'],
                        dp['sh_coefficients_rest'], res.buffers, RS, res.state, live_blocks=flags)
    grads = {k: t.cpu().numpy().reshape(g[k].shape) for k, t in zip(helpers.GRAD_KEYS, grads)}
    report = {k: helpers.rel_inf(grads[k], g[k]) for k in helpers.GRAD_KEYS}
    acc = be.view(res.buffers[0].cpu(), be.blob_layout(0, N, view.width, view.height, res.state[1], res.state[2]), 'acc', torch.float32)[:9 * N].reshape(N, 9).numpy()
    reached_dev = c['visible'] & ((acc.view(np.uint32) & 0x7fffffff) != 0).any(axis=1)
    differ = reached_dev != c['reached']
    candidates, risk_pixels = may_flip(c, dec if device != 'cpu' else None)
    report.update(reached_differs=int(differ.sum()), borderline_pixels=risk_pixels, unexplained=int((differ & ~candidates).sum()))
    print('unreached', device, report)
    for k in helpers.GRAD_KEYS:
        assert report[k] < TOL, (k, report)
    assert report['unexplained'] == 0 and report['reached_differs'] <= 3 * risk_pixels, report
    rows = c['visible'] & ~reached_dev
    assert rows.sum() >= c['unreached'].sum() - 3 * risk_pixels
    for k in helpers.GRAD_KEYS:
        assert not grads[k][rows].any(), (k, 'non-zero gradient of an unreached Gaussian')
        assert np.abs(grads[k][reached_dev]).max() > 0, k
    d = dens.cpu().numpy()
    assert np.array_equal(d[0], np.where(c['visible'], 4.0, 3.0).astype(np.float32)), 'densification_info[0] counts the VISIBLE Gaussians'
    assert np.array_equal(d[1][rows], np.full(int(rows.sum()), 0.25, np.float32)), 'densification_info[1] of an unreached Gaussian moved'
    assert np.array_equal(d[1][~c['visible']], np.full(int((~c['visible']).sum()), 0.25, np.float32))
    assert helpers.rel_inf(d[1] - 0.25, c['dens'][1]) < TOL
    assert np.array_equal(flags.cpu().numpy(), blocks_of(c['visible']).any(axis=1).astype(np.uint8)), 'live_blocks is "any visible Gaussian in the block"'
    return report


def check_hot(be, oracle, device: str) -> dict:
    """The record of a Gaussian with more than 256 tiles arrives through the hot replicas: a reached test in front of the fold would see zeros."""
    params, view = hot_scene()
    S, RS = helpers.settings_pair(view, device=device)
    f = oracle.forward(*helpers.np_params(params), S, bucket_size=64)
    assert f['n_touched'][0] > 256 and (f['n_touched'][1:] > 0).sum() >= 3 and f['n_touched'][1:].max() <= 256, f['n_touched']
    gi = (np.random.default_rng(6).standard_normal(f['image'].shape) / f['image'].size).astype(np.float32)
    g = oracle.backward(f, S, gi, np.zeros((2, 7), np.float32))
    dp = {k: v.to(device) for k, v in params.items()}
    res = be.forward(*[dp[k] for k in helpers.NAMES], RS)
    grads = be.backward(None, torch.from_numpy(gi).to(device), res.image, dp['means'], dp['scales'], dp['rotations'], dp['opacities'],
                        dp['sh_coefficients_rest'], res.buffers, RS, res.state)
    report = {}
    for k, t in zip(helpers.GRAD_KEYS, grads):
        a = t.cpu().numpy().reshape(g[k].shape)
        report[k] = helpers.rel_inf(a, g[k])
        assert np.abs(g[k][0]).max() > 0 and np.abs(a[0]).max() > 0, (k, 'the hot Gaussian has no gradient')
        report[k + '_hot'] = helpers.rel_inf(a[0], g[k][0])
    print('hot', device, report)
    assert max(report.values()) < TOL, report
    return report


def check_optimizers(be, device: str, monkeypatch, steps: int = 2) -> dict:
    """backward + FusedAdam.step and FusedRasterizerOptimizer, two iterations each, against the same steps fed from the oracle's gradients (the fused suite's
    bars: the step each parameter took and both moments to 1e-4 of their max-abs value, fewer than max(1e-4, two rows) of the entries beyond 1e-4 of their
    own magnitude). Moments start non-zero, so in the second step an unreached Gaussian moves on momentum alone."""
    import FasterGSCudaBackend as FGS
    from FasterGSCudaBackend import adam as A, fused as F, rasterization as R
    from oracle import oracle as O
    if device == 'cpu':                                # the public operators refuse CPU tensors: point them at the simulation
        monkeypatch.setattr(R, '_require_gpu', lambda t: None)
        for module in (R, A, F):
            monkeypatch.setattr(module, 'default_backend', lambda: be)
    c = case()
    view, S = c['view'], c['S']
    _, RS = helpers.settings_pair(view, device=device)
    gi = torch.from_numpy(c['gi']).to(device)
    P0 = {k: c['params'][k].clone() for k in ORDER}
    MV0 = {k: helpers.seeded_moments(P0[k].shape, 31 + i) for i, k in enumerate(ORDER)}

    # the oracle's two steps
    oP = {k: np.ascontiguousarray(P0[k].numpy().copy()) for k in ORDER}
    oM = {k: np.ascontiguousarray(MV0[k][0].numpy().copy()) for k in ORDER}
    oV = {k: np.ascontiguousarray(MV0[k][1].numpy().copy()) for k in ORDER}
    never_reached = np.ones(N, bool)
    for step in range(1, steps + 1):
        f = O.forward(*[oP[k] for k in helpers.NAMES], S, bucket_size=64)
        g = O.backward(f, S, c['gi'], np.zeros((2, N), np.float32))
        never_reached &= (f['n_touched'] > 0) & ~(records_of(g, N) != 0).any(axis=1)
        for k, lr in zip(ORDER, LRS):
            O.adam_step(np.ascontiguousarray(g[GRAD_OF[k]].reshape(oP[k].shape)), oP[k], oM[k], oV[k], step, lr)
    assert never_reached.sum() > 300

    def via_fused_adam():
        P = {k: P0[k].to(device).clone().requires_grad_(True) for k in ORDER}
        opt = FGS.FusedAdam([{'params': [P[k]], 'lr': lr, 'name': k} for k, lr in zip(ORDER, LRS)], lr=0.0, eps=1e-15)
        for k in ORDER:
            opt.state[P[k]] = {'step': 0, 'exp_avg': MV0[k][0].to(device).clone(), 'exp_avg_sq': MV0[k][1].to(device).clone()}
        for _ in range(steps):
            image = FGS.diff_rasterize(P['means'], P['scales'], P['rotations'], P['opacities'], P['sh_coefficients_0'], P['sh_coefficients_rest'],
                                       torch.empty(0, device=device), RS)
            (image * gi).sum().backward()
            opt.step()
            opt.zero_grad()
        return ({k: P[k].detach().cpu().numpy() for k in ORDER}, {k: opt.state[P[k]]['exp_avg'].cpu().numpy() for k in ORDER},
                {k: opt.state[P[k]]['exp_avg_sq'].cpu().numpy() for k in ORDER})

    def via_fused_kernel():
        opt = FGS.FusedRasterizerOptimizer([P0[k].to(device).clone() for k in ORDER], LRS)
        opt.exp_avg = [MV0[k][0].to(device).clone() for k in ORDER]
        opt.exp_avg_sq = [MV0[k][1].to(device).clone() for k in ORDER]
        for _ in range(steps):
            opt.render_and_step(RS, lambda image: gi)
        return tuple({k: t.cpu().numpy() for k, t in zip(ORDER, ts)} for ts in (opt.params, opt.exp_avg, opt.exp_avg_sq))

    report = {}
    for name, run in (('FusedAdam', via_fused_adam), ('FusedRasterizerOptimizer', via_fused_kernel)):
        dP, dM, dV = run()
        for k in ORDER:
            start = P0[k].numpy()
            moved_ref, moved = oP[k] - start, dP[k] - start
            fig = (helpers.rel_inf(moved, moved_ref), helpers.rel_inf(dM[k], oM[k]), helpers.rel_inf(dV[k], oV[k]))
            elem = (helpers.elementwise_fraction(moved, moved_ref), helpers.elementwise_fraction(dM[k], oM[k]), helpers.elementwise_fraction(dV[k], oV[k]))
            report[name, k] = fig + elem
        print('optimizers', device, name, {k: report[name, k] for k in ORDER})
        for k in ORDER:
            assert max(report[name, k][:3]) < TOL, (name, k, report[name, k])
            assert max(report[name, k][3:]) < max(helpers.ELEM_FRACTION, 2.0 * oP[k][0].size / oP[k].size), (name, k, 'element-wise 1e-4', report[name, k])
        # momentum alone: a zero gradient twice -> exp_avg = m0 * 0.9 * 0.9 (fp32), and the parameter moved
        m0 = MV0['means'][0].numpy()
        assert np.abs(dM['means'][never_reached] - m0[never_reached] * 0.9 ** steps).max() < 1e-5 * np.abs(m0).max(), name
        assert np.abs(dP['means'][never_reached] - P0['means'].numpy()[never_reached]).max(axis=1).min() > 0, name
    return report


def check_depth_only(be, device: str) -> dict:
    """Depth-supervised pass with grad_image = 0: the colour sums of every record are zero, the others and dL/dz are not. Against the fp64 reference of
    tests/aux_grad_cases.py at its bar; every Gaussian the reference gives a gradient keeps one."""
    import aux_grad_cases as cases
    c = cases.case('partial_tiles')
    ref = depth_only_reference()
    out = cases.run(be, c, np.zeros_like(c['gC']), None, c['gD'], device)
    report = {k: helpers.rel_inf(out[k], np.asarray(ref[k]).reshape(out[k].shape)) for k in ('means', 'scales', 'rotations', 'opacities')}
    print('depth only', device, report)
    assert max(report.values()) < cases.GRAD_TOL, report
    assert not out['sh0'].any() and not out['sh_rest'].any()
    n = out['means'].shape[0]
    contributes = np.abs(np.asarray(ref['means']).reshape(n, 3)).max(axis=1) > 1e-3 * np.abs(ref['means']).max()
    assert contributes.sum() > 50 and (np.abs(out['means'][contributes]).max(axis=1) > 0).all()
    return report


@functools.lru_cache(maxsize=None)
def depth_only_reference() -> dict:
    import aux_grad_cases as cases
    c = cases.case('partial_tiles')
    return cases.aux_autograd_reference(cases.named_params(c['params']), c['S'], c['f'], 0.0 * c['gC'], 0.0 * c['gA'], c['gD'])
