"""Scenes, fp64 reference and comparisons shared by tests/test_geometry.py (CPU simulation) and tests/test_gpu_geometry.py (MI355X): the training render
that returns the depth-distortion map X and the blend M of five per-Gaussian surface channels from ONE extra walk, differentiably (fgs_blend_geometry /
fgs_backward_geometry, diff_rasterize_geometry, render_image_training_geometry, training_iteration(geometry_render=True)).

Scenes: aux_grad_cases.case(name), all four, in both modes of the distortion term; `stacked` walks tile lists of more than three 192-entry batches
(check_long_lists asserts it). normal_cases.small_scene / disk_patch for the composed checks.
Reference: feature_cases._graph(name) (weights w, blend order, leaves) with t of distortion_cases._t_of, X = distortion_cases.distortion_abs(w, t) and
M = (w @ F).T; the loss is sum(gC image) + sum(gX X) + sum(gM M) with aux_grad_cases' gC, distortion_cases.grad_map (gX) and feature_cases.grad_map(name, 5)
(gM), all zero on the flip pixels, and feature_cases.features(name, 5) (any sign -- channel 4 does NOT hold ones, so X may not lean on it). It is pinned
twice (check_reference_pins): gM = 0 gives distortion_cases.reference, gX = 0 gives feature_cases.reference(name, 5), both to 1e-12.

Bars, none derived from the kernels' output: aux_grad_cases.MAP_TOL (1e-4) for maps on the kept pixels, GRAD_TOL (1e-4) for each gradient tensor
(helpers.rel_inf against fp64), RERUN_TOL = 1e-5 between two runs of one pass (the order of the float atomics is the only difference) and between the
operator and the backend, normal_cases.OPERATOR_TOL_SIM (1e-5) for compositions -- the 1e-5 that tests/test_gpu_normal_consistency.py passes to
check_operators on the device is the same number. The restatement figures of distortion_cases' docstring (the prefix arithmetic in fp32: at most 7.3e-7
beside the colour term, 8.8e-7 alone) and the fp32 dot of five products (a few 1e-7) say why those bars are within reach of one walk carrying both."""
from __future__ import annotations

import functools

import numpy as np
import torch

import aux_grad_cases as aux
import distortion_cases
import feature_cases
import helpers
import normal_cases
from harness.scenes import View

MAP_TOL, GRAD_TOL = aux.MAP_TOL, aux.GRAD_TOL
RERUN_TOL = 1e-5
MODES = distortion_cases.MODES
PARITY = [(name, mode) for name in aux.CASES for mode in MODES]
ALONE = distortion_cases.ALONE
GEO_KEYS = ('means', 'scales', 'rotations', 'opacities')
ALL_KEYS = helpers.GRAD_KEYS + ('features',)
F = 5


def features(name: str) -> np.ndarray:
    return feature_cases.features(name, F)


def grad_x(name: str) -> np.ndarray:
    return distortion_cases.grad_map(name)


def grad_m(name: str) -> np.ndarray:
    return feature_cases.grad_map(name, F)


def surface_features(be, c: dict, device='cpu') -> torch.Tensor:
    """The real surface features of the case's Gaussians for its camera (fgs_surface_features): channel 4 holds ones."""
    p, v = c['params'], c['view']
    f = be.surface_features(p['means'].to(device), p['scales'].to(device), p['rotations'].to(device), v.w2c.to(device), v.position.to(device))
    assert bool((f[:, 4] == 1).all())
    return f


# ---- the fp64 reference -----------------------------------------------------------------------------------------------------------------------------------
def geometry_autograd_reference(name: str, mode: str, feats: np.ndarray, gC, gX, gM) -> dict:
    """fp64 image, X ('map'), M ('surface'), the six gradients and grad_surface_features ('features') of sum(gC image) + sum(gX X) + sum(gM M)."""
    G = feature_cases._graph(name)
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    H, W = G['H'], G['W']
    Fe = t64(feats).requires_grad_(True)
    X = distortion_cases.distortion_abs(G['w'], distortion_cases._t_of(name, mode)).reshape(H, W)
    M = (G['w'] @ Fe[G['order']]).T.reshape(F, H, W)
    loss = (G['image'] * t64(gC).reshape(3, H, W)).sum() + (X * t64(gX).reshape(H, W)).sum() + (M * t64(gM).reshape(F, H, W)).sum()
    leaves = list(G['P'].values()) + [Fe]
    grads = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    out = {'image': G['image'].detach().numpy(), 'map': X.detach().numpy(), 'surface': M.detach().numpy()}
    for (k, v), g in zip(list(G['P'].items()) + [('features', Fe)], grads):
        out[k] = g.numpy() if g is not None else np.zeros(tuple(v.shape))
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str, mode: str) -> dict:
    """The fp64 reference of (case, mode) for (gC, gX, gM) all present: once per process, shared, read-only."""
    return geometry_autograd_reference(name, mode, features(name), aux.case(name)['gC'], grad_x(name), grad_m(name))


def check_reference_pins(name: str) -> None:
    """gM = 0: the reference IS distortion_cases.reference (both modes); gX = 0: it IS feature_cases.reference(name, 5). To 1e-12."""
    c = aux.case(name)
    for mode in MODES:
        mine, theirs = geometry_autograd_reference(name, mode, features(name), c['gC'], grad_x(name), 0.0 * grad_m(name)), distortion_cases.reference(name, mode)
        assert np.abs(mine['image'] - theirs['image']).max() < 1e-12 and helpers.rel_inf(mine['map'], theirs['map']) < 1e-12, (name, mode)
        for k in helpers.GRAD_KEYS:
            assert helpers.rel_inf(mine[k], np.asarray(theirs[k]).reshape(mine[k].shape)) < 1e-12, (name, mode, k)
    mine, theirs = geometry_autograd_reference(name, 'linear', features(name), c['gC'], 0.0 * grad_x(name), grad_m(name)), feature_cases.reference(name, F)
    assert helpers.rel_inf(mine['surface'], theirs['map']) < 1e-12, name
    for k in ALL_KEYS:
        assert helpers.rel_inf(mine[k], np.asarray(theirs[k]).reshape(mine[k].shape)) < 1e-12, (name, k)


# ---- through the backend ----------------------------------------------------------------------------------------------------------------------------------
def run(be, c: dict, mode: str, feats, gC, gX, gM, device='cpu', res=None, RS=None) -> dict:
    """forward + blend_geometry + backward_geometry through the backend: numpy image, X ('map'), M ('surface'), the state, the six gradients under
    helpers.GRAD_KEYS and 'features' (None when neither map has a gradient)."""
    RS = aux.settings_of(c, device) if RS is None else RS
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    res = be.forward(*p, RS) if res is None else res
    normalized = mode == 'normalized'
    fe = torch.as_tensor(feats).to(device)
    state = be.blend_geometry(p[0], fe, res, p[0].shape[0], RS, normalized)
    dev = lambda g: None if g is None else torch.as_tensor(g).to(device)
    grads = be.backward_geometry(None, dev(gC), dev(gX), dev(gM), res.image, state, fe, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state, normalized)
    out = {'image': res.image.cpu().numpy(), 'map': state[0].cpu().numpy(), 'surface': state[2:7].cpu().numpy(), 'state': state, 'res': res}
    out.update({k: g.cpu().numpy() for k, g in zip(helpers.GRAD_KEYS, grads[:6])})
    out['features'] = None if grads[6] is None else grads[6].cpu().numpy()
    return out


def check_against_reference(be, name: str, mode: str, device='cpu', exact_image: bool = True) -> dict:
    """1. One (case, mode) end to end, all three upstream gradients present: X, the five planes of M, the image against plain `forward`, the six
    gradients and grad_surface_features against fp64, and a rerun; every figure is printed before it is held to its bar."""
    c, ref = aux.case(name), reference(name, mode)
    args = (be, c, mode, features(name), c['gC'], grad_x(name), grad_m(name), device)
    out, again = run(*args), run(*args)
    plain = aux.run_plain(be, c, c['gC'], device)
    keep = c['keep']
    report = {'zeroed': float((~keep).mean()), 'map': helpers.rel_inf(out['map'][keep], ref['map'][keep]),
              'image_vs_plain': float(np.abs(out['image'] - plain['image']).max()), 'map_rerun': helpers.rel_inf(again['map'], out['map']),
              'surface_rerun': helpers.rel_inf(again['surface'], out['surface'])}
    for ch in range(F):
        report[f'surface{ch}'] = helpers.rel_inf(out['surface'][ch][keep], ref['surface'][ch][keep])
    for k in ALL_KEYS:
        report[k] = helpers.rel_inf(out[k], np.asarray(ref[k]).reshape(out[k].shape))
        report[k + '_rerun'] = helpers.rel_inf(again[k], out[k])
    print(name, mode, device, report)
    n_processed = c['f']['n_processed'].reshape(keep.shape)
    assert not out['map'][n_processed < 2].any(), name                        # fewer than two Gaussians: X exactly 0
    assert not out['map'][n_processed == 0].any() and not out['surface'][:, n_processed == 0].any(), name     # nothing blended: zeros in all public planes
    assert np.isfinite(out['state'].cpu().numpy()).all() and float(np.abs(ref['map']).max()) > 0
    assert report['map'] < MAP_TOL, (name, mode, report)
    for ch in range(F):
        assert report[f'surface{ch}'] < MAP_TOL, (name, mode, ch, report)
    if exact_image:
        assert np.array_equal(out['image'], plain['image']), name
    else:
        assert helpers.rel_inf(out['image'], plain['image']) < MAP_TOL, (name, report)
    for k in ALL_KEYS:
        assert report[k] < GRAD_TOL, (name, mode, k, report)
        assert report[k + '_rerun'] < RERUN_TOL, (name, mode, k, report)
    assert report['map_rerun'] < RERUN_TOL and report['surface_rerun'] < RERUN_TOL, (name, mode, report)
    return report


def check_long_lists(be, device='cpu') -> None:
    """`stacked` walks lists longer than one 192-entry batch: the second staging of a tile is exercised by every check on it."""
    c = aux.case('stacked')
    RS = aux.settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    res = be.forward(*p, RS)
    dec = helpers.decode_forward(be, res, p[0].shape[0], c['view'].width, c['view'].height)
    assert int(dec['max_n_processed'].max()) > 192, int(dec['max_n_processed'].max())


def check_replaced_operators(be, name: str, mode: str, device='cpu', exact: bool = True) -> dict:
    """2. Against the operators it replaces, for real surface features (channel 4 all ones): plane 0 = blend_distortion's plane 0 and state[2:7] =
    blend_features (F = 5) -- bit for bit on the simulation, MAP_TOL on the device; the private planes hold what blend_distortion's hold; and by
    linearity the gradients for (gC, gX, gM) = backward_distortion(gC, gX) + backward_features(0, gM) within GRAD_TOL."""
    c = aux.case(name)
    RS = aux.settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    n, keep = p[0].shape[0], c['keep']
    normalized = mode == 'normalized'
    fe = surface_features(be, c, device)
    res = be.forward(*p, RS)
    state = be.blend_geometry(p[0], fe, res, n, RS, normalized)
    dstate = be.blend_distortion(p[0], res, n, RS, normalized)
    fmap = be.blend_features(fe, res, n, RS)
    assert state.shape == (8, c['view'].height, c['view'].width) and state[2:7].is_contiguous()
    if exact:
        assert torch.equal(state[0], dstate[0]) and torch.equal(state[2:7], fmap), (name, mode)
        assert torch.equal(state[7], dstate[1]) and torch.equal(state[1], dstate[2]) and torch.equal(state[6], state[7]), (name, mode)
    report = {'map': helpers.rel_inf(state[0].cpu().numpy()[keep], dstate[0].cpu().numpy()[keep]),
              'surface': helpers.rel_inf(state[2:7].cpu().numpy()[:, keep], fmap.cpu().numpy()[:, keep])}
    gC, gX, gM = (torch.as_tensor(g).to(device) for g in (c['gC'], grad_x(name), grad_m(name)))
    one = be.backward_geometry(None, gC, gX, gM, res.image, state, fe, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state, normalized)
    dist = be.backward_distortion(None, gC, gX, res.image, dstate, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state, normalized)
    feat = be.backward_features(None, torch.zeros_like(gC), gM, res.image, fmap, fe, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
    for k, g, a, b in zip(helpers.GRAD_KEYS, one[:6], dist, feat[:6]):
        report[k] = helpers.rel_inf(g.cpu().numpy(), (a + b).cpu().numpy())
    report['features'] = helpers.rel_inf(one[6].cpu().numpy(), feat[6].cpu().numpy())
    print('replaced operators', name, mode, device, report)
    assert report['map'] < MAP_TOL and report['surface'] < MAP_TOL, (name, mode, report)
    for k in ALL_KEYS:
        assert report[k] < GRAD_TOL, (name, mode, k, report)
    return report


def check_terms_alone(be, name: str, mode: str, device='cpu') -> dict:
    """3. gC = 0, gM = 0 (zeros, not None): distortion_cases.reference_alone at GRAD_TOL, SH gradients and grad_surface_features exactly 0. gX None:
    the feature reference. Both None: the plain pass within RERUN_TOL, no feature gradient."""
    c = aux.case(name)
    zero_c = np.zeros_like(c['gC'])
    ref = distortion_cases.reference_alone(name, mode)
    out = run(be, c, mode, features(name), zero_c, grad_x(name), np.zeros_like(grad_m(name)), device)
    report = {'x_' + k: helpers.rel_inf(out[k], np.asarray(ref[k]).reshape(out[k].shape)) for k in GEO_KEYS}
    assert not out['sh0'].any() and not out['sh_rest'].any() and not out['features'].any(), (name, mode)
    only_x = run(be, c, mode, features(name), zero_c, grad_x(name), None, device)
    assert not only_x['features'].any() and not only_x['sh0'].any()
    report.update({'x_none_' + k: helpers.rel_inf(only_x[k], np.asarray(ref[k]).reshape(only_x[k].shape)) for k in GEO_KEYS})
    fref = feature_cases.reference(name, F)
    only_m = run(be, c, mode, features(name), c['gC'], None, grad_m(name), device)
    report.update({'m_' + k: helpers.rel_inf(only_m[k], np.asarray(fref[k]).reshape(only_m[k].shape)) for k in ALL_KEYS})
    print('terms alone', name, mode, device, report)
    for k, figure in report.items():
        assert figure < GRAD_TOL, (name, mode, k, report)
    for k in GEO_KEYS:
        assert float(np.abs(ref[k]).max()) > 0
    plain = aux.run_plain(be, c, c['gC'], device)
    none = run(be, c, mode, features(name), c['gC'], None, None, device)
    assert none['features'] is None
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(none[k], plain[k]) < RERUN_TOL, ('neither map gradient', k)
    return report


def check_boundaries(be, device='cpu') -> None:
    """4. A second backward pass over retained buffers equals the first; poisoned scratch changes nothing; n = 0; an offset added to w2c[2, 3] leaves
    the linear X (and the planes of M, whose features are given) unchanged."""
    name, mode = 'hot', 'normalized'
    c = aux.case(name)
    args = (c, mode, features(name), c['gC'], grad_x(name), grad_m(name), device)
    first = run(be, *args)
    plain = aux.run_plain(be, c, c['gC'], device)
    second = run(be, *args, res=first['res'])
    for k in ALL_KEYS:
        assert helpers.rel_inf(second[k], first[k]) < RERUN_TOL, ('second pass', k)
    assert max(float(np.abs(first[k] - plain[k]).max()) for k in GEO_KEYS) > 0             # the terms are there
    dirty = run(helpers.poisoned(be), *args)
    for k in ('image', 'map', 'surface') + ALL_KEYS:
        assert helpers.rel_inf(dirty[k], first[k]) < RERUN_TOL, ('poisoned', k)

    for name in ('partial_tiles', 'stacked'):
        c = aux.case(name)
        RS = aux.settings_of(c, device)
        p = [c['params'][k].to(device) for k in helpers.NAMES]
        n, keep = p[0].shape[0], c['keep']
        fe = torch.as_tensor(features(name)).to(device)
        res = be.forward(*p, RS)
        state = be.blend_geometry(p[0], fe, res, n, RS, False).cpu().numpy()
        v = c['view']
        w2c = v.w2c.clone()
        w2c[2, 3] += 3.0
        moved = View(w2c, v.position, v.width, v.height, v.focal_x, v.focal_y, v.center_x, v.center_y, v.near_plane, v.far_plane, v.background_color)
        RS_moved = helpers.settings_pair(moved, c['K'], c['aa'], device=device)[1]
        shifted = be.blend_geometry(p[0], fe, res, n, RS_moved, False).cpu().numpy()
        report = {'offset': helpers.rel_inf(shifted[0][keep], state[0][keep]), 'surface': helpers.rel_inf(shifted[2:7], state[2:7])}
        print('offset', name, device, report)
        assert report['offset'] < MAP_TOL and report['surface'] == 0.0, (name, report)

    c = aux.case('partial_tiles')
    RS = aux.settings_of(c, device)
    H, W = c['view'].height, c['view'].width
    empty = [c['params'][k][:0].contiguous().to(device) for k in helpers.NAMES]
    r0 = be.forward(*empty, RS)
    f0 = torch.zeros((0, F), device=device)
    s0 = be.blend_geometry(empty[0], f0, r0, 0, RS)
    assert s0.shape == (8, H, W) and not s0.any()
    g0 = be.backward_geometry(None, torch.ones_like(r0.image), torch.ones_like(s0[0]), torch.ones_like(s0[2:7]), r0.image, s0, f0, empty[0], empty[1],
                              empty[2], empty[3], empty[5], r0.buffers, RS, r0.state)
    assert len(g0) == 7 and all(g.shape[0] == 0 for g in g0) and g0[6].shape == (0, F)


def check_refusals(be, device='cpu') -> None:
    """5. Every refusal through the backend, with its text."""
    import pytest
    name = 'partial_tiles'
    c = aux.case(name)
    RS = aux.settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    n = p[0].shape[0]
    total_rest = p[5].shape[1]
    res = be.forward(*p, RS)
    fe = torch.as_tensor(features(name)).to(device)
    gi, gX, gM = (torch.as_tensor(g).to(device) for g in (c['gC'], grad_x(name), grad_m(name)))
    state = be.blend_geometry(p[0], fe, res, n, RS)
    back = lambda st=state, gx=gX, gm=gM, r=res, settings=RS, f=fe: be.backward_geometry(None, gi, gx, gm, r.image, st, f, p[0], p[1], p[2], p[3], p[5],
                                                                                           r.buffers, settings, r.state)
    with pytest.raises(RuntimeError, match=r'means must be a contiguous float32 \[N, 3\]'):
        be.blend_geometry(p[0][:-1].contiguous(), fe, res, n, RS)
    for bad in (fe[:-1].contiguous(), fe[:, :4].contiguous(), torch.zeros((n, 6), device=device), fe.t().contiguous().t()):
        with pytest.raises(RuntimeError, match=r'surface_features must be a contiguous float32 \[N, 5\]'):
            be.blend_geometry(p[0], bad, res, n, RS)
        with pytest.raises(RuntimeError, match=r'surface_features must be a contiguous float32 \[N, 5\]'):
            back(f=bad)
    with pytest.raises(RuntimeError, match='grad_distortion must be'):
        back(gx=gX[:-1])
    with pytest.raises(RuntimeError, match='grad_surface_map must be'):
        back(gm=gM[:4])
    with pytest.raises(RuntimeError, match='geometry_state must be'):
        back(st=state[:7])
    v = c['view']
    for near, far in ((0.0, 10.0), (-1.0, 10.0), (2.0, 2.0), (2.0, 1.0)):
        bad = View(v.w2c, v.position, v.width, v.height, v.focal_x, v.focal_y, v.center_x, v.center_y, near, far, v.background_color)
        RS_bad = helpers.settings_pair(bad, c['K'], c['aa'], device=device)[1]
        with pytest.raises(RuntimeError, match='0 < near_plane < far_plane'):
            be.blend_geometry(p[0], fe, res, n, RS_bad)
        with pytest.raises(RuntimeError, match='0 < near_plane < far_plane'):
            back(settings=RS_bad)
        with pytest.raises(RuntimeError, match='0 < near_plane < far_plane'):
            back(settings=RS_bad, gx=None)                               # the mode is the state's: refused with the feature gradient alone as well
        be.blend_geometry(p[0], fe, res, n, RS_bad, False)
    asynchronous = be.forward(*p, RS, instance_capacity=1 << 20)
    with pytest.raises(RuntimeError, match='fgs_forward_async'):
        be.blend_geometry(p[0], fe, asynchronous, n, RS)
    with pytest.raises(RuntimeError, match='fgs_forward_async'):
        back(r=asynchronous)
    # the record path for real: one owner's K1, then the render from its splat records -- the state that pass returns is refused
    rec = torch.zeros((1, n, 56), dtype=torch.uint8, device=device)
    counts = torch.zeros((1, 2), dtype=torch.int32, device=device)
    be.shard_preprocess(*p, [RS], rec, counts)
    n_visible, n_instances = (int(x) for x in counts[0].cpu())
    assert n_visible > 0
    records = be.forward_from_records(rec.view(-1), n_visible, n_instances, RS, total_rest)
    head = lambda t: t[:n_visible].contiguous()
    with pytest.raises(RuntimeError, match='record'):
        be.blend_geometry(head(p[0]), head(fe), records, n_visible, RS)
    with pytest.raises(RuntimeError, match='record'):
        be.backward_geometry(None, gi, gX, gM, records.image, state, head(fe), head(p[0]), head(p[1]), head(p[2]), head(p[3]), head(p[5]), records.buffers,
                             RS, records.state)
    with pytest.raises(RuntimeError, match='takes no geometry gradient'):
        be.backward_adam_fused(None, gi, res.image, [], [], [], res.buffers, RS, res.state, 1, [], grad_geometry=gX)
    with pytest.raises(RuntimeError, match='takes no geometry gradient'):
        be.backward_to_records(gi, res.image, res.buffers, RS, res.state, 15, grad_geometry=gM)


def check_two_kernel_k12_is_refused(dev_be, device='cpu') -> None:
    """5. The dev option's two-kernel K12 (fgs_debug_set_option(3, 0), dev flavour only) is refused with its text, not ignored."""
    import pytest
    c = aux.case('partial_tiles')
    assert dev_be.lib.fgs_debug_set_option(3, 0) == 0
    try:
        with pytest.raises(RuntimeError, match='one-kernel K12 only'):
            run(dev_be, c, 'linear', features('partial_tiles'), c['gC'], grad_x('partial_tiles'), grad_m('partial_tiles'), device)
    finally:
        assert dev_be.lib.fgs_debug_set_option(3, 1) == 0


def check_abi_refusals(lib, _lib) -> None:
    """5. The C entry points refuse by themselves, before anything is launched; the ABI version stays 3."""
    import ctypes as C
    st = _lib.ForwardState()
    S = _lib.Settings(1, 1, 1, 16, 15, 128, 128, 1.0, 1.0, 0.0, 0.0, 0.2, 100.0, 0)
    blend = lambda means=1, feats=1, state=st, mode=1, out=1, settings=S: lib.fgs_blend_geometry(means, feats, 1, 1, 1, 10, C.byref(settings), C.byref(state),
                                                                                                   mode, out, None)
    back = lambda state=st, mode=1, feats=1, gstate=1, gx=1, gm=1, gf=1, settings=S: lib.fgs_backward_geometry(
        1, 1, None, None, None, *([1] * 17), 10, C.byref(settings), C.byref(state), None, None, feats, gstate, gx, gm, gf, mode, None)     # no alpha / depth gradient
    for call in (blend, back):
        for bad in (2, -1):
            assert call(mode=bad) == -1 and b'distortion mode' in lib.fgs_last_error()
        for near, far in ((0.0, 100.0), (5.0, 5.0), (5.0, 1.0)):
            planes = _lib.Settings(1, 1, 1, 16, 15, 128, 128, 1.0, 1.0, 0.0, 0.0, near, far, 0)
            assert call(settings=planes) == -1 and b'0 < near_plane < far_plane' in lib.fgs_last_error()
        for bit, text in ((4, b'fgs_forward_async'), (8, b'record')):
            assert call(state=_lib.ForwardState(0, 0, 0, bit)) == -1 and text in lib.fgs_last_error()
    assert blend(out=None) == -1 and b'NULL geometry_state' in lib.fgs_last_error()
    assert blend(means=None) == -1 and b'NULL means' in lib.fgs_last_error()
    assert blend(feats=None) == -1 and b'NULL surface_features' in lib.fgs_last_error()
    assert back(gstate=None) == -1 and b'NULL geometry_state' in lib.fgs_last_error()
    assert back(gx=None, gstate=None) == -1 and b'NULL geometry_state' in lib.fgs_last_error()     # one upstream gradient is enough to be the geometry pass
    assert back(feats=None) == -1 and b'NULL surface_features' in lib.fgs_last_error()
    assert back(gf=None) == -1 and b'grad_surface_features' in lib.fgs_last_error()
    assert lib.fgs_abi_version() == 3


# ---- 6. the public operator -------------------------------------------------------------------------------------------------------------------------------
def check_operator(B, be, name: str, device='cpu') -> None:
    """B.diff_rasterize_geometry against the backend `be` it runs on: outputs and the seven gradients equal to the backend's in both modes, a second
    backward over the retained graph, non-contiguous gX and gM, each output unused in turn, features that do not require grad, torch.no_grad()."""
    import pytest
    c = aux.case(name)
    RS = aux.settings_of(c, device)
    gC, gX, gM = (torch.as_tensor(g).to(device) for g in (c['gC'], grad_x(name), grad_m(name)))
    f = features(name)
    leaves_of = lambda: [c['params'][k].to(device).clone().requires_grad_(True) for k in helpers.NAMES]
    feats_of = lambda grad=True: torch.as_tensor(f).to(device).clone().requires_grad_(grad)
    none = torch.empty(0)
    close = lambda got, want, what: [_assert_close(g, want[k], (what, k)) for k, g in zip(ALL_KEYS, got)]
    for mode in MODES:
        direct = run(be, c, mode, f, c['gC'], gX, gM, device)
        leaves, fe = leaves_of(), feats_of()
        image, dmap, smap = B.diff_rasterize_geometry(*leaves, none, RS, fe, normalized=mode == 'normalized')
        assert image.shape == (3, c['view'].height, c['view'].width) and dmap.shape == image.shape[1:] and smap.shape == (F,) + image.shape[1:]
        assert torch.equal(image.detach().cpu(), torch.as_tensor(direct['image'])) and torch.equal(dmap.detach().cpu(), torch.as_tensor(direct['map']))
        assert torch.equal(smap.detach().cpu(), torch.as_tensor(direct['surface']))
        loss = (image * gC).sum() + (dmap * gX).sum() + (smap * gM).sum()
        first = torch.autograd.grad(loss, leaves + [fe], retain_graph=True)
        second = torch.autograd.grad(loss, leaves + [fe])
        close(first, direct, mode)
        close(second, {k: g.cpu().numpy() for k, g in zip(ALL_KEYS, first)}, mode + ' retained')
    direct = run(be, c, 'normalized', f, c['gC'], gX, gM, device)

    # non-contiguous incoming gradients are made contiguous; the default mode is the normalized one; features without requires_grad get no gradient
    leaves, fe = leaves_of(), feats_of(False)
    image, dmap, smap = B.diff_rasterize_geometry(*leaves, none, RS, fe)
    gX_t, gM_t = gX.t().contiguous().t(), gM.transpose(1, 2).contiguous().transpose(1, 2)
    assert not gX_t.is_contiguous() and not gM_t.is_contiguous()
    close(torch.autograd.grad((image * gC).sum() + (dmap * gX_t).sum() + (smap * gM_t).sum(), leaves), direct, 'strided')

    # each output unused in turn: the backend's pass with that gradient None (the image's arrives as None and is passed on as zeros)
    zero_c = np.zeros_like(c['gC'])
    for what, (uc, ux, um) in {'no image': (False, True, True), 'no distortion': (True, False, True), 'no surface map': (True, True, False)}.items():
        leaves, fe = leaves_of(), feats_of()
        image, dmap, smap = B.diff_rasterize_geometry(*leaves, none, RS, fe)
        loss = sum(term for used, term in ((uc, (image * gC).sum()), (ux, (dmap * gX).sum()), (um, (smap * gM).sum())) if used)
        got = torch.autograd.grad(loss, leaves + [fe], allow_unused=True)
        want = run(be, c, 'normalized', f, c['gC'] if uc else zero_c, gX if ux else None, gM if um else None, device)
        close(got[:6], want, what)
        _assert_close(got[6], want['features'], (what, 'features'))
        if not um:
            assert not got[6].any()
    # neither map in the loss: the plain pass, and the features get no gradient
    leaves, fe = leaves_of(), feats_of()
    image, _, _ = B.diff_rasterize_geometry(*leaves, none, RS, fe)
    unused = torch.autograd.grad((image * gC).sum(), leaves + [fe], allow_unused=True)
    assert unused[6] is None
    leaves = leaves_of()
    plain = torch.autograd.grad((B.diff_rasterize(*leaves, none, RS) * gC).sum(), leaves)
    for k, g, q in zip(helpers.GRAD_KEYS, unused, plain):
        assert helpers.rel_inf(g.cpu().numpy(), q.cpu().numpy()) < RERUN_TOL, k

    with torch.no_grad():
        image, dmap, smap = B.diff_rasterize_geometry(*leaves_of(), none, RS, feats_of(False))
    assert not dmap.requires_grad and not smap.requires_grad
    assert torch.equal(dmap.cpu(), torch.as_tensor(direct['map'])) and torch.equal(smap.cpu(), torch.as_tensor(direct['surface']))
    with pytest.raises(RuntimeError, match=r'surface_features must be a contiguous float32 \[N, 5\]'):
        B.diff_rasterize_geometry(*leaves_of(), none, RS, feats_of(False)[:-1])


def _assert_close(got, want, what) -> None:
    figure = helpers.rel_inf(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want)
    assert figure < RERUN_TOL, (what, figure)


# ---- 7. the composed graph --------------------------------------------------------------------------------------------------------------------------------
COMPOSED_WEIGHTS = (1.0, 1.0, 0.1)      # a, b, c of a X.mean() + b E.mean() + c depth_l1


def check_composed(B, device='cpu', tol: float = normal_cases.OPERATOR_TOL_SIM, min_alpha: float = 0.3) -> dict:
    """a X.mean() + b normal_consistency(M).mean() + c depth_l1_loss(M[4], M[3], target) on normal_cases.small_scene: the gradients through the ONE
    render equal those of the same loss assembled from diff_rasterize_distortion, diff_rasterize_features and normal_consistency."""
    T, params, view = normal_cases.small_scene(device)
    RS = T.extract_settings(view, 16, view.background_color)
    none = torch.empty(0)
    a, b, c = COMPOSED_WEIGHTS
    with torch.no_grad():
        g0 = [params[k].to(device) for k in helpers.NAMES]
        feats = B.gaussian_surface_features(g0[0], g0[1], g0[2], view.w2c, view.position)
        _, _, M0 = B.diff_rasterize_geometry(*g0, none, RS, feats)
        target = torch.where(M0[4] > 0.5, 1.1 * M0[3] / M0[4].clamp_min(1e-8), torch.zeros_like(M0[3]))
    assert float((target > 0).float().mean()) > 0.1

    def loss_of(X, M):
        E = B.normal_consistency(M, RS, min_alpha=min_alpha)
        terms = (X.mean(), E.mean(), T.depth_l1_loss(M[4], M[3], target))
        return a * terms[0] + b * terms[1] + c * terms[2], [float(t.detach()) for t in terms]

    def one_render(leaves):
        feats = B.gaussian_surface_features(leaves[0], leaves[1], leaves[2], view.w2c, view.position)
        _, X, M = B.diff_rasterize_geometry(*leaves, none, RS, feats)
        return X, M

    def two_renders(leaves):
        feats = B.gaussian_surface_features(leaves[0], leaves[1], leaves[2], view.w2c, view.position)
        _, X = B.diff_rasterize_distortion(*leaves, none, RS)
        _, M = B.diff_rasterize_features(*leaves, none, RS, feats)
        return X, M

    results = []
    for render in (one_render, two_renders):
        leaves = [params[k].to(device).clone().requires_grad_(True) for k in helpers.NAMES]
        loss, terms = loss_of(*render(leaves))
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
        results.append((float(loss.detach()), terms, [torch.zeros_like(p) if g is None else g for p, g in zip(leaves, grads)]))
    (loss1, terms1, g1), (loss2, terms2, g2) = results
    errs = {k: helpers.rel_inf(x.cpu().numpy(), y.cpu().numpy()) for k, x, y in zip(helpers.GRAD_KEYS[:4], g1, g2)}
    errs['loss'] = abs(loss1 - loss2) / abs(loss2)
    print(f'composed graph on {device}: terms {terms1}, rel_inf of the one render against the two {errs}')
    assert all(t > 0 and np.isfinite(t) for t in terms1)
    assert all(float(g.abs().max()) > 0 for g in g1[:4]) and not g1[4].any() and not g1[5].any()
    assert max(errs.values()) < tol, errs
    return errs


# ---- 8. the harness ---------------------------------------------------------------------------------------------------------------------------------------
HARNESS_WEIGHTS = {'distortion_weight': 10.0, 'normal_weight': 0.05, 'depth_weight': 0.5}


def check_training_iteration(device='cpu', min_alpha: float = 0.3) -> None:
    """geometry_render=True with all three weights: the first loss is the plain first loss plus the three terms, each evaluated under no_grad (rtol
    1e-4); three steps stay finite and update densification_info; the default is the plain iteration; without the flag the old ValueErrors still
    fire, with the flag and absgrad it raises."""
    import pytest
    T, params, view = normal_cases.small_scene(device)
    dev = torch.device(device)
    truth = T.Gaussians(params, dev)
    with torch.no_grad():
        target = T.render_image_training(truth, view, False, view.background_color).clone()
        _, X, E, alpha, depth = T.render_image_training_geometry(truth, view, False, view.background_color, min_alpha=min_alpha)
        depth_target = torch.where(alpha > 0.5, 1.1 * depth / alpha.clamp_min(1e-8), torch.zeros_like(depth))
        terms = (float(X.mean()), float(E.mean()), float(T.depth_l1_loss(alpha, depth, depth_target)))
    assert X.shape == E.shape == alpha.shape == depth.shape == (view.height, view.width) and all(t > 0 for t in terms), terms
    w = HARNESS_WEIGHTS
    expected = w['distortion_weight'] * terms[0] + w['normal_weight'] * terms[1] + w['depth_weight'] * terms[2]

    def first_loss(**kw):
        g = T.Gaussians({k: v.clone() for k, v in params.items()}, dev)
        g.training_setup(training_cameras_extent=4.0)
        losses = [float(T.training_iteration(g, view, target, it, **kw)) for it in range(3)]
        assert all(np.isfinite(losses)), losses
        return losses[0], g
    plain, _ = first_loss()
    default, _ = first_loss(geometry_render=False)
    flag_only, _ = first_loss(geometry_render=True)
    with_terms, g = first_loss(geometry_render=True, depth_target=depth_target, normal_min_alpha=min_alpha, **w)
    print(f'harness on {device}: plain {plain}, with the three terms {with_terms}, terms {terms}')
    assert default == plain
    assert abs(flag_only - plain) <= 1e-4 * abs(plain)
    assert abs((with_terms - plain) - expected) <= 1e-4 * (abs(plain) + expected), (with_terms, plain, expected)
    assert g.densification_info[0].max() > 0 and all(bool(torch.isfinite(getattr(g, k)).all()) for k in T.PARAM_ORDER)
    with pytest.raises(ValueError, match='distortion term does not combine with depth supervision or absgrad in one render'):
        T.training_iteration(g, view, target, 3, distortion_weight=1.0, depth_target=depth_target, depth_weight=1.0)
    with pytest.raises(ValueError, match='normal-consistency term does not combine with the distortion term, depth supervision or absgrad in one render'):
        T.training_iteration(g, view, target, 3, normal_weight=1.0, distortion_weight=1.0)
    with pytest.raises(ValueError, match='does not combine'):
        T.training_iteration(g, view, target, 3, geometry_render=True, absgrad=True, **w)


# ---- 9. it regularises ------------------------------------------------------------------------------------------------------------------------------------
def check_regularises(device='cpu', steps: int = 30, lr: float = 5e-3) -> tuple:
    """Perturbed flat disks: `steps` Adam steps on X.mean() + E.mean() alone, over means, scales, rotations and opacities, through the one render."""
    T, _, view = normal_cases.small_scene(device)
    g = T.Gaussians(normal_cases.disk_patch(), torch.device(device))
    opt = torch.optim.Adam([g.means, g.scales, g.rotations, g.opacities], lr=lr)
    history = []
    for _ in range(steps + 1):
        _, X, E, _, _ = T.render_image_training_geometry(g, view, False, view.background_color)
        loss = X.mean() + E.mean()
        history.append((float(X.detach().mean()), float(E.detach().mean())))
        if len(history) > steps:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f'geometry terms on {device}: (X.mean(), E.mean()) {history[0]} -> {history[-1]} in {steps} steps')
    assert all(np.isfinite(x) and np.isfinite(e) for x, e in history) and sum(history[0]) > 0
    assert sum(history[-1]) < sum(history[0]), (history[0], history[-1])
    return history[0], history[-1]
