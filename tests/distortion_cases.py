"""Scenes, fp64 reference and comparisons shared by tests/test_distortion.py (CPU simulation) and tests/test_gpu_distortion.py (MI355X): the training
render that also returns the depth-distortion map X(p) = sum_a sum_b w_a w_b |t_a - t_b| differentiably (fgs_blend_distortion /
fgs_backward_distortion, diff_rasterize_distortion).

Scenes: aux_grad_cases.case(name), all four, in both modes ('linear': t = z; 'normalized': t = far (z - near) / ((far - near) z)).
Reference: the fp64 autograd graph of feature_cases._graph (weights w, blend order, leaves) with t computed in double from the leaves and X written as the
explicit double sum with the absolute value, chunked over pixels. It is pinned twice (check_reference_pins): with gX = 0 it reproduces
aux_grad_cases.reference_rgb to 1e-12, and the prefix form 2 sum_i w_i (t_i A_{i-1} - D_{i-1}) equals the absolute-value form to 1e-12, which is also the
check that t is ordered along the walk. Upstream gradients: aux_grad_cases' gC, and a seeded normal gX / (H W), zero on the flip pixels like gC.

Bars: aux_grad_cases.MAP_TOL (1e-4) for the map on the kept pixels, GRAD_TOL (1e-4) for each gradient tensor (helpers.rel_inf against fp64), 1e-5 between
two runs of one pass. X is a difference of products, so before the kernels were held to those bars the SAME prefix formulas were evaluated in fp32 torch
on the CPU (restatement_figures: w rounded to fp32, t - t0 of the tile formed in fp32 as the kernels form it, exclusive fp32 cumsums, X, e_i and dX/dt_i
in fp32; e_i and dX/dt_i then go through the fp64 graph, so what is measured is the fp32 prefix arithmetic alone). rel_inf against the fp64 reference:

    case          mode        map      means    scales   rotations opacities  (sh0, sh_rest: 0, the term does not reach them)
    s0            linear      2.2e-07  1.6e-07  6.4e-07  2.9e-07   3.3e-07
    s0            normalized  2.5e-07  1.5e-08  1.5e-08  8.6e-09   1.1e-08
    partial_tiles linear      2.5e-07  1.8e-07  1.5e-07  4.9e-07   2.7e-07
    partial_tiles normalized  2.6e-07  1.2e-08  1.2e-08  1.2e-08   1.4e-08
    stacked       linear      1.7e-07  5.7e-07  4.5e-07  1.9e-07   1.2e-07
    stacked       normalized  2.1e-07  1.3e-08  9.2e-09  4.2e-09   7.1e-09
    hot           linear      2.6e-07  1.2e-07  5.9e-07  3.2e-07   7.3e-07
    hot           normalized  2.8e-07  2.1e-08  3.8e-08  2.1e-08   4.6e-08

(the gradients are those of sum(gC image) + sum(gX X); in normalized mode t spans a small part of [0, 1) on these scenes, X is small beside the
colour term and its error smaller still). The largest figure is 7.3e-7: none uses more than half of its bar (5e-5), so every bar stays the
project's. ALONE (check_term_alone) holds the six gradients of sum(gX X) by itself, gC = 0, to GRAD_TOL as well, so that the term is not judged beside
a larger one; its restatement figures (means, scales, rotations, opacities): partial_tiles linear 2.5e-07 1.9e-07 6.1e-07 3.2e-07, normalized 3.8e-07
2.6e-07 4.7e-07 4.6e-07; stacked linear 8.8e-07 3.1e-07 3.2e-07 1.1e-07, normalized 6.7e-07 2.7e-07 2.7e-07 1.5e-07. The bars are not derived from
the kernels' output."""
from __future__ import annotations

import functools

import numpy as np
import torch

import aux_grad_cases as aux
import feature_cases
import helpers
from harness.scenes import View

MAP_TOL, GRAD_TOL = aux.MAP_TOL, aux.GRAD_TOL
RERUN_TOL = 1e-5
MODES = ('linear', 'normalized')
PARITY = [(name, mode) for name in aux.CASES for mode in MODES]
ALONE = [(name, mode) for name in ('partial_tiles', 'stacked') for mode in MODES]
CHUNK = 4096                            # pixels per piece of the explicit double sum


def grad_map(name: str) -> np.ndarray:
    """gX [H,W] float32: seeded normal / (H W), zero on the flip pixels."""
    c = aux.case(name)
    H, W = c['view'].height, c['view'].width
    g = (np.random.default_rng(31).standard_normal((H, W)) / (H * W)).astype(np.float32)
    g[~c['keep']] = 0.0
    return g


def depth_values(c: dict, z: torch.Tensor, mode: str) -> torch.Tensor:
    """t of view-space depths z in the dtype of z."""
    if mode == 'linear':
        return z
    near, far = float(c['view'].near_plane), float(c['view'].far_plane)
    return far * (z - near) / ((far - near) * z)


def _t_of(name: str, mode: str) -> torch.Tensor:
    """t per Gaussian of the blend order [V], in double, differentiable in the means leaf of the case's graph."""
    c, G = aux.case(name), feature_cases._graph(name)
    w2c = torch.tensor(np.asarray(c['S'].w2c), dtype=torch.float64)
    m = G['P']['means'][G['order']]
    return depth_values(c, m @ w2c[2, :3] + w2c[2, 3], mode)


def distortion_abs(w: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """X [P] = sum_a sum_b w_a w_b |t_a - t_b|, the double sum written out, a piece of pixels at a time."""
    M = (t[:, None] - t[None, :]).abs()
    return torch.cat([((w[k:k + CHUNK] @ M) * w[k:k + CHUNK]).sum(dim=1) for k in range(0, w.shape[0], CHUNK)])


def distortion_prefix(w: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """X [P] = 2 sum_i w_i (t_i A_{i-1} - D_{i-1}) in the dtype of w."""
    zero = torch.zeros_like(w[:, :1])
    A = torch.cat([zero, torch.cumsum(w, dim=1)[:, :-1]], dim=1)
    D = torch.cat([zero, torch.cumsum(w * t[None, :], dim=1)[:, :-1]], dim=1)
    return 2.0 * (w * (t[None, :] * A - D)).sum(dim=1)


def distortion_autograd_reference(name: str, mode: str, gC: np.ndarray, gX: np.ndarray) -> dict:
    """fp64 image, map and the six gradients of sum(gC image) + sum(gX X)."""
    G = feature_cases._graph(name)
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    H, W = G['H'], G['W']
    X = distortion_abs(G['w'], _t_of(name, mode)).reshape(H, W)
    loss = (G['image'] * t64(gC).reshape(3, H, W)).sum() + (X * t64(gX).reshape(H, W)).sum()
    grads = torch.autograd.grad(loss, list(G['P'].values()), retain_graph=True, allow_unused=True)
    out = {'image': G['image'].detach().numpy(), 'map': X.detach().numpy()}
    for (k, v), g in zip(G['P'].items(), grads):
        out[k] = g.numpy() if g is not None else np.zeros(tuple(v.shape))
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str, mode: str) -> dict:
    """The fp64 reference of (case, mode) for aux_grad_cases' gC and this module's gX: once per process, shared, read-only."""
    return distortion_autograd_reference(name, mode, aux.case(name)['gC'], grad_map(name))


@functools.lru_cache(maxsize=None)
def reference_alone(name: str, mode: str) -> dict:
    """... and for gX alone (gC = 0): the gradients of the distortion term by itself."""
    return distortion_autograd_reference(name, mode, 0.0 * aux.case(name)['gC'], grad_map(name))


def check_reference_pins(name: str) -> None:
    """gX = 0: the reference IS aux_grad_cases.reference_rgb; and the prefix form equals the absolute-value form in both modes (t is ordered)."""
    c, G = aux.case(name), feature_cases._graph(name)
    mine = distortion_autograd_reference(name, 'linear', c['gC'], 0.0 * grad_map(name))
    theirs = aux.reference_rgb(name)
    assert np.abs(mine['image'] - theirs['image']).max() < 1e-12
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(mine[k], np.asarray(theirs[k]).reshape(mine[k].shape)) < 1e-12, (name, k)
    with torch.no_grad():
        for mode in MODES:
            t = _t_of(name, mode)
            figure = helpers.rel_inf(distortion_prefix(G['w'], t).numpy(), distortion_abs(G['w'], t).numpy())
            print(name, mode, 'prefix vs absolute value', figure)
            assert figure < 1e-12, (name, mode, figure)


def _tile_origin_rank(name: str) -> torch.Tensor:
    """Per pixel: the position in the blend order of the first entry of its tile's list (0 for a tile with an empty list)."""
    c, G = aux.case(name), feature_cases._graph(name)
    fwd, H, W = c['f'], G['H'], G['W']
    gw, gh = fwd['grid']
    rank = torch.full((G['N'],), -1, dtype=torch.int64)
    rank[G['order']] = torch.arange(G['order'].numel())
    first = torch.full((gw * gh,), G['order'].numel(), dtype=torch.int64)
    first.scatter_reduce_(0, torch.tensor(fwd['inst_keys'].astype(np.int64)), rank[torch.tensor(fwd['inst_prims'].astype(np.int64))], reduce='amin')
    first[first == G['order'].numel()] = 0
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    return first[((ys // 12) * gw + (xs // 16)).reshape(-1)]


def restatement_figures(name: str, mode: str, with_image: bool = True) -> dict:
    """The prefix formulas of the kernels in fp32 torch on the CPU against the fp64 reference: rel_inf of the map and of the six gradients. The fp32
    part is what the kernels do in fp32 -- w, t - t0 of the tile, the exclusive prefixes, X, e_i, dX/dt_i -- and the rest of the chain is the fp64 graph."""
    c, G = aux.case(name), feature_cases._graph(name)
    ref = reference(name, mode) if with_image else reference_alone(name, mode)
    f32 = torch.float32
    H, W = G['H'], G['W']
    w = G['w'].detach().to(f32)
    w2c = torch.tensor(np.asarray(c['S'].w2c), dtype=f32)
    z = G['P']['means'].detach().to(f32)[G['order']] @ w2c[2, :3] + w2c[2, 3]
    z0 = z[_tile_origin_rank(name)]                                    # [P]
    ts = z[None, :] - z0[:, None]
    if mode == 'normalized':
        near, far = float(c['view'].near_plane), float(c['view'].far_plane)
        ts = torch.tensor(far * near / (far - near), dtype=f32) * ts / (z[None, :] * z0[:, None])
    zero = torch.zeros_like(w[:, :1])
    A_in, D_in = torch.cumsum(w, dim=1), torch.cumsum(w * ts, dim=1)
    A, D = torch.cat([zero, A_in[:, :-1]], dim=1), torch.cat([zero, D_in[:, :-1]], dim=1)
    A_n, D_n = A_in[:, -1:], D_in[:, -1:]
    X = 2.0 * (w * (ts * A - D)).sum(dim=1)
    e = 2.0 * (ts * (2.0 * A - A_n) - 2.0 * D + D_n)
    dXdt = 2.0 * w * (2.0 * A + w - A_n)
    assert X.dtype == e.dtype == dXdt.dtype == f32
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    gX = t64(grad_map(name)).reshape(-1)
    loss_image = (G['image'] * t64(c['gC']).reshape(3, H, W)).sum()
    grads = torch.autograd.grad([loss_image, G['w'], _t_of(name, mode)], list(G['P'].values()),
                                grad_outputs=[torch.full((), 1.0 if with_image else 0.0, dtype=torch.float64), gX[:, None] * e.double(), (gX[:, None] * dXdt.double()).sum(dim=0)],
                                retain_graph=True, allow_unused=True)
    keep = c['keep'].reshape(-1)
    report = {'map': helpers.rel_inf(X.numpy()[keep], ref['map'].reshape(-1)[keep])}
    for (k, v), g in zip(G['P'].items(), grads):
        g = g.numpy() if g is not None else np.zeros(tuple(v.shape))
        report[k] = helpers.rel_inf(g, ref[k])
    return report


def run(be, c: dict, mode: str, gC, gX, device='cpu', res=None, RS=None) -> dict:
    """forward + blend_distortion + backward_distortion through the backend: numpy image, map, state and the six gradients under helpers.GRAD_KEYS."""
    RS = aux.settings_of(c, device) if RS is None else RS
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    res = be.forward(*p, RS) if res is None else res
    normalized = mode == 'normalized'
    state = be.blend_distortion(p[0], res, p[0].shape[0], RS, normalized)
    dev = lambda g: None if g is None else torch.as_tensor(g).to(device)
    grads = be.backward_distortion(None, dev(gC), dev(gX), res.image, state, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state, normalized)
    out = {'image': res.image.cpu().numpy(), 'map': state[0].cpu().numpy(), 'state': state, 'res': res}
    out.update({k: g.cpu().numpy() for k, g in zip(helpers.GRAD_KEYS, grads)})
    return out


def check_against_reference(be, name: str, mode: str, device='cpu', exact_image: bool = True) -> dict:
    """One (case, mode) end to end: map, image, the six gradients against fp64 and a rerun; every figure is printed before it is held to its bar."""
    c, ref = aux.case(name), reference(name, mode)
    gX = grad_map(name)
    out = run(be, c, mode, c['gC'], gX, device)
    again = run(be, c, mode, c['gC'], gX, device)
    plain = aux.run_plain(be, c, c['gC'], device)
    keep = c['keep']
    report = {'zeroed': float((~keep).mean()), 'map': helpers.rel_inf(out['map'][keep], ref['map'][keep]),
              'image_vs_plain': float(np.abs(out['image'] - plain['image']).max())}
    for k in helpers.GRAD_KEYS:
        report[k] = helpers.rel_inf(out[k], np.asarray(ref[k]).reshape(out[k].shape))
        report[k + '_rerun'] = helpers.rel_inf(again[k], out[k])
    report['map_rerun'] = helpers.rel_inf(again['map'], out['map'])
    print(name, mode, device, report)
    fewer_than_two = c['f']['n_processed'].reshape(keep.shape) < 2
    assert not out['map'][fewer_than_two].any(), name
    assert np.isfinite(out['map']).all() and float(np.abs(ref['map']).max()) > 0
    assert report['map'] < MAP_TOL, (name, mode, report)
    if exact_image:
        assert np.array_equal(out['image'], plain['image']), name
    else:
        assert helpers.rel_inf(out['image'], plain['image']) < MAP_TOL, (name, report)
    for k in helpers.GRAD_KEYS:
        assert report[k] < GRAD_TOL, (name, mode, k, report)
        assert report[k + '_rerun'] < RERUN_TOL, (name, mode, k, report)
    assert report['map_rerun'] < RERUN_TOL, (name, mode, report)
    return report


def check_term_alone(be, name: str, mode: str, device='cpu') -> dict:
    """gC = 0: the four gradients the distortion term reaches against the fp64 gradients of sum(gX X) alone; the SH gradients are exactly 0."""
    c, ref = aux.case(name), reference_alone(name, mode)
    out = run(be, c, mode, np.zeros_like(c['gC']), grad_map(name), device)
    report = {k: helpers.rel_inf(out[k], np.asarray(ref[k]).reshape(out[k].shape)) for k in ('means', 'scales', 'rotations', 'opacities')}
    print('term alone', name, mode, device, report)
    assert not out['sh0'].any() and not out['sh_rest'].any() and not ref['sh0'].any() and not ref['sh_rest'].any()
    for k, figure in report.items():
        assert float(np.abs(ref[k]).max()) > 0 and figure < GRAD_TOL, (name, mode, k, report)
    return report


def check_state(be, device='cpu') -> None:
    """Plane 1 of the state is forward_aux's alpha. Plane 2 is kept in a t shifted by a tile-uniform origin, so instead of comparing it with the
    expected depth: an offset added to every view-space depth (w2c[2, 3], handed to blend_distortion only -- the forward pass is the same one)
    leaves the linear X unchanged."""
    for name in ('partial_tiles', 'stacked'):
        c = aux.case(name)
        RS = aux.settings_of(c, device)
        p = [c['params'][k].to(device) for k in helpers.NAMES]
        n, keep = p[0].shape[0], c['keep']
        res = be.forward_aux(*p, RS)                                     # its buffers serve the distortion blend as well
        state = be.blend_distortion(p[0], res, n, RS, False).cpu().numpy()
        v = c['view']
        w2c = v.w2c.clone()
        w2c[2, 3] += 3.0
        moved = View(w2c, v.position, v.width, v.height, v.focal_x, v.focal_y, v.center_x, v.center_y, v.near_plane, v.far_plane, v.background_color)
        RS_moved = helpers.settings_pair(moved, c['K'], c['aa'], device=device)[1]
        shifted = be.blend_distortion(p[0], res, n, RS_moved, False).cpu().numpy()
        report = {'plane1_vs_alpha': helpers.rel_inf(state[1][keep], res.alpha.cpu().numpy()[keep]),
                  'offset': helpers.rel_inf(shifted[0][keep], state[0][keep])}
        print('state', name, device, report)
        assert report['plane1_vs_alpha'] < MAP_TOL and report['offset'] < MAP_TOL, (name, report)


def check_boundaries(be, device='cpu') -> None:
    """gX = None is the plain pass; gC = 0 with gX != 0 moves means, scales, rotations and opacities and leaves the SH gradients exactly 0; a second
    backward pass over retained buffers equals the first; poisoned scratch changes nothing."""
    name, mode = 'hot', 'normalized'
    c = aux.case(name)
    gX = grad_map(name)
    first = run(be, c, mode, c['gC'], gX, device)
    plain = aux.run_plain(be, c, c['gC'], device)
    none = run(be, c, mode, c['gC'], None, device)
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(none[k], plain[k]) < RERUN_TOL, ('no distortion gradient', k)
    only = run(be, c, mode, np.zeros_like(c['gC']), gX, device)
    for k in ('means', 'scales', 'rotations', 'opacities'):
        assert float(np.abs(only[k]).max()) > 0, k
    assert not only['sh0'].any() and not only['sh_rest'].any()
    second = run(be, c, mode, c['gC'], gX, device, res=first['res'])
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(second[k], first[k]) < RERUN_TOL, ('second pass', k)
    assert max(float(np.abs(first[k] - plain[k]).max()) for k in ('means', 'scales', 'rotations', 'opacities')) > 0       # the distortion term is there
    dirty = run(helpers.poisoned(be), c, mode, c['gC'], gX, device)
    for k in ('image', 'map') + helpers.GRAD_KEYS:
        assert helpers.rel_inf(dirty[k], first[k]) < RERUN_TOL, ('poisoned', k)


def check_errors_and_empty(be, device='cpu') -> None:
    """Every refusal with its text, and n = 0."""
    import pytest
    c = aux.case('partial_tiles')
    RS = aux.settings_of(c, device)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    n, H, W = p[0].shape[0], c['view'].height, c['view'].width
    total_rest = p[5].shape[1]
    res = be.forward(*p, RS)
    gi = torch.as_tensor(c['gC']).to(device)
    gX = torch.as_tensor(grad_map('partial_tiles')).to(device)
    state = be.blend_distortion(p[0], res, n, RS)
    back = lambda st, g, r=res, settings=RS: be.backward_distortion(None, gi, g, r.image, st, p[0], p[1], p[2], p[3], p[5], r.buffers, settings, r.state)
    with pytest.raises(RuntimeError, match=r'means must be a contiguous float32 \[N, 3\]'):
        be.blend_distortion(p[0][:-1].contiguous(), res, n, RS)
    with pytest.raises(RuntimeError, match='grad_distortion must be'):
        back(state, gX[:-1])
    with pytest.raises(RuntimeError, match='distortion_state must be'):
        back(state[:2], gX)
    # the planes of the normalized mode: refused by the library, forward and backward; the linear mode does not look at them
    v = c['view']
    for near, far in ((0.0, 10.0), (-1.0, 10.0), (2.0, 2.0), (2.0, 1.0)):
        bad = View(v.w2c, v.position, v.width, v.height, v.focal_x, v.focal_y, v.center_x, v.center_y, near, far, v.background_color)
        RS_bad = helpers.settings_pair(bad, c['K'], c['aa'], device=device)[1]
        with pytest.raises(RuntimeError, match='0 < near_plane < far_plane'):
            be.blend_distortion(p[0], res, n, RS_bad)
        with pytest.raises(RuntimeError, match='0 < near_plane < far_plane'):
            back(state, gX, settings=RS_bad)
        be.blend_distortion(p[0], res, n, RS_bad, False)
    asynchronous = be.forward(*p, RS, instance_capacity=1 << 20)
    with pytest.raises(RuntimeError, match='fgs_forward_async'):
        be.blend_distortion(p[0], asynchronous, n, RS)
    with pytest.raises(RuntimeError, match='fgs_forward_async'):
        back(state, gX, asynchronous)
    # the record path for real: one owner's K1, then the render from its splat records -- the state that pass returns is refused
    rec = torch.zeros((1, n, 56), dtype=torch.uint8, device=device)
    counts = torch.zeros((1, 2), dtype=torch.int32, device=device)
    be.shard_preprocess(*p, [RS], rec, counts)
    n_visible, n_instances = (int(x) for x in counts[0].cpu())
    assert n_visible > 0
    records = be.forward_from_records(rec.view(-1), n_visible, n_instances, RS, total_rest)
    with pytest.raises(RuntimeError, match='record'):
        be.blend_distortion(p[0][:n_visible].contiguous(), records, n_visible, RS)
    with pytest.raises(RuntimeError, match='record'):
        be.backward_distortion(None, gi, gX, records.image, state, p[0][:n_visible].contiguous(), p[1][:n_visible].contiguous(),
                               p[2][:n_visible].contiguous(), p[3][:n_visible].contiguous(), p[5][:n_visible].contiguous(), records.buffers, RS, records.state)
    with pytest.raises(RuntimeError, match='takes no distortion gradient'):
        be.backward_adam_fused(None, gi, res.image, [], [], [], res.buffers, RS, res.state, 1, [], grad_distortion=gX)
    with pytest.raises(RuntimeError, match='takes no distortion gradient'):
        be.backward_to_records(gi, res.image, res.buffers, RS, res.state, 15, grad_distortion=gX)
    # n = 0: a zero state, empty gradients
    empty = [t[:0].contiguous() for t in p]
    r0 = be.forward(*empty, RS)
    s0 = be.blend_distortion(empty[0], r0, 0, RS)
    assert s0.shape == (3, H, W) and not s0.any()
    g0 = be.backward_distortion(None, torch.ones_like(r0.image), torch.ones_like(s0[0]), r0.image, s0, empty[0], empty[1], empty[2], empty[3], empty[5],
                                r0.buffers, RS, r0.state)
    assert len(g0) == 6 and all(g.shape[0] == 0 for g in g0)


def check_abi_refusals(lib, _lib) -> None:
    """The C entry points refuse by themselves, before anything is launched; the ABI version stays 3."""
    import ctypes as C
    st = _lib.ForwardState()
    S = _lib.Settings(1, 1, 1, 16, 15, 128, 128, 1.0, 1.0, 0.0, 0.0, 0.2, 100.0, 0)
    blend = lambda means=1, state=st, mode=1, out=1, settings=S: lib.fgs_blend_distortion(means, 1, 1, 1, 10, C.byref(settings), C.byref(state), mode, out, None)
    back = lambda state=st, mode=1, dstate=1, settings=S, g=1: lib.fgs_backward_distortion(
        *([1] * 22), 10, C.byref(settings), C.byref(state), None, None, dstate, g, mode, None)
    for call in (blend, back):
        for bad in (2, -1):
            assert call(mode=bad) == -1 and b'distortion mode' in lib.fgs_last_error()
        for near, far in ((0.0, 100.0), (5.0, 5.0), (5.0, 1.0)):
            planes = _lib.Settings(1, 1, 1, 16, 15, 128, 128, 1.0, 1.0, 0.0, 0.0, near, far, 0)
            assert call(settings=planes) == -1 and b'0 < near_plane < far_plane' in lib.fgs_last_error()
        for bit, text in ((4, b'fgs_forward_async'), (8, b'record')):
            assert call(state=_lib.ForwardState(0, 0, 0, bit)) == -1 and text in lib.fgs_last_error()
    assert blend(out=None) == -1 and b'NULL distortion_state' in lib.fgs_last_error()
    assert blend(means=None) == -1 and b'NULL means' in lib.fgs_last_error()
    assert back(dstate=None) == -1 and b'NULL distortion_state' in lib.fgs_last_error()
    assert lib.fgs_abi_version() == 3


def check_operator(B, be, name: str, device='cpu') -> None:
    """The public operator B.diff_rasterize_distortion against the backend `be` it runs on: outputs and the six gradients equal to the backend's, a
    second backward over the retained graph, a non-contiguous gX, an unused map = the plain pass, an unused image, torch.no_grad()."""
    c = aux.case(name)
    RS = aux.settings_of(c, device)
    gC = torch.as_tensor(c['gC']).to(device)
    gX = torch.as_tensor(grad_map(name)).to(device)
    leaves_of = lambda: [c['params'][k].to(device).clone().requires_grad_(True) for k in helpers.NAMES]
    none = torch.empty(0)
    for mode in MODES:
        direct = run(be, c, mode, c['gC'], gX, device)
        leaves = leaves_of()
        image, dmap = B.diff_rasterize_distortion(*leaves, none, RS, normalized=mode == 'normalized')
        assert image.shape == (3, c['view'].height, c['view'].width) and dmap.shape == image.shape[1:]
        assert torch.equal(dmap.detach().cpu(), torch.as_tensor(direct['map'])) and torch.equal(image.detach().cpu(), torch.as_tensor(direct['image']))
        loss = (image * gC).sum() + (dmap * gX).sum()
        first = torch.autograd.grad(loss, leaves, retain_graph=True)
        second = torch.autograd.grad(loss, leaves)
        for k, g1, g2 in zip(helpers.GRAD_KEYS, first, second):
            assert helpers.rel_inf(g1.cpu().numpy(), direct[k]) < RERUN_TOL, (mode, k)
            assert helpers.rel_inf(g2.cpu().numpy(), g1.cpu().numpy()) < RERUN_TOL, (mode, k)
    direct = run(be, c, 'normalized', c['gC'], gX, device)

    # a non-contiguous incoming gradient is made contiguous; the default mode is the normalized one
    leaves = leaves_of()
    image, dmap = B.diff_rasterize_distortion(*leaves, none, RS)
    gX_t = gX.t().contiguous().t()
    assert not gX_t.is_contiguous()
    strided = torch.autograd.grad((image * gC).sum() + (dmap * gX_t).sum(), leaves)
    for k, g in zip(helpers.GRAD_KEYS, strided):
        assert helpers.rel_inf(g.cpu().numpy(), direct[k]) < RERUN_TOL, k

    # the map is not part of the loss: the pass is the plain one
    leaves = leaves_of()
    image, _ = B.diff_rasterize_distortion(*leaves, none, RS)
    unused = torch.autograd.grad((image * gC).sum(), leaves)
    leaves = leaves_of()
    plain = torch.autograd.grad((B.diff_rasterize(*leaves, none, RS) * gC).sum(), leaves)
    for k, g, q in zip(helpers.GRAD_KEYS, unused, plain):
        assert helpers.rel_inf(g.cpu().numpy(), q.cpu().numpy()) < RERUN_TOL, k

    # the image is not part of the loss: its gradient arrives as None and is passed on as zeros
    leaves = leaves_of()
    _, dmap = B.diff_rasterize_distortion(*leaves, none, RS)
    only = torch.autograd.grad((dmap * gX).sum(), leaves)
    want = run(be, c, 'normalized', np.zeros_like(c['gC']), gX, device)
    for k, g in zip(helpers.GRAD_KEYS, only):
        assert helpers.rel_inf(g.cpu().numpy(), want[k]) < RERUN_TOL, k
    assert float(only[0].abs().max()) > 0

    with torch.no_grad():
        image, dmap = B.diff_rasterize_distortion(*leaves_of(), none, RS)
    assert not dmap.requires_grad and torch.equal(dmap.cpu(), torch.as_tensor(direct['map']))
