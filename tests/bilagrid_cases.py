"""Bilateral-grid colour correction (csrc/bilagrid.hip): definitions, the fp64 reference, the seeded cases and the bars that tests/test_bilagrid.py
(CPU simulation of the product sources) and tests/test_gpu_bilagrid.py (MI355X) share.

Reference: the definition itself in fp64 torch with autograd on the CPU -- F.grid_sample(G[None], 2 (x, y, g) - 1, mode='bilinear',
align_corners=True, padding_mode='border') with x = (px + 0.5) / W, y = (py + 0.5) / H, g = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1), followed by the
3 x 4 matrix product. The kernels restate it as a trilinear interpolation with clamped corner indices; an fp32 evaluation of either misses the fp64 one
by 1e-7 .. 7e-7 (rel_inf), so the project's bar rel_inf < 1e-4 (aux_grad_cases.GRAD_TOL) applies unchanged.

Inputs are seeded: grids [I | 0] + 0.2 N(0, 1), images uniform in [-0.2, 1.2], upstream gradients N(0, 1) / (3 H W). The gradient through the guide is
discontinuous at the lattice planes and at the two ends of the clamp, so a pixel whose UNCLAMPED guide lies within 1e-4 of 0 or 1, or lies strictly
inside (0, 1) with guide * (L - 1) within 1e-4 of an integer, is drawn again until none is left (a clamped pixel sits on plane 0 or L - 1 by
definition and a grid with L = 1 has no plane to cross: neither is "near" one). Nothing is masked; about 4 % of the pixels stay clamped.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import aux_grad_cases as aux
import helpers

TOL = aux.GRAD_TOL              # 1e-4: out, grad_image, grad_grid against fp64
IDENTITY_TOL = 1e-6             # an identity grid returns the image / the upstream gradient
TV_TOL = 1e-5
RUN_TO_RUN = 1e-5               # two device runs differ by the order of float atomics (the bar of test_gpu_aux_grad.py)
LUMA = (0.299, 0.587, 0.114)

# name: ((W, H), (Wg, Hg, L), the kernels stage the grid under a tile in LDS)
CASES = {
    'fine': ((50, 37), (16, 16, 8), False),         # partial tiles on both axes, dozens of cells under one tile: the global-memory path
    'coarse': ((64, 48), (3, 2, 4), True),          # several workgroups inside one cell: LDS staging, contended flushes
    'flat1': ((21, 13), (1, 1, 1), True),           # degenerate axes
    'flat2': ((21, 13), (2, 2, 2), True),
    'wide': ((256, 144), (16, 16, 8), True),        # GPU only: 36 workgroups (64 x 16 pixel tiles), four or five of them over every cell
    'crowd': ((768, 432), (2, 2, 2), True),         # GPU only: 324 workgroups flushing into the same eight lattice points
}
CPU_CASES = ('fine', 'coarse', 'flat1', 'flat2')
GPU_CASES = CPU_CASES + ('wide', 'crowd')


def identity_grid(gw: int, gh: int, gl: int) -> torch.Tensor:
    g = torch.zeros(12, gl, gh, gw, dtype=torch.float32)
    g[[0, 5, 10]] = 1.0
    return g


def guide64(image: np.ndarray) -> np.ndarray:
    im = np.asarray(image, np.float64)
    return LUMA[0] * im[0] + LUMA[1] * im[1] + LUMA[2] * im[2]


def near_a_discontinuity(image: np.ndarray, gl: int) -> np.ndarray:
    raw = guide64(image)
    bad = (np.abs(raw) < 1e-4) | (np.abs(raw - 1.0) < 1e-4)
    if gl > 1:
        z = raw * (gl - 1)
        bad |= (raw > 0) & (raw < 1) & (np.abs(z - np.round(z)) < 1e-4)
    return bad


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    (w, h), (gw, gh, gl), staged = CASES[name]
    seed = 100 + sorted(CASES).index(name)
    gen = torch.Generator().manual_seed(seed)
    grid = (identity_grid(gw, gh, gl) + 0.2 * torch.randn(12, gl, gh, gw, generator=gen)).contiguous()
    image = (torch.rand(3, h, w, generator=gen) * 1.4 - 0.2).contiguous()
    for _ in range(100):
        bad = torch.from_numpy(near_a_discontinuity(image.numpy(), gl))
        if not bad.any():
            break
        fresh = torch.rand(3, h, w, generator=gen) * 1.4 - 0.2
        image = torch.where(bad[None], fresh, image).contiguous()
    assert not near_a_discontinuity(image.numpy(), gl).any(), name
    raw = guide64(image.numpy())
    clamped = float(((raw < 0) | (raw > 1)).mean())
    assert clamped > 0, name                           # the zero-gradient rule of the clamped guide is exercised
    gO = (torch.randn(3, h, w, generator=gen) / (3 * h * w)).contiguous()
    return {'name': name, 'grid': grid, 'image': image, 'gO': gO, 'extents': (gw, gh, gl), 'size': (w, h), 'staged': staged, 'clamped': clamped}


def reference_of(image: torch.Tensor, grid: torch.Tensor, gO: torch.Tensor) -> dict:
    """out, grad_image and grad_grid of the grid_sample formulation in fp64 (numpy arrays)."""
    Cm = image.detach().double().cpu().requires_grad_(True)
    G = grid.detach().double().cpu().requires_grad_(True)
    _, h, w = Cm.shape
    xs = ((torch.arange(w, dtype=torch.float64) + 0.5) / w)[None, :].expand(h, w)
    ys = ((torch.arange(h, dtype=torch.float64) + 0.5) / h)[:, None].expand(h, w)
    g = (LUMA[0] * Cm[0] + LUMA[1] * Cm[1] + LUMA[2] * Cm[2]).clamp(0.0, 1.0)
    coords = torch.stack([xs, ys, g], dim=-1) * 2.0 - 1.0                     # (x, y, z) -> (Wg, Hg, L)
    M = F.grid_sample(G[None], coords[None, None], mode='bilinear', align_corners=True, padding_mode='border')[0, :, 0].reshape(3, 4, h, w)
    out = (M[:, :3] * Cm[None]).sum(dim=1) + M[:, 3]
    (out * gO.detach().double().cpu()).sum().backward()
    return {'out': out.detach().numpy(), 'grad_image': Cm.grad.numpy(), 'grad_grid': G.grad.numpy()}


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """The fp64 reference of case `name`: once per process, shared, read-only."""
    c = case(name)
    return reference_of(c['image'], c['grid'], c['gO'])


def tv_reference(grid: torch.Tensor) -> tuple:
    G = grid.detach().double().cpu().requires_grad_(True)
    tv = sum(((G.narrow(d, 1, G.shape[d] - 1) - G.narrow(d, 0, G.shape[d] - 1)) ** 2).mean() for d in (1, 2, 3) if G.shape[d] > 1)
    tv = tv + 0.0 * G.sum()
    tv.backward()
    return float(tv.detach()), G.grad.numpy()


def run(be, c: dict, device='cpu', need_grid: bool = True, need_image: bool = True) -> dict:
    image, grid, gO = (c[k].to(device) for k in ('image', 'grid', 'gO'))
    out = be.bilagrid_slice(image, grid)
    gg, gi = be.bilagrid_slice_backward(image, grid, gO, need_grid=need_grid, need_image=need_image)
    return {'out': out.cpu().numpy(), 'grad_grid': None if gg is None else gg.cpu().numpy(), 'grad_image': None if gi is None else gi.cpu().numpy()}


def poisoned(be):
    """helpers.poisoned plus this operator's scratch: everything arrives as 0xFF bytes."""
    class Poisoned(type(helpers.poisoned(be))):
        def _scratch_bilagrid(self, extents, device):
            t = super()._scratch_bilagrid(extents, device)
            t.fill_(255)
            return t
    return Poisoned(be.lib)


# ---- the checks -------------------------------------------------------------------------------------------------------------------------------------------
def check_parity(be, name: str, device='cpu') -> dict:
    """1. out, grad_image, grad_grid against fp64 at rel_inf < 1e-4; the path the case is meant to take is the one that ran."""
    c, ref = case(name), reference(name)
    assert be.bilagrid_staged(c['grid'].shape, *c['size']) == c['staged'], name
    got = run(be, c, device)
    errs = {k: helpers.rel_inf(got[k], ref[k]) for k in ('out', 'grad_image', 'grad_grid')}
    print(f'bilagrid {name} on {device}: clamped share {c["clamped"]:.3f}, rel_inf vs fp64 {errs}')
    assert all(np.isfinite(got[k]).all() for k in errs) and max(errs.values()) < TOL, (name, errs)
    return errs


def check_identity(be, name: str, device='cpu') -> None:
    """2. An identity grid returns the image, and grad_image = gO."""
    c = case(name)
    ident = dict(c, grid=identity_grid(*c['extents']))
    got = run(be, ident, device)
    assert helpers.rel_inf(got['out'], c['image'].numpy()) < IDENTITY_TOL and helpers.rel_inf(got['grad_image'], c['gO'].numpy()) < IDENTITY_TOL, name


def check_null_gradients(be, name: str, device='cpu', exact_grid: bool = True) -> None:
    """3. A NULL grad_grid / grad_image leaves the other one as the full call computes it: bit for bit (the grid gradient on the device: up to the
    order of its atomics)."""
    c = case(name)
    full, only_image, only_grid = run(be, c, device), run(be, c, device, need_grid=False), run(be, c, device, need_image=False)
    assert only_image['grad_grid'] is None and only_grid['grad_image'] is None
    assert np.array_equal(only_image['grad_image'], full['grad_image']), name
    if exact_grid:
        assert np.array_equal(only_grid['grad_grid'], full['grad_grid']), name
    else:
        assert helpers.rel_inf(only_grid['grad_grid'], full['grad_grid']) < RUN_TO_RUN, name


def check_stale_scratch(be, name: str, device='cpu', exact: bool = True) -> None:
    """4. Scratch that arrives as 0xFF bytes changes nothing."""
    c = case(name)
    clean, dirty = run(be, c, device), run(poisoned(be), c, device)
    assert np.array_equal(dirty['out'], clean['out']) and np.array_equal(dirty['grad_image'], clean['grad_image']), name
    if exact:
        assert np.array_equal(dirty['grad_grid'], clean['grad_grid']), name
    else:
        assert helpers.rel_inf(dirty['grad_grid'], clean['grad_grid']) < RUN_TO_RUN, name


def check_tv(be, device='cpu') -> None:
    """5. TV value and gradient against fp64 at 1e-5; an extent-1 axis contributes exactly 0; tv([I | 0]) == 0 exactly."""
    for name in ('fine', 'coarse', 'flat1', 'flat2'):
        c = case(name)
        tv, grad = be.bilagrid_tv(c['grid'].to(device))
        ref_tv, ref_grad = tv_reference(c['grid'])
        assert abs(float(tv) - ref_tv) <= TV_TOL * abs(ref_tv) and helpers.rel_inf(grad.cpu().numpy(), ref_grad) < TV_TOL, (name, float(tv), ref_tv)
        ident, ident_grad = be.bilagrid_tv(identity_grid(*c['extents']).to(device))
        assert float(ident) == 0.0 and not ident_grad.any(), name
        assert be.bilagrid_tv(c['grid'].to(device), with_grad=False)[1] is None
    gen = torch.Generator().manual_seed(9)
    flat_tv, flat_grad = be.bilagrid_tv(torch.randn(12, 1, 1, 1, generator=gen).to(device))
    assert float(flat_tv) == 0.0 and not flat_grad.any()                                  # three extent-1 axes: exactly 0
    line = torch.randn(12, 1, 1, 5, generator=gen)                                        # only x has neighbours: the other two axes add exactly 0
    tv, grad = be.bilagrid_tv(line.to(device))
    d = (line[..., 1:] - line[..., :-1]).double()
    assert abs(float(tv) - float((d ** 2).mean())) <= TV_TOL * float((d ** 2).mean())
    ref_tv, ref_grad = tv_reference(line)
    assert helpers.rel_inf(grad.cpu().numpy(), ref_grad) < TV_TOL


def check_refusals(be, device='cpu') -> None:
    """6. The refusals of the C ABI by their error text, and of the backend's argument checks; the ABI version stays 3."""
    lib = be.lib
    c = case('coarse')
    image, grid, gO = (c[k].to(device) for k in ('image', 'grid', 'gO'))
    (gw, gh, gl), (w, h) = c['extents'], c['size']
    out, gg, gi = torch.empty_like(image), torch.full_like(grid, 7.0), torch.full_like(image, 7.0)
    scratch = torch.empty(int(lib.fgs_bilagrid_scratch_bytes(gw, gh, gl)), dtype=torch.uint8, device=device)
    assert scratch.numel() == 4 * 12 * gw * gh * gl and lib.fgs_bilagrid_scratch_bytes(0, gh, gl) == 0
    P = lambda t: t.data_ptr()
    err = lambda: lib.fgs_last_error().decode()
    assert lib.fgs_bilagrid_slice(None, gw, gh, gl, P(image), w, h, P(out), None) == -1 and 'NULL' in err()
    assert lib.fgs_bilagrid_slice(P(grid), gw, gh, gl, None, w, h, P(out), None) == -1 and 'NULL' in err()
    assert lib.fgs_bilagrid_slice(P(grid), gw, gh, gl, P(image), w, h, None, None) == -1 and 'NULL' in err()
    assert lib.fgs_bilagrid_slice(P(grid), 0, gh, gl, P(image), w, h, P(out), None) == -1 and 'grid extents' in err()
    assert lib.fgs_bilagrid_slice(P(grid), gw, gh, -1, P(image), w, h, P(out), None) == -1 and 'grid extents' in err()
    assert lib.fgs_bilagrid_slice(P(grid), gw, gh, gl, P(image), 0, h, P(out), None) == -1 and 'image size' in err()
    assert lib.fgs_bilagrid_slice(P(grid), gw, gh, gl, P(image), w, h, P(image), None) == -1 and 'aliases image' in err()
    assert lib.fgs_bilagrid_slice(P(grid), gw, gh, gl, P(image), w, h, P(image) + 4 * w, None) == -1 and 'aliases image' in err()
    back = lambda *a: lib.fgs_bilagrid_slice_backward(*a, None)
    assert back(None, gw, gh, gl, P(image), P(gO), w, h, P(gg), P(gi), P(scratch)) == -1 and 'NULL' in err()
    assert back(P(grid), gw, gh, gl, P(image), None, w, h, P(gg), P(gi), P(scratch)) == -1 and 'NULL' in err()
    assert back(P(grid), gw, gh, gl, P(image), P(gO), w, h, None, None, P(scratch)) == -1 and 'both NULL' in err()
    assert back(P(grid), gw, gh, gl, P(image), P(gO), w, h, P(gg), P(gi), None) == -1 and 'needs scratch' in err()
    assert back(P(grid), gw, 0, gl, P(image), P(gO), w, h, P(gg), P(gi), P(scratch)) == -1 and 'grid extents' in err()
    assert back(P(grid), gw, gh, gl, P(image), P(gO), w, -3, P(gg), P(gi), P(scratch)) == -1 and 'image size' in err()
    loss = torch.full((), 7.0, device=device)
    assert lib.fgs_bilagrid_tv(None, gw, gh, gl, P(loss), P(gg), None) == -1 and 'NULL' in err()
    assert lib.fgs_bilagrid_tv(P(grid), gw, gh, gl, None, P(gg), None) == -1 and 'NULL' in err()
    assert lib.fgs_bilagrid_tv(P(grid), gw, gh, 0, P(loss), P(gg), None) == -1 and 'grid extents' in err()
    assert lib.fgs_bilagrid_staged(gw, gh, gl, 0, h) < 0 and lib.fgs_bilagrid_staged(0, gh, gl, w, h) < 0
    assert float(loss) == 7.0 and bool((gg == 7.0).all()) and bool((gi == 7.0).all())            # a refused call writes nothing
    assert lib.fgs_abi_version() == 3
    # the backend's checks: dtype, shape, device, contiguity
    import pytest
    with pytest.raises(RuntimeError, match='contiguous float32'):
        be.bilagrid_slice(image.double(), grid)
    with pytest.raises(RuntimeError, match='contiguous float32'):
        be.bilagrid_slice(image, grid.transpose(2, 3))
    with pytest.raises(RuntimeError, match=r'\[12, L, Hg, Wg\]'):
        be.bilagrid_slice(image, grid[:11].contiguous())
    with pytest.raises(RuntimeError, match=r'\[3, H, W\]'):
        be.bilagrid_slice(image[:2].contiguous(), grid)
    with pytest.raises(RuntimeError, match='shape of the image'):
        be.bilagrid_slice_backward(image, grid, gO[:, :-1].contiguous())
    with pytest.raises(RuntimeError, match='contiguous float32'):
        be.bilagrid_tv(grid.half())
    if device != 'cpu':
        with pytest.raises(RuntimeError, match='contiguous float32'):
            be.bilagrid_slice(image.cpu(), grid)


def check_operators(B, be, device='cpu', tol: float = 0.0) -> None:
    """7. torch.autograd.grad through diff_rasterize -> bilagrid_slice -> sum on `partial_tiles` equals the backend pieces composed by hand; no_grad runs
    the forward pass only; an input without requires_grad gets None."""
    c = aux.case('partial_tiles')
    RS = aux.settings_of(c, device)
    h, w = c['view'].height, c['view'].width
    gen = torch.Generator().manual_seed(3)
    grid = (identity_grid(5, 4, 3) + 0.2 * torch.randn(12, 3, 4, 5, generator=gen)).to(device)
    same = (lambda a, b: torch.equal(a, b)) if tol == 0.0 else (lambda a, b: helpers.rel_inf(a.cpu().numpy(), b.cpu().numpy()) < tol)
    p = [c['params'][k].to(device) for k in helpers.NAMES]
    res = be.forward(*p, RS)
    out_hand = be.bilagrid_slice(res.image, grid)
    gg_hand, gi_hand = be.bilagrid_slice_backward(res.image, grid, torch.ones_like(out_hand))
    grads_hand = be.backward(None, gi_hand, res.image, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)

    leaves = [t.clone().requires_grad_(True) for t in p]
    grid_leaf = grid.clone().requires_grad_(True)
    out = B.bilagrid_slice(B.diff_rasterize(*leaves, torch.empty(0), RS), grid_leaf)
    assert out.shape == (3, h, w) and same(out.detach(), out_hand)
    grads = torch.autograd.grad(out.sum(), leaves + [grid_leaf])
    assert same(grads[6], gg_hand)
    for k, g, ref in zip(helpers.GRAD_KEYS, grads[:6], grads_hand):
        assert same(g, ref.reshape(g.shape)), k

    with torch.no_grad():
        quiet = B.bilagrid_slice(res.image, grid_leaf)
        tv_quiet = B.bilagrid_tv_loss(grid_leaf)
    assert not quiet.requires_grad and quiet.grad_fn is None and same(quiet, out_hand) and not tv_quiet.requires_grad
    image_leaf = res.image.clone().requires_grad_(True)
    only_image = B.bilagrid_slice(image_leaf, grid)                                        # the grid does not require a gradient
    (gi,) = torch.autograd.grad(only_image.sum(), [image_leaf])
    assert same(gi, gi_hand)
    only_grid = B.bilagrid_slice(res.image, grid_leaf)
    only_grid.sum().backward()
    assert same(grid_leaf.grad, gg_hand) and image_leaf.grad is None
    calls = []
    spy = type(be).bilagrid_slice_backward
    try:                                                                                   # ... and it costs nothing: the backend is asked for one gradient
        type(be).bilagrid_slice_backward = lambda self, *a, **k: calls.append(k) or spy(self, *a, **k)
        torch.autograd.grad(B.bilagrid_slice(image_leaf, grid).sum(), [image_leaf])
    finally:
        type(be).bilagrid_slice_backward = spy
    assert calls == [{'need_grid': False, 'need_image': True}]
    # the regulariser: one node whose backward scales the kept gradient
    tv_hand, tv_grad_hand = be.bilagrid_tv(grid)
    grid_leaf.grad = None
    tv = B.bilagrid_tv_loss(grid_leaf)
    (3.0 * tv).backward()
    assert same(tv.detach(), tv_hand) and same(grid_leaf.grad, 3.0 * tv_grad_hand)


def training_pair(device='cpu', n: int = 1000, size: 'tuple | None' = None):
    """make_s0(n) at its own size (or, for the simulation, the same camera at `size` = (W, H)) with the Gaussians at the truth, and a fixed non-identity
    grid for the target to go through."""
    from harness import trainer as T
    from harness.scenes import View, make_s0
    dev = torch.device(device)
    params, view = make_s0(n=n)
    if size is not None:
        f = view.focal_x * size[0] / view.width
        view = View(view.w2c, view.position, size[0], size[1], f, f, size[0] / 2.0, size[1] / 2.0, view.near_plane, view.far_plane, view.background_color)
    view = view.to(dev)
    g = T.Gaussians(params, dev)
    gen = torch.Generator().manual_seed(17)
    fixed = identity_grid(4, 4, 2)
    fixed[[0, 5, 10]] *= torch.tensor([0.8, 0.9, 1.1])[:, None, None, None]               # a colour cast ...
    fixed = (fixed + 0.03 * torch.randn(fixed.shape, generator=gen)).to(dev).contiguous()  # ... that varies over the image and with luma
    return T, g, view, fixed


def check_training_iteration(be, device='cpu', exact: bool = True) -> None:
    """8a. One training_iteration(..., bilagrid=m, view_index=0) equals the same step composed by hand from the operators and torch Adam."""
    import FasterGSCudaBackend as B
    from harness.bilagrid import BilateralGrids
    T, g, view, fixed = training_pair(device, n=300)
    with torch.no_grad():
        target = B.bilagrid_slice(T.render_image_training(g, view, False, view.background_color), fixed)
    start = {k: getattr(g, k).detach().clone() for k in T.PARAM_ORDER}
    gen = torch.Generator().manual_seed(4)
    grid0 = (identity_grid(6, 5, 3) + 0.05 * torch.randn(12, 3, 5, 6, generator=gen)).to(device)

    def fresh():
        gg = T.Gaussians({k: v.clone() for k, v in start.items()}, torch.device(device))      # the module adopts the tensors it is given
        gg.training_setup(training_cameras_extent=4.0)
        m = BilateralGrids(2, shape=(6, 5, 3), device=device)
        with torch.no_grad():
            m.grids[0].copy_(grid0)
        m.training_setup()
        return gg, m
    ga, ma = fresh()
    loss_a = T.training_iteration(ga, view, target, 0, bilagrid=ma, view_index=0, tv_weight=10.0)
    gb, mb = fresh()
    gb.update_learning_rate(1)
    image = T.render_image_training(gb, view, True, view.background_color)
    loss_b = T.photometric_loss(B.bilagrid_slice(image, mb.grids[0]), target) + 10.0 * B.bilagrid_tv_loss(mb.grids[0])
    loss_b.backward()
    gb.optimizer.step()
    gb.optimizer.zero_grad()
    mb.optimizer.step()
    mb.optimizer.zero_grad()
    same = torch.equal if exact else (lambda a, b: helpers.rel_inf(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < RUN_TO_RUN)
    assert same(loss_a, loss_b.detach())
    for k in T.PARAM_ORDER:
        assert same(getattr(ga, k), getattr(gb, k)), k
        assert not torch.equal(getattr(ga, k), start[k].to(device)) or getattr(ga, k).numel() == 0, k
    assert same(ma.grids[0], mb.grids[0]) and not torch.equal(ma.grids[0], grid0)
    assert torch.equal(ma.grids[1], identity_grid(6, 5, 3).to(device)) and ma.grids[1] not in ma.optimizer.state      # the unseen view was not stepped


def check_training_run(device='cpu', steps: int = 30, n: int = 1000, size: 'tuple | None' = None) -> tuple:
    """8b. `steps` iterations against a target that went through a fixed non-identity grid, the Gaussians frozen at the truth: the image loss ends lower than
    the identity grid gives, and every loss is finite."""
    import FasterGSCudaBackend as B
    from harness.bilagrid import BilateralGrids
    T, g, view, fixed = training_pair(device, n=n, size=size)
    with torch.no_grad():
        rendered = T.render_image_training(g, view, False, view.background_color)
        target = B.bilagrid_slice(rendered, fixed)
        identity_loss = float(T.photometric_loss(rendered, target))
    g.training_setup(training_cameras_extent=4.0)
    for group in g.optimizer.param_groups:                  # frozen at the truth
        group['lr'] = 0.0
    g.update_learning_rate = lambda iteration: None
    m = BilateralGrids(1, shape=(4, 4, 2), device=device)
    m.training_setup()
    before = {k: getattr(g, k).detach().clone() for k in T.PARAM_ORDER}
    losses = [float(T.training_iteration(g, view, target, it, bilagrid=m, view_index=0)) for it in range(steps)]
    with torch.no_grad():
        final_loss = float(T.photometric_loss(m(rendered, 0), target))
    print(f'bilagrid training on {device}: identity grid {identity_loss:.5f}, after {steps} steps {final_loss:.5f}; losses {losses[0]:.5f} -> {losses[-1]:.5f}')
    assert all(np.isfinite(losses)) and np.isfinite(final_loss)
    assert final_loss < identity_loss
    assert all(torch.equal(getattr(g, k), before[k]) for k in T.PARAM_ORDER)
    corrected = T.render_image_corrected(g, view, m, 0)
    assert corrected.shape == rendered.shape and float(corrected.min()) >= 0.0 and float(corrected.max()) <= 1.0
    return identity_loss, final_loss


def check_checkpoint_round_trip(tmp_path, device='cpu', exact: bool = True) -> None:
    """8c. Save after two iterations, load into fresh objects, run a third on both: the same Gaussians and grids."""
    import FasterGSCudaBackend as B
    from harness import checkpoint as CK
    from harness.bilagrid import BilateralGrids
    T, g, view, fixed = training_pair(device, n=300)
    with torch.no_grad():
        target = B.bilagrid_slice(T.render_image_training(g, view, False, view.background_color), fixed)
    g.training_setup(training_cameras_extent=4.0)
    m = BilateralGrids(2, shape=(4, 3, 2), device=device)
    m.training_setup()
    for it in range(2):
        T.training_iteration(g, view, target, it, bilagrid=m, view_index=it % 2)
    T.training_iteration(g, view, target, 2, bilagrid=m, view_index=0)          # view 0 stepped twice, view 1 once
    path = tmp_path / 'with_grids.pt'
    CK.save_checkpoint(g, path, iteration=3, bilagrid=m)
    m2 = BilateralGrids(2, shape=(4, 3, 2), device=device)
    g2, it2 = CK.load_checkpoint(path, torch.device(device), bilagrid=m2)
    assert it2 == 3 and all(torch.equal(a, b) for a, b in zip(m.grids, m2.grids))
    assert [int(m2.optimizer.state[p]['step']) for p in m2.grids] == [2, 1]
    la = T.training_iteration(g, view, target, 3, bilagrid=m, view_index=1)
    lb = T.training_iteration(g2, view, target, 3, bilagrid=m2, view_index=1)
    same = torch.equal if exact else (lambda a, b: helpers.rel_inf(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < RUN_TO_RUN)
    assert same(la, lb)
    for k in T.PARAM_ORDER:
        assert same(getattr(g, k), getattr(g2, k)), k
    assert all(same(a, b) for a, b in zip(m.grids, m2.grids))
    # a checkpoint without grids loads as before, with or without the argument's absence; asking one for grids is an error
    plain = tmp_path / 'plain.pt'
    CK.save_checkpoint(g, plain, iteration=4)
    g3, it3 = CK.load_checkpoint(plain, torch.device(device))
    assert it3 == 4 and torch.equal(g3.means, g.means)
    g4, it4 = CK.load_checkpoint(path, torch.device(device))                     # the grids of the file are simply not read
    assert it4 == 3 and g4.means.shape == g.means.shape
    import pytest
    with pytest.raises(ValueError, match='no bilateral grids'):
        CK.load_checkpoint(plain, torch.device(device), bilagrid=m2)
    with pytest.raises(ValueError, match='grids of'):
        CK.load_checkpoint(path, torch.device(device), bilagrid=BilateralGrids(3, shape=(4, 3, 2), device=device))
