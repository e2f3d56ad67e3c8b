"""Shapes, weight patterns, fp64 reference and comparisons shared by tests/test_weighted_loss.py (CPU simulation) and tests/test_gpu_weighted_loss.py
(MI355X): the weighted L1 + DSSIM loss (csrc/loss.hip, the WEIGHTED instantiations) through its three call forms.

Definition (INTEGRATION.md 'Weighted loss'): w^ = w where w > 0 else 0; S = sum w^; x' = x where w^ > 0 else y;
  L1_w = sum w^ |x' - y| / (3 S),  SSIM_w = sum w^ SSIM(x', y) / (3 S),  loss = l1 * L1_w + ld * (1 - SSIM_w);  S = 0: loss 0, L1_w 0, SSIM_w 1, gradient 0.

Reference: truth() -- that definition as torch conv2d + autograd in double. The fp32 arm of a three-way comparison is the SAME model in float32 (the C oracle
has no weighted form); on `noise` content it is within 1e-6 (gradient, relative max-norm) and 4e-8 (loss) of the fp64 model at these shapes and patterns, far
inside the project's bars, which the kernels are therefore held to there: GRAD_TOL = 1e-4 and LOSS_TOL = 2e-6 (tests/loss_cases.py). On smooth_bright content, where fp32 cannot hold 1e-4, the
existing three-way rule applies: helpers.THREE_WAY_FACTOR x the float32 model's own error.

Everything "bit for bit" below is torch.equal on the outputs, after NaN has been excluded by an isfinite check."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import helpers
import loss_cases as base

LOSS_TOL, GRAD_TOL, DEFAULT_LAMBDAS, FORMS, LARGE = base.LOSS_TOL, base.GRAD_TOL, base.DEFAULT_LAMBDAS, base.FORMS, base.LARGE
# from loss_cases.SHAPES: inside the halo; one past both tilings; the halo crossing a tile edge; XCD bands with spare workgroups; one tile row
SHAPES = [(5, 7), (33, 65), (38, 70), (70, 100), (8, 300)]
assert all(s in base.SHAPES for s in SHAPES)
TRUTH_PATTERNS = ('soft', 'hole', 'blocks', 'one_pixel')
PATTERNS = ('ones',) + TRUTH_PATTERNS + ('zeros', 'negative_nan')
_id = lambda s: f'{s[0]}x{s[1]}'


@functools.lru_cache(maxsize=None)
def weight(shape: tuple, pattern: str) -> np.ndarray:
    """Seeded float32 [H,W] weights; once per process, read-only."""
    h, w = shape
    rng = np.random.default_rng(2000 + PATTERNS.index(pattern))
    soft = (2.0 * (1.0 - rng.random((h, w)))).astype(np.float32)                  # uniform in (0, 2]
    if pattern == 'ones':
        out = np.ones((h, w), np.float32)
    elif pattern == 'soft':
        out = soft
    elif pattern == 'hole':         # a zero rectangle over the middle half of each axis: 16 x 32 at 33 x 65 (columns 16 .. 47 straddle the forward tile edge at
        out = soft.copy()           # x = 32), wider than the 11-pixel window wherever the image is, so its core lies outside every window of a valid pixel
        out[h // 4:h - h // 4, w // 4:w - w // 4] = 0.0
    elif pattern == 'blocks':       # alternating 8 x 8 blocks of zero and random weights (the block at the origin is zero)
        out = np.where(base.equal_blocks(h, w), np.float32(0.0), soft)
        if not out.any():           # 5 x 7 is one block: keep its last row, so that S > 0
            out[-1] = soft[-1]
    elif pattern == 'one_pixel':    # S is the weight of ONE pixel, in the last (partial) tile
        out = np.zeros((h, w), np.float32)
        out[-1, -1] = 0.7
    elif pattern == 'zeros':
        out = np.zeros((h, w), np.float32)
    elif pattern == 'negative_nan':
        out = soft.copy()
        pick = rng.random((h, w))
        out[pick < 0.15] *= -1.0
        out[pick > 0.85] = np.nan
    else:
        raise KeyError(pattern)
    out = np.ascontiguousarray(out, np.float32)
    out.setflags(write=False)
    return out


def effective(w: np.ndarray) -> np.ndarray:
    w = np.asarray(w, np.float32)
    with np.errstate(invalid='ignore'):
        return np.where(w > 0, w, np.float32(0.0)).astype(np.float32)


def truth(x, y, w, lambda_l1: float = 0.8, lambda_dssim: float = 0.2, dtype=torch.float64):
    """The definition as torch conv2d + autograd in `dtype`: (loss, l1_w, ssim_w, dloss/dimage [3,H,W]). S must be > 0."""
    g = torch.tensor([np.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float64)
    g = g / g.sum()
    win = (g[:, None] * g[None, :])[None, None].expand(3, 1, 11, 11).contiguous().to(dtype)
    tx = torch.tensor(np.nan_to_num(np.asarray(x), nan=0.5), dtype=dtype, requires_grad=True)     # NaN written into ignored pixels would poison torch.where's gradient
    ty = torch.tensor(np.asarray(y), dtype=dtype)
    tw = torch.tensor(effective(w)).to(dtype)
    xp = torch.where(tw > 0, tx, ty)
    a, b = xp[None], ty[None]
    conv = lambda t: F.conv2d(t, win, padding=5, groups=3)
    mu1, mu2 = conv(a), conv(b)
    s11, s22, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    ssim_map = (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4)))[0]
    s = tw.sum()
    ssim = (tw * ssim_map).sum() / (3 * s)
    l1 = (tw * (xp - ty).abs()).sum() / (3 * s)
    loss = lambda_l1 * l1 + lambda_dssim * (1 - ssim)
    loss.backward()
    return float(loss.detach()), float(l1.detach()), float(ssim.detach()), tx.grad.numpy().astype(np.float64)


_REFERENCES: dict = {}


def references(shape: tuple, pattern: str, content: str = 'noise', lambdas: tuple = DEFAULT_LAMBDAS) -> dict:
    """truth() in double and in float32 of one case for upstream 1: once per process, shared, read-only."""
    key = (tuple(shape), pattern, content, tuple(float(v) for v in lambdas))
    if key not in _REFERENCES:
        x, y = base.pair(tuple(shape), content)
        w = weight(tuple(shape), pattern)
        t, m = truth(x, y, w, *lambdas), truth(x, y, w, *lambdas, dtype=torch.float32)
        t[3].setflags(write=False)
        m[3].setflags(write=False)
        _REFERENCES[key] = {'truth': t, 'model32': m}
    return _REFERENCES[key]


def _tensor(a, device) -> torch.Tensor:
    return torch.tensor(np.ascontiguousarray(a)).to(device)


def run(be, device, x, y, w, form: str = 'one_call', lambdas: tuple = DEFAULT_LAMBDAS, upstream: float | None = None) -> dict:
    """One of the three call forms with a weight (numpy array or tensor of any mask dtype): {'loss', 'means' (or None), 'grad'} on `device`."""
    tx, ty = _tensor(x, device), _tensor(y, device)
    tw = w.to(device) if isinstance(w, torch.Tensor) else _tensor(w, device)
    if form == 'one_call':
        assert upstream is None
        loss, grad, means = be.l1_dssim(tx, ty, *lambdas, with_grad=True, weight=tw)
    elif form == 'split':
        loss, means, scratch = be.l1_dssim_forward(tx, ty, *lambdas, weight=tw)
        up = None if upstream is None else torch.tensor(upstream, dtype=torch.float32, device=device)
        grad = be.l1_dssim_backward(tx, ty, scratch, up, *lambdas, weight=tw)
    elif form == 'autograd':
        with base.autograd_backend(be) as l1_dssim_loss:
            tx.requires_grad_(True)
            loss = l1_dssim_loss(tx, ty, *lambdas, weight=tw)
            (loss if upstream is None else upstream * loss).backward()
        loss, grad, means = loss.detach(), tx.grad, None
    else:
        raise KeyError(form)
    return {'loss': loss, 'means': means, 'grad': grad}


def same_bits(a: dict, b: dict, what) -> None:
    assert torch.equal(a['loss'], b['loss']), (what, 'loss', float(a['loss']), float(b['loss']))
    if a['means'] is not None and b['means'] is not None:
        assert torch.equal(a['means'], b['means']), (what, 'means')
    assert torch.equal(a['grad'], b['grad']), (what, 'gradient', float((a['grad'] - b['grad']).abs().max()))


def finite(out: dict, what) -> None:
    assert bool(torch.isfinite(out['loss'])) and bool(torch.isfinite(out['grad']).all()), (what, 'not finite')
    assert out['means'] is None or bool(torch.isfinite(out['means']).all()), (what, 'means not finite')


def check_against_truth(be, device, shape: tuple, pattern: str, form: str = 'one_call', content: str = 'noise', lambdas: tuple = DEFAULT_LAMBDAS,
                        upstream: float | None = None) -> dict:
    """One case through one call form against the fp64 model; every figure is printed and logged (FGS_TOL_LOG) before it is held to its bar."""
    shape = tuple(shape)
    x, y = base.pair(shape, content)
    w = weight(shape, pattern)
    ref = references(shape, pattern, content, lambdas)
    (t_loss, t_l1, t_ssim, t_grad), (m_loss, m_l1, m_ssim, m_grad) = ref['truth'], ref['model32']
    out = run(be, device, x, y, w, form, lambdas, upstream)
    up = 1.0 if upstream is None else float(upstream)
    label = f'weighted_{pattern}_{content}_{_id(shape)}_{form}'
    finite(out, label)
    grad = out['grad'].cpu().numpy()
    assert grad.shape == x.shape and grad.dtype == np.float32
    sums = [('loss', float(out['loss']), t_loss, m_loss)]
    if out['means'] is not None:
        sums += [('l1', float(out['means'][0]), t_l1, m_l1), ('ssim', float(out['means'][1]), t_ssim, m_ssim)]
    report = {name: (abs(k - t), abs(m - t)) for name, k, t, m in sums}
    e_k, e_m = helpers.rel_inf(grad, t_grad * up), helpers.rel_inf(m_grad * up, t_grad * up)
    report['rel_inf'] = (e_k, e_m)
    helpers.log_note('weighted_loss_case', label, **{k: f'({v[0]:.4g},{v[1]:.4g})' for k, v in report.items()})
    print(label, report)
    for name, _, _, _ in sums:
        e_kernel, e_model = report[name]
        assert e_kernel <= (LOSS_TOL if content == 'noise' else max(LOSS_TOL, helpers.THREE_WAY_FACTOR * e_model)), (label, name, report)
    assert e_k <= GRAD_TOL or (content != 'noise' and e_k <= helpers.THREE_WAY_FACTOR * e_m), (label, 'gradient, max-norm', report)
    assert np.all(grad[:, effective(w) == 0] == 0.0), (label, 'gradient where the weight does not count')
    return out


def check_forms_agree(be, device, shape: tuple, pattern: str = 'hole') -> None:
    """one_call, split and autograd: each against the fp64 model, all three bit for bit."""
    outs = {form: check_against_truth(be, device, shape, pattern, form) for form in FORMS}
    for form in ('split', 'autograd'):
        same_bits(outs[form], outs['one_call'], (shape, pattern, form))


def check_upstream_scalars(be, device, shape: tuple = (33, 65), pattern: str = 'blocks') -> None:
    """-0.37 as a device scalar to the backward call and through autograd; 3 * loss + loss.detach() through autograd."""
    check_against_truth(be, device, shape, pattern, 'split', upstream=-0.37)
    check_against_truth(be, device, shape, pattern, 'autograd', upstream=-0.37)
    x, y = base.pair(shape, 'noise')
    ref = references(shape, pattern)
    tx, ty, tw = _tensor(x, device).requires_grad_(True), _tensor(y, device), _tensor(weight(shape, pattern), device)
    with base.autograd_backend(be) as l1_dssim_loss:
        loss = l1_dssim_loss(tx, ty, weight=tw)
        total = 3.0 * loss + loss.detach()
        total.backward()
    e_k = helpers.rel_inf(tx.grad.cpu().numpy(), 3.0 * ref['truth'][3])
    print('composite', e_k, abs(float(loss.detach()) - ref['truth'][0]))
    assert float(total.detach()) == float(3.0 * loss.detach() + loss.detach())
    assert abs(float(loss.detach()) - ref['truth'][0]) <= LOSS_TOL and e_k <= GRAD_TOL


def run_unweighted(be, device, x, y, form: str) -> dict:
    return base.run(be, device, x, y, form)


def check_ones_equal_unweighted(be, device, shape: tuple, forms=FORMS) -> None:
    """Invariant 1: all-ones weights give the bits of the existing unweighted entry points (H W < 2^24), in every call form."""
    x, y = base.pair(tuple(shape), 'noise')
    for form in forms:
        a, b = run(be, device, x, y, weight(tuple(shape), 'ones'), form), run_unweighted(be, device, x, y, form)
        finite(a, (shape, form))
        same_bits(a, b, (shape, 'ones against the unweighted entry point', form))


def check_ignored_pixels(be, device, shape: tuple, pattern: str, form: str = 'one_call') -> None:
    """Invariants 2 and 3: the gradient is == 0.0 wherever the weight does not count, and NaN (or any other value) written into those pixels of the image
    changes no bit of loss, means and gradient, which stay finite."""
    x, y = base.pair(tuple(shape), 'noise')
    w = weight(tuple(shape), pattern)
    dead = effective(w) == 0
    assert dead.any() and not dead.all()
    plain = run(be, device, x, y, w, form)
    finite(plain, (shape, pattern, form))
    assert bool((plain['grad'].cpu()[:, torch.from_numpy(dead)] == 0.0).all()), (shape, pattern, form, 'gradient at ignored pixels')
    for fill in (np.nan, 1e30, -3.0):
        xn = np.array(x, copy=True)
        xn[:, dead] = fill
        same_bits(run(be, device, xn, y, w, form), plain, (shape, pattern, form, 'ignored pixels set to', fill))


def check_scale_invariance(be, device, shape: tuple, pattern: str = 'soft') -> None:
    """Invariant 4: weight and 4 * weight give identical bits."""
    x, y = base.pair(tuple(shape), 'noise')
    w = weight(tuple(shape), pattern)
    for form in ('one_call', 'split'):
        same_bits(run(be, device, x, y, 4.0 * w, form), run(be, device, x, y, w, form), (shape, pattern, form, 'x4'))


def check_negative_nan(be, device, shape: tuple) -> None:
    """Negative and NaN weights count as 0: the same bits as the run with those entries set to 0."""
    x, y = base.pair(tuple(shape), 'noise')
    w = weight(tuple(shape), 'negative_nan')
    assert np.isnan(w).any() and (w < 0).any()
    for form in ('one_call', 'split'):
        a = run(be, device, x, y, w, form)
        finite(a, (shape, form))
        same_bits(a, run(be, device, x, y, effective(w), form), (shape, form, 'negative / NaN weights'))


def check_zeros(be, device, shape: tuple) -> None:
    """S = 0: loss 0, means (0, 1), gradient all 0.0, everything finite -- in every call form."""
    x, y = base.pair(tuple(shape), 'noise')
    for form in FORMS:
        out = run(be, device, x, y, weight(tuple(shape), 'zeros'), form)
        finite(out, (shape, form))
        assert float(out['loss']) == 0.0, (shape, form, float(out['loss']))
        assert out['means'] is None or (float(out['means'][0]) == 0.0 and float(out['means'][1]) == 1.0), (shape, form)
        assert bool((out['grad'] == 0.0).all()), (shape, form)


def call_c_abi(be, device, x, y, w, fill: int, lambdas: tuple = DEFAULT_LAMBDAS):
    """fgs_l1_dssim_weighted_loss itself, on a scratch buffer whose every byte is `fill` on the way in: (sums [3], grad [3,H,W]) on `device`."""
    _, _backend = helpers.backend_modules()
    tx, ty, tw = _tensor(x, device), _tensor(y, device), _tensor(w, device)
    _, h, wd = tx.shape
    sums = torch.full((3,), float('nan'), dtype=torch.float32, device=device)
    grad = torch.full_like(tx, float('nan'))
    scratch = torch.full((int(be.lib.fgs_l1_dssim_weighted_scratch_bytes(wd, h)),), fill, dtype=torch.uint8, device=device)
    code = be.lib.fgs_l1_dssim_weighted_loss(tx.data_ptr(), ty.data_ptr(), tw.data_ptr(), wd, h, float(lambdas[0]), float(lambdas[1]), sums.data_ptr(),
                                             grad.data_ptr(), scratch.data_ptr(), _backend._stream_of(tx.device))
    assert code == 0, (code, be.lib.fgs_last_error())
    return sums, grad


def check_scratch_independence(be, device, shape: tuple, pattern: str = 'blocks') -> None:
    """Scratch of 0xFF bytes against scratch of zeros: every scratch word the kernels consume (the tiles' weight sums and S included) was produced by them."""
    x, y = base.pair(tuple(shape), 'noise')
    w = weight(tuple(shape), pattern)
    sums_ff, grad_ff = call_c_abi(be, device, x, y, w, 0xFF)
    sums_00, grad_00 = call_c_abi(be, device, x, y, w, 0x00)
    assert bool(torch.isfinite(sums_ff).all()) and bool(torch.isfinite(grad_ff).all()), shape
    assert torch.equal(sums_ff, sums_00) and torch.equal(grad_ff, grad_00), shape
    out = run(be, device, x, y, w)
    assert torch.equal(sums_ff[2], out['loss']) and torch.equal(sums_ff[:2], out['means']) and torch.equal(grad_ff, out['grad']), shape


def check_reproducible(be, device, shape: tuple, pattern: str = 'soft') -> None:
    x, y = base.pair(tuple(shape), 'noise')
    w = weight(tuple(shape), pattern)
    same_bits(run(be, device, x, y, w), run(be, device, x, y, w), (shape, 'two runs'))


def check_l1_term_alone(be, device, shape: tuple, form: str = 'one_call') -> None:
    """lambda = (1, 0) with a binary mask: +-lambda_l1 * w^ / (3 S) within 1 ulp on valid unequal pixels, 0.0 elsewhere."""
    x, y = base.pair(tuple(shape), 'noise')
    mask = (weight(tuple(shape), 'blocks') > 0).astype(np.float32)
    grad = run(be, device, x, y, mask, form, (1.0, 0.0))['grad'].cpu().numpy()
    assert np.isfinite(grad).all()
    valid = (mask > 0)[None] & (x != y)
    assert valid.any() and np.all(grad[~valid] == 0.0), (shape, form)
    expect = np.float32(1.0) / (np.float32(3.0) * np.float32(mask.sum()))
    want = np.where(x > y, expect, -expect).astype(np.float32)
    apart = base._ulp_apart(grad[valid], want[valid])
    assert int(apart.max()) <= 1, (shape, form, int(apart.max()))


def check_bool_mask(be, device, shape: tuple = (33, 65)) -> None:
    """A bool mask and an integer mask equal the same mask as float32, bit for bit, through autograd (harness.loss converts) and the Backend."""
    x, y = base.pair(tuple(shape), 'noise')
    mask = torch.from_numpy(weight(tuple(shape), 'hole') > 0)
    for form in ('autograd', 'one_call'):
        as_float = run(be, device, x, y, mask.to(torch.float32), form)
        same_bits(run(be, device, x, y, mask, form), as_float, (shape, form, 'bool'))
        same_bits(run(be, device, x, y, mask.to(torch.int64), form), as_float, (shape, form, 'int64'))


def check_refusals(be, device, other_device) -> None:
    """The C ABI refuses NULL weight / NULL pointers / non-positive sizes / a misaligned scratch with FGS_ERR_INVALID_ARGUMENT and a text; Backend refuses a
    weight of the wrong shape, rank or device with RuntimeError. Nothing is launched."""
    _, _backend = helpers.backend_modules()
    import pytest
    h, wd = 5, 7
    x, y = base.pair((h, wd), 'noise')
    tx, ty, tw = _tensor(x, device), _tensor(y, device), _tensor(weight((h, wd), 'soft'), device)
    sums, grad = torch.zeros(3, device=device), torch.zeros_like(tx)
    scratch = torch.zeros(int(be.lib.fgs_l1_dssim_weighted_scratch_bytes(wd, h)) + 8, dtype=torch.uint8, device=device)
    assert be.lib.fgs_l1_dssim_weighted_scratch_bytes(0, 5) == 0 and be.lib.fgs_l1_dssim_weighted_scratch_bytes(wd, h) > be.lib.fgs_l1_dssim_scratch_bytes(wd, h)
    stream = _backend._stream_of(tx.device)
    P = lambda t: t.data_ptr()
    good = dict(image=P(tx), target=P(ty), weight=P(tw), width=wd, height=h, out=P(sums), scratch=P(scratch))
    bad = [('weight', None, b'weight'), ('image', None, b'NULL'), ('target', None, b'NULL'), ('out', None, b'NULL'), ('scratch', None, b'NULL'),
           ('width', 0, b'size'), ('height', -3, b'size'), ('scratch', P(scratch) + 4, b'aligned')]
    for key, value, text in bad:
        a = dict(good, **{key: value})
        code = be.lib.fgs_l1_dssim_weighted_loss(a['image'], a['target'], a['weight'], a['width'], a['height'], 0.8, 0.2, a['out'], P(grad), a['scratch'], stream)
        assert code == -1 and text in be.lib.fgs_last_error(), ('loss', key, code, be.lib.fgs_last_error())
        a = dict(dict(good, out=P(grad)), **{key: value})
        code = be.lib.fgs_l1_dssim_weighted_backward(a['image'], a['target'], a['weight'], a['width'], a['height'], 0.8, 0.2, None, a['out'], a['scratch'], stream)
        assert code == -1 and text in be.lib.fgs_last_error(), ('backward', key, code, be.lib.fgs_last_error())
    for wrong in (tw[:-1], tw.t().contiguous(), tw[None], tw.reshape(-1), torch.zeros(h, wd, device=other_device), 1.0):
        with pytest.raises(RuntimeError, match='weight'):
            be.l1_dssim(tx, ty, weight=wrong)
        with pytest.raises(RuntimeError, match='weight'):
            be.l1_dssim_forward(tx, ty, weight=wrong)
    _, _, scratch_w = be.l1_dssim_forward(tx, ty, weight=tw)
    with pytest.raises(RuntimeError, match='weight'):
        be.l1_dssim_backward(tx, ty, scratch_w, weight=tw[:-1])
    _, _, scratch_u = be.l1_dssim_forward(tx, ty)
    with pytest.raises(RuntimeError, match='scratch'):                       # the unweighted scratch is too small for the weighted backward call
        be.l1_dssim_backward(tx, ty, scratch_u, weight=tw)
    with base.autograd_backend(be) as l1_dssim_loss:                          # the weight is not differentiable: no gradient reaches it
        tw_g = tw.clone().requires_grad_(True)
        l1_dssim_loss(tx.clone().requires_grad_(True), ty, weight=tw_g).backward()
        assert tw_g.grad is None


# ---- harness: training_iteration(..., loss_weight=) ------------------------------------------------------------------------------------------------
def _scene(device, n: int = 300):
    import bilagrid_cases
    T, g, view, _ = bilagrid_cases.training_pair(device, n=n)
    with torch.no_grad():
        rendered = T.render_image_training(g, view, False, view.background_color)
    gen = torch.Generator().manual_seed(23)
    target = (rendered.cpu() + 0.05 * torch.randn(rendered.shape, generator=gen)).clamp(0, 1).to(device)
    start = {k: getattr(g, k).detach().clone() for k in T.PARAM_ORDER}

    def fresh():
        gg = T.Gaussians({k: v.clone() for k, v in start.items()}, torch.device(device))
        gg.training_setup(training_cameras_extent=4.0)
        return gg
    return T, view, target, fresh


def check_training_iteration_ones(device, steps: int, exact_parameters: bool) -> None:
    """loss_weight = ones equals the step without it: the loss returned by the first step bit for bit; with exact_parameters (the simulation, where the
    rasterizer is deterministic) also every parameter after `steps` steps, on each branch (plain, depth, absgrad)."""
    T, view, target, fresh = _scene(device)
    ones = torch.ones(view.height, view.width, device=device)
    depth_target = torch.full((view.height, view.width), 3.0, device=device)
    for kw in ({}, {'depth_target': depth_target, 'depth_weight': 0.5}, {'absgrad': True}):
        ga, gb = fresh(), fresh()
        la = [T.training_iteration(ga, view, target, it, **kw) for it in range(steps)]
        lb = [T.training_iteration(gb, view, target, it, loss_weight=ones, **kw) for it in range(steps)]
        assert torch.equal(la[0], lb[0]), (kw.keys(), float(la[0]), float(lb[0]))
        if exact_parameters:
            for k in T.PARAM_ORDER:
                assert torch.equal(getattr(ga, k), getattr(gb, k)), (kw.keys(), k)


def check_training_iteration_hole(device) -> None:
    """With a hole mask the gradient that reaches the rendered image is 0.0 on the hole and not elsewhere; the step is finite and moves the parameters."""
    T, view, target, fresh = _scene(device)
    g = fresh()
    mask = torch.ones(view.height, view.width, dtype=torch.bool, device=device)
    mask[view.height // 4:view.height - view.height // 4, view.width // 4:view.width - view.width // 4] = False
    seen = {}

    def loss_fn(image, target, weight=None):
        image.register_hook(lambda grad: seen.__setitem__('grad', grad.detach().clone()))
        return T.photometric_loss(image, target, weight=weight)
    before = g.means.detach().clone()
    loss = T.training_iteration(g, view, target, 0, loss_fn=loss_fn, loss_weight=mask)
    assert bool(torch.isfinite(loss)) and not torch.equal(g.means, before)
    grad = seen['grad']
    assert bool(torch.isfinite(grad).all()) and bool((grad[:, ~mask] == 0.0).all()) and bool((grad[:, mask] != 0.0).any())


def check_training_iteration_bilagrid(device) -> None:
    """The bilagrid path takes loss_weight: the CORRECTED image is weighted (ones: the loss of the step without a weight, bit for bit), a hole mask gives
    a finite step."""
    from harness.bilagrid import BilateralGrids
    T, view, target, fresh = _scene(device)

    def step(weight):
        g = fresh()
        m = BilateralGrids(1, shape=(4, 4, 2), device=device)
        m.training_setup()
        return T.training_iteration(g, view, target, 0, bilagrid=m, view_index=0, loss_weight=weight), m
    plain, _ = step(None)
    ones, _ = step(torch.ones(view.height, view.width, device=device))
    assert torch.equal(plain, ones), (float(plain), float(ones))
    mask = torch.ones(view.height, view.width, device=device)
    mask[: view.height // 2] = 0.0
    holed, m = step(mask)
    assert bool(torch.isfinite(holed)) and not torch.equal(holed, plain)
    assert bool(torch.isfinite(m.grids[0]).all())
