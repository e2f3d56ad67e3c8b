"""Shapes, contents, fp64 reference and comparisons shared by tests/test_loss.py (CPU simulation) and tests/test_gpu_loss.py (MI355X): the fused
L1 + DSSIM loss (csrc/loss.hip: ssim_forward_kernel, ssim_backward_kernel, ssim_reduce_kernel) through its three call forms.

Reference: truth() -- the published SSIM of 3D Gaussian Splatting as torch conv2d + autograd in double, independent of the derivative algebra that the
fp32 oracle (oracle/fgs_oracle.c: orc_l1_dssim) and the kernels share. Both fp32 results are measured against it (three-way): on smooth bright content
s11 = m11 - mu1^2 cancels against C2 = 9e-4 and the fp32 ORACLE is 1.5e-4 to 2.9e-4 (rel_inf) off the fp64 gradient, so "1e-4 against the oracle" holds
on noise only.

Shapes: the forward kernel filters 32 x 32 tiles, the backward kernel 64 x 32; both deal their tiles to 8 XCD bands of ceil(tiles / 8) with spare
workgroups. SHAPES are the smallest images that reach each edge of either tiling (the table beside it).

Bars (none comes from the kernels' own output):
  loss, l1, ssim      |kernel - truth| <= max(2e-6, THREE_WAY_FACTOR * |oracle32 - truth|); 2e-6 is the bar the GPU test of the loss always had
  gradient, max-norm  rel_inf(kernel, truth) <= 1e-4 (the fp32 bar of BASELINE.json), or <= THREE_WAY_FACTOR * rel_inf(oracle32, truth)
  gradient, by entry  helpers.elementwise_three_way / three_way_ok
  half_equal          with lambda_dssim = 0 the gradient is == 0.0 where target == image and +-lambda_l1 * upstream / n within 1 ulp elsewhere
  equal               truth is ~1e-16, so absolute: loss == 0, l1 == 0, |ssim - 1| <= 1e-6, n * max|grad| <= 4 x the oracle's and <= 1e-4 * lambda_l1
                      (a wrong sign term alone would give lambda_l1)"""
from __future__ import annotations

import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

import helpers

LOSS_TOL = 2e-6
GRAD_TOL = 1e-4
EQUAL_SSIM_TOL = 1e-6
EQUAL_GRAD_FACTOR = 4.0
EQUAL_GRAD_CONDITION = 1e-4
DEFAULT_LAMBDAS = (0.8, 0.2)

# (H, W)                what it reaches
SHAPES = [
    (1, 1), (5, 7), (11, 11),     # inside the 5-pixel halo; 3 H W odd, so the partial sums start one float behind the maps (LossScratch::partials_at)
    (32, 32), (33, 33),           # exactly one forward tile; one past
    (32, 64), (33, 65),           # exactly one backward tile; one past both tilings
    (38, 70),                     # 6 px past a tile edge: the halo just crosses it
    (70, 100),                    # forward 36 workgroups, per_xcd 5, last band holds 1; backward 18, per_xcd 3, XCDs 6 and 7 empty; bands split mid-row / mid-channel
    (8, 300), (300, 8),           # one tile row; one tile column
]
FORM_SHAPES = [(33, 65), (70, 100), (8, 300)]
CONTENT_SHAPES = [(5, 7), (33, 65), (70, 100)]
CONTENTS = ('noise', 'smooth_bright', 'blocks', 'overrange', 'black', 'half_equal', 'equal')
FORMS = ('one_call', 'split', 'autograd')
LARGE = (360, 640)


def noise_pair(h: int, w: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    x = rng.random((3, h, w)).astype(np.float32)
    y = np.clip(x + 0.1 * rng.standard_normal((3, h, w)).astype(np.float32), 0, 1).astype(np.float32)
    return x, y


def equal_blocks(h: int, w: int) -> np.ndarray:
    """[H,W] bool: the alternating 8 x 8 blocks on which half_equal's target IS the image (the block at the origin is one: 5 x 7 is all equal)."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return ((yy // 8 + xx // 8) % 2) == 0


@functools.lru_cache(maxsize=None)
def pair(shape: tuple, content: str):
    """Seeded float32 (image, target), [3,H,W] each; once per process, read-only."""
    h, w = shape
    rng = np.random.default_rng(1000 + CONTENTS.index(content))
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    if content == 'noise':
        x, y = noise_pair(h, w, seed=7)
    elif content == 'smooth_bright':                      # what a trained render looks like: 0.8 .. 1.0, the target a few thousandths away
        base = 0.9 + 0.1 * np.sin(xx / 17.0) * np.cos(yy / 13.0)
        x = np.stack([base, 0.98 * base, 0.95 * base])
        y = x + 0.004 * rng.standard_normal((3, h, w))
    elif content == 'blocks':                             # hard 0 / 1 edges: cells 6 px wide, 5 px high; the target is the 1-px shift, compressed
        board = (((xx // 6) + (yy // 5)) % 2).astype(np.float64)
        x = np.stack([board, board, board])
        y = np.roll(x, (1, 1), axis=(1, 2)) * 0.9 + 0.05
    elif content == 'overrange':
        x, y = 1.8 * rng.random((3, h, w)), rng.random((3, h, w))
    elif content == 'black':
        x = np.zeros((3, h, w))
        y = 0.002 * rng.random((3, h, w))
        y[:, :h // 2] = 0.0
    elif content == 'half_equal':
        x, y = noise_pair(h, w, seed=8)
        y = np.where(equal_blocks(h, w)[None], x, y)
    elif content == 'equal':
        x, _ = noise_pair(h, w, seed=9)
        y = x
    else:
        raise KeyError(content)
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def is_equal_case(shape: tuple, content: str) -> bool:
    x, y = pair(shape, content)
    return bool(np.array_equal(x, y))


def truth(x, y, lambda_l1: float = 0.8, lambda_dssim: float = 0.2):
    """fp64 torch conv2d + autograd model of lambda_l1 * L1 + lambda_dssim * (1 - SSIM): (loss, l1, ssim, dloss/dimage [3,H,W] float64)."""
    g = torch.tensor([np.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float64)
    g = g / g.sum()
    w = (g[:, None] * g[None, :])[None, None].expand(3, 1, 11, 11).contiguous()
    tx = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    ty = torch.tensor(np.asarray(y), dtype=torch.float64)
    a, b = tx[None], ty[None]
    conv = lambda t: F.conv2d(t, w, padding=5, groups=3)
    mu1, mu2 = conv(a), conv(b)
    s11, s22, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    ssim = (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))).mean()
    l1 = (tx - ty).abs().mean()
    loss = lambda_l1 * l1 + lambda_dssim * (1 - ssim)
    loss.backward()
    return float(loss.detach()), float(l1.detach()), float(ssim.detach()), tx.grad.numpy()


_REFERENCES: dict = {}


def references(oracle, shape: tuple, content: str, lambdas: tuple = DEFAULT_LAMBDAS) -> dict:
    """truth() and the fp32 oracle (oracle.l1_dssim) of one case for upstream 1: once per process, shared, read-only."""
    key = (tuple(shape), content, tuple(float(v) for v in lambdas))
    if key not in _REFERENCES:
        x, y = pair(tuple(shape), content)
        t, o = truth(x, y, *lambdas), oracle.l1_dssim(x, y, *lambdas)
        t[3].setflags(write=False)
        o[3].setflags(write=False)
        _REFERENCES[key] = {'truth': t, 'oracle': o}
    return _REFERENCES[key]


@contextlib.contextmanager
def autograd_backend(be):
    """harness.loss reaches the backend through default_backend(): `be` for the duration (the simulation on the CPU; on the device it is `be` anyway)."""
    helpers.backend_modules()
    import harness.loss as L
    saved = L.default_backend
    L.default_backend = lambda: be
    try:
        yield L.l1_dssim_loss
    finally:
        L.default_backend = saved


def _tensor(a, device) -> torch.Tensor:
    return torch.tensor(np.ascontiguousarray(a)).to(device)          # a copy: the cases' arrays are read-only


def _log(kind: str, label: str, report: dict) -> None:
    """One FGS_TOL_LOG line per case: pairs are (kernel, fp32 oracle) against fp64; elementwise = (fraction kernel, fraction oracle, entries)."""
    fmt = lambda v: '(' + ','.join(fmt(e) for e in v) + ')' if isinstance(v, tuple) else (f'{v:.4g}' if isinstance(v, float) else str(v))
    helpers.log_note(kind, label, **{k: fmt(v) for k, v in report.items() if k != 'label'})


def run(be, device, x, y, form: str = 'one_call', lambdas: tuple = DEFAULT_LAMBDAS, upstream: float | None = None) -> dict:
    """One of the three call forms: {'loss': 0-dim tensor, 'means': (l1, ssim) tensor or None, 'grad': [3,H,W] tensor}, all on `device`.
    `upstream` (None = 1): 'split' hands it to l1_dssim_backward as a device scalar, 'autograd' multiplies the loss by it; 'one_call' has none."""
    tx, ty = _tensor(x, device), _tensor(y, device)
    if form == 'one_call':
        assert upstream is None, 'l1_dssim(with_grad=True) has no upstream scalar'
        loss, grad, means = be.l1_dssim(tx, ty, *lambdas, with_grad=True)
    elif form == 'split':
        loss, means, scratch = be.l1_dssim_forward(tx, ty, *lambdas)
        up = None if upstream is None else torch.tensor(upstream, dtype=torch.float32, device=device)
        grad = be.l1_dssim_backward(tx, ty, scratch, up, *lambdas)
    elif form == 'autograd':
        with autograd_backend(be) as l1_dssim_loss:
            tx.requires_grad_(True)
            loss = l1_dssim_loss(tx, ty, *lambdas)
            (loss if upstream is None else upstream * loss).backward()
        loss, grad, means = loss.detach(), tx.grad, None
    else:
        raise KeyError(form)
    return {'loss': loss, 'means': means, 'grad': grad}


def _ulp_apart(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in float32 steps between two float32 arrays of one sign pattern."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_l1_term_alone(be, device, shape: tuple, content: str, form: str, lambda_l1: float, upstream: float | None) -> None:
    """lambda_dssim = 0: the gradient is the L1 term and nothing else -- exactly 0.0 where target == image, +-lambda_l1 * upstream / n within 1 ulp elsewhere."""
    x, y = pair(shape, content)
    grad = run(be, device, x, y, form, (lambda_l1, 0.0), upstream)['grad'].cpu().numpy()
    assert np.isfinite(grad).all(), (shape, content, form)
    same = x == y
    assert np.all(grad[same] == 0.0), (shape, content, form, 'L1 term on equal pixels', float(np.abs(grad[same]).max()))
    expect = np.float32(np.float32(lambda_l1) / np.float32(x.size) * np.float32(1.0 if upstream is None else upstream))
    want = np.where(x > y, expect, -expect).astype(np.float32)
    apart = _ulp_apart(grad[~same], want[~same])
    assert apart.size == 0 or int(apart.max()) <= 1, (shape, content, form, 'L1 term, float32 steps from +-lambda_l1 * upstream / n', int(apart.max()))


def check_against_truth(be, oracle, device, shape: tuple, content: str = 'noise', form: str = 'one_call', lambdas: tuple = DEFAULT_LAMBDAS,
                        upstream: float | None = None) -> dict:
    """One case through one call form against the fp64 model and the fp32 oracle; every figure is logged (FGS_TOL_LOG) and printed before it is held to its
    bar. Returns run()'s dictionary, for the bit-for-bit comparisons between forms."""
    shape = tuple(shape)
    x, y = pair(shape, content)
    n = x.size
    ref = references(oracle, shape, content, lambdas)
    (t_loss, t_l1, t_ssim, t_grad), (o_loss, o_l1, o_ssim, o_grad) = ref['truth'], ref['oracle']
    out = run(be, device, x, y, form, lambdas, upstream)
    up = 1.0 if upstream is None else float(upstream)
    grad = out['grad'].cpu().numpy()
    assert grad.shape == x.shape and grad.dtype == np.float32
    label = f'{content}_{shape[0]}x{shape[1]}_{form}'
    report = {'label': label, 'lambdas': tuple(lambdas), 'upstream': up}
    assert np.isfinite(grad).all(), (label, 'gradient not finite')
    k_loss = float(out['loss'])
    sums = [('loss', k_loss, t_loss, o_loss)]
    if out['means'] is not None:
        sums += [('l1', float(out['means'][0]), t_l1, o_l1), ('ssim', float(out['means'][1]), t_ssim, o_ssim)]
    for name, k, t, o in sums:
        report[name] = (abs(k - t), abs(o - t))

    if is_equal_case(shape, content):
        lambda_l1 = float(lambdas[0])
        assert lambda_l1 > 0.0, 'the condition of the equal case needs an L1 term'
        report['n_max_grad'] = (float(n * np.abs(grad).max()), float(n * np.abs(o_grad).max() * abs(up)))
        _log('loss_case_equal', label, report)
        print(report)
        assert k_loss == 0.0, (label, report)
        if out['means'] is not None:
            assert float(out['means'][0]) == 0.0 and abs(float(out['means'][1]) - 1.0) <= EQUAL_SSIM_TOL, (label, report)
        assert report['n_max_grad'][0] <= EQUAL_GRAD_FACTOR * report['n_max_grad'][1], (label, report)
        assert report['n_max_grad'][0] <= EQUAL_GRAD_CONDITION * lambda_l1 * abs(up), (label, report)
        return out

    tg, og = t_grad * up, o_grad.astype(np.float64) * up
    e_k, e_o = helpers.rel_inf(grad, tg), helpers.rel_inf(og, tg)
    fh, fo, entries = helpers.elementwise_three_way(grad, og, tg, kind='loss_' + label)
    report.update(rel_inf=(e_k, e_o), elementwise=(fh, fo, entries), three_way_ratio=(fh / fo if fo > 0 else 0.0))
    _log('loss_case', label, report)
    print(report)
    for name, _, _, _ in sums:
        e_kernel, e_oracle = report[name]
        assert e_kernel <= max(LOSS_TOL, helpers.THREE_WAY_FACTOR * e_oracle), (label, name, report)
    assert e_k <= GRAD_TOL or e_k <= helpers.THREE_WAY_FACTOR * e_o, (label, 'gradient, max-norm', report)
    assert helpers.three_way_ok(fh, fo, entries), (label, 'gradient, element-wise 1e-4 three-way', report)
    if content == 'half_equal':
        check_l1_term_alone(be, device, shape, content, form, float(lambdas[0]) or DEFAULT_LAMBDAS[0], upstream)
    return out


def check_forms_agree(be, oracle, device, shape: tuple) -> None:
    """one_call, split and autograd with upstream 1 on noise: each against the fp64 model, and all three bit for bit in loss and gradient."""
    outs = {form: check_against_truth(be, oracle, device, shape, 'noise', form) for form in FORMS}
    for form in ('split', 'autograd'):
        assert torch.equal(outs[form]['loss'], outs['one_call']['loss']), (shape, form, 'loss')
        assert torch.equal(outs[form]['grad'], outs['one_call']['grad']), (shape, form, 'gradient')
    assert torch.equal(outs['split']['means'], outs['one_call']['means']), (shape, 'means')


def check_composite_graph(be, oracle, device, shape: tuple) -> None:
    """3 * loss + loss.detach(): the upstream scalar autograd hands the node is 3, and nothing of the detached branch reaches the gradient."""
    x, y = pair(shape, 'noise')
    ref = references(oracle, shape, 'noise')
    tx, ty = _tensor(x, device).requires_grad_(True), _tensor(y, device)
    with autograd_backend(be) as l1_dssim_loss:
        loss = l1_dssim_loss(tx, ty)
        total = 3.0 * loss + loss.detach()
        total.backward()
    grad = tx.grad.cpu().numpy()
    tg, og = 3.0 * ref['truth'][3], 3.0 * ref['oracle'][3].astype(np.float64)
    e_k, e_o = helpers.rel_inf(grad, tg), helpers.rel_inf(og, tg)
    fh, fo, entries = helpers.elementwise_three_way(grad, og, tg, kind=f'loss_composite_{shape[0]}x{shape[1]}')
    report = {'rel_inf': (e_k, e_o), 'elementwise': (fh, fo, entries), 'loss': (abs(float(loss.detach()) - ref['truth'][0]), abs(ref['oracle'][0] - ref['truth'][0]))}
    _log('loss_case', f'composite_{shape[0]}x{shape[1]}_autograd', report)
    print(report)
    assert np.isfinite(grad).all()
    assert float(total.detach()) == float(3.0 * loss.detach() + loss.detach())
    assert report['loss'][0] <= max(LOSS_TOL, helpers.THREE_WAY_FACTOR * report['loss'][1]), report
    assert e_k <= GRAD_TOL or e_k <= helpers.THREE_WAY_FACTOR * e_o, report
    assert helpers.three_way_ok(fh, fo, entries), report


def check_non_contiguous(be, device, shape: tuple) -> None:
    """l1_dssim_loss on a [H,W,3] tensor permuted to [3,H,W]: loss and gradient equal the contiguous call's bit for bit, image.grad has the image's shape."""
    x, y = pair(shape, 'noise')
    ty = _tensor(y, device)
    with autograd_backend(be) as l1_dssim_loss:
        plain = _tensor(x, device).requires_grad_(True)
        loss_plain = l1_dssim_loss(plain, ty)
        loss_plain.backward()
        hwc = _tensor(np.moveaxis(np.asarray(x), 0, -1), device).requires_grad_(True)
        image = hwc.permute(2, 0, 1)
        assert not image.is_contiguous() and image.shape == plain.shape
        image.retain_grad()
        loss = l1_dssim_loss(image, ty)
        loss.backward()
    assert torch.equal(loss.detach(), loss_plain.detach())
    assert image.grad.shape == image.shape and torch.equal(image.grad, plain.grad)
    assert hwc.grad.shape == hwc.shape and torch.equal(hwc.grad.permute(2, 0, 1), plain.grad)


def call_c_abi(be, device, x, y, fill: int, lambdas: tuple = DEFAULT_LAMBDAS):
    """fgs_l1_dssim_loss itself, on a scratch buffer whose every byte is `fill` on the way in: (sums [3], grad [3,H,W]) on `device`."""
    _, _backend = helpers.backend_modules()
    tx, ty = _tensor(x, device), _tensor(y, device)
    _, h, w = tx.shape
    sums = torch.full((3,), float('nan'), dtype=torch.float32, device=device)
    grad = torch.full_like(tx, float('nan'))
    scratch = torch.full((int(be.lib.fgs_l1_dssim_scratch_bytes(w, h)),), fill, dtype=torch.uint8, device=device)
    code = be.lib.fgs_l1_dssim_loss(tx.data_ptr(), ty.data_ptr(), w, h, float(lambdas[0]), float(lambdas[1]), sums.data_ptr(), grad.data_ptr(),
                                    scratch.data_ptr(), _backend._stream_of(tx.device))
    assert code == 0, code
    return sums, grad


def check_scratch_independence(be, device, shape: tuple) -> None:
    """Scratch of 0xFF bytes (NaN as floats) against scratch of zeros: every scratch word the kernels consume was first produced by them -- the partial
    sums of every tile the reduction runs over included -- so sums and gradient are the same bits."""
    x, y = pair(shape, 'noise')
    sums_ff, grad_ff = call_c_abi(be, device, x, y, 0xFF)
    sums_00, grad_00 = call_c_abi(be, device, x, y, 0x00)
    assert bool(torch.isfinite(sums_ff).all()) and bool(torch.isfinite(grad_ff).all()), shape
    assert torch.equal(sums_ff, sums_00) and torch.equal(grad_ff, grad_00), shape
    loss, grad, means = be.l1_dssim(_tensor(x, device), _tensor(y, device))
    assert torch.equal(sums_ff[2], loss) and torch.equal(sums_ff[:2], means) and torch.equal(grad_ff, grad), shape


def check_reproducible(be, device, shape: tuple, content: str = 'noise') -> None:
    """loss.hip promises a fixed reduction order: two runs of one input give the same bits in sums and gradient."""
    x, y = pair(shape, content)
    a, b = run(be, device, x, y), run(be, device, x, y)
    assert torch.equal(a['loss'], b['loss']) and torch.equal(a['means'], b['means']) and torch.equal(a['grad'], b['grad']), shape
