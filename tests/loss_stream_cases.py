"""Shapes and checks of the STREAMING loss kernels (csrc/loss.hip), shared by tests/test_loss_stream.py (CPU simulation) and
tests/test_gpu_loss_stream.py (MI355X). The reference (loss_cases.truth, fp64 conv2d + autograd), the contents and every bar are those of
tests/loss_cases.py and tests/weighted_loss_cases.py, unchanged; only the shapes are new: the smallest images that reach each edge of the new geometry.

Geometry: a wave owns a strip of S = 64 columns of one channel and a band of B output rows (forward B_FWD, backward B_BWD), walks input rows
y0 - 5 .. y1 + 4, keeps 11 horizontally filtered rows in a register ring and emits an output row from the 11th input row on. Four consecutive
(channel, band, strip) units share a workgroup; workgroups are dealt to 8 XCD regions of ceil(groups / 8), the spare ones return at once.

  widths   1, 5, 6 (inside the halo; the right halo lanes just start to load), S - 1, S, S + 1 (one strip; one column into the next), S + 5, S + 6 (the
           next strip's left halo is all image; one past), 2 S + 1 (three strips)
  heights  1, 5, 6, 10, 11 (the ring just fills: 11 input rows are all image only from H = 11 on), B - 1, B, B + 1, B + 5, B + 6 (the next band's upper halo is
           all image; one past), 2 B + 1 (three bands)
paired so that no case exceeds (2 B + 1) x (2 S + 1).

Streaming against tiled (the dev switch, option 16: bit 0 the tiled forward kernel, bit 1 the tiled backward kernel of csrc/loss_exhibits.hip): both forms
sum the taps of both passes from t = 0 to 10 into 0.0f through one explicit fused multiply-add (fgs_loss.h: tap) and share the per-pixel algebra
(ssim_point, loss_gradient), so the three derivative maps and the unweighted gradient are held to ZERO units in the last place, element by element. The weighted
gradient is divided by 3 S, and S is a sum over the forward kernel's units, whose order differs between the forms (last-bit differences of S were measured
at 1080p: profiles/loss_streaming.txt): it is held to zero where S is the same number, i.e. between the two BACKWARD kernels behind one forward kernel, for
both forward kernels. The loss scalars differ by summation order only and are each held to truth."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import loss_cases as base
import weighted_loss_cases as wcases

S = 64
B_FWD = 24          # csrc/loss.hip: FGS_LOSS_BAND_H
B_BWD = 24          # csrc/loss.hip: FGS_LOSS_BWD_BAND_H
LOSS_FORM_OPTION = 16
TILED_FORWARD, TILED_BACKWARD = 1, 2

WIDTHS = [1, 5, 6, S - 1, S, S + 1, S + 5, S + 6, 2 * S + 1]


def band_heights(b: int) -> list:
    return [1, 5, 6, 10, 11, b - 1, b, b + 1, b + 5, b + 6, 2 * b + 1]


def _pairs() -> list:
    heights = band_heights(B_FWD) + [h for h in band_heights(B_BWD) if h not in band_heights(B_FWD)]
    # every height once and every width at least once: the widths are walked round, the tallest cases get the widest images
    out = [(h, WIDTHS[(i * 4 + 3) % len(WIDTHS)]) for i, h in enumerate(sorted(heights))]
    assert {w for _, w in out} == set(WIDTHS) and {h for h, _ in out} == set(heights)
    return out


def units(shape: tuple, b: int) -> int:
    h, w = shape
    return 3 * ((w + S - 1) // S) * ((h + b - 1) // b)


def groups(shape: tuple, b: int) -> int:
    return (units(shape, b) + 3) // 4


SHAPES = _pairs()
# 3 strips x 3 bands x 3 channels = 27 units = 7 workgroups: not a multiple of 8 (one spare workgroup, XCD regions of 1 with the last one empty), and the last
# workgroup has one spare wave
UNEVEN = (2 * B_FWD + 1, 2 * S + 1)
# 3 H W odd puts the partial sums one float behind the maps (LossScratch::partials_at)
ODD = (11, S + 1)
EXTRA = [s for s in (UNEVEN, ODD) if s not in SHAPES]
ALL_SHAPES = SHAPES + EXTRA
assert groups(UNEVEN, B_FWD) % 8 != 0 and groups(UNEVEN, B_BWD) % 8 != 0 and units(UNEVEN, B_FWD) % 4 != 0
assert (3 * ODD[0] * ODD[1]) % 2 == 1
assert all(h <= 2 * max(B_FWD, B_BWD) + 1 and w <= 2 * S + 1 for h, w in ALL_SHAPES)
# the comparisons between formulations: a shape inside the halo, one that crosses a strip and a band edge by one, and the uneven one
FORMULATION_SHAPES = [(5, 6), (max(B_FWD, B_BWD) + 1, S + 1), UNEVEN]
shape_id = lambda s: f'{s[0]}x{s[1]}'


def bad_weight(shape: tuple) -> np.ndarray:
    """weighted_loss_cases' soft weights with every 3rd entry 0, every 5th negative and every 7th NaN (flat index, from 1: entry 0 always counts)."""
    w = np.array(wcases.weight(tuple(shape), 'soft'), copy=True)
    flat = w.reshape(-1)
    idx = np.arange(flat.size)
    flat[(idx % 3 == 2)] = 0.0
    flat[(idx % 5 == 4)] *= -1.0
    flat[(idx % 7 == 6)] = np.nan
    return w


def check_shape(be, oracle, device, shape: tuple) -> None:
    """Everything the edge table asks of one shape: the three call forms against the fp64 model and bit for bit among themselves; all-ones weights against
    the unweighted entry points; zero, negative and NaN weights; two runs bit for bit."""
    shape = tuple(shape)
    base.check_forms_agree(be, oracle, device, shape)
    wcases.check_ones_equal_unweighted(be, device, shape)
    wcases.check_zeros(be, device, shape)
    x, y = base.pair(shape, 'noise')
    w = bad_weight(shape)
    eff = wcases.effective(w)
    for form in ('one_call', 'split'):
        a = wcases.run(be, device, x, y, w, form)
        wcases.finite(a, (shape, form))
        wcases.same_bits(a, wcases.run(be, device, x, y, eff, form), (shape, form, 'zero / negative / NaN weights'))
        grad = a['grad'].cpu().numpy()
        assert np.all(grad[:, eff == 0] == 0.0), (shape, form, 'gradient where the weight does not count')
    t_loss, _, _, t_grad = wcases.truth(x, y, w)
    import helpers
    e_loss, e_grad = abs(float(a['loss']) - t_loss), helpers.rel_inf(grad, t_grad)
    print('weighted', shape_id(shape), {'loss': e_loss, 'rel_inf': e_grad})
    assert e_loss <= wcases.LOSS_TOL and e_grad <= wcases.GRAD_TOL, (shape, e_loss, e_grad)
    base.check_reproducible(be, device, shape)
    wcases.check_reproducible(be, device, shape)


@contextlib.contextmanager
def loss_form(be, value: int):
    """The dev library's option 16 for the duration; the product's kernels (0) afterwards."""
    assert be.lib.fgs_debug_set_option(LOSS_FORM_OPTION, value) == 0, be.lib.fgs_last_error()
    try:
        yield
    finally:
        be.lib.fgs_debug_set_option(LOSS_FORM_OPTION, 0)


def _ulp_apart(a: torch.Tensor, b: torch.Tensor) -> int:
    """The worst distance in float32 steps between two finite float32 tensors (0 where the bits are equal, +0.0 and -0.0 included as 0 apart)."""
    ia, ib = a.cpu().contiguous().view(torch.int32).to(torch.int64), b.cpu().contiguous().view(torch.int32).to(torch.int64)
    ia, ib = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia), torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)      # sign-magnitude -> a line
    return int((ia - ib).abs().max()) if ia.numel() else 0


def _maps(scratch: torch.Tensor, shape: tuple) -> torch.Tensor:
    """The three derivative maps a forward call left at the head of its scratch: [3, 3, H, W] float32."""
    h, w = shape
    return scratch[:4 * 9 * h * w].view(torch.float32).view(3, 3, h, w).clone()


def check_streaming_against_tiled(be, oracle, device, shape: tuple, content: str = 'noise') -> dict:
    """The derivative maps of both forward kernels (unweighted and weighted) and the gradients of both backward kernels from the SAME maps, element by
    element: zero float32 steps apart. Each formulation's loss scalars are held to truth by the bar of loss_cases (2e-6 or three-way)."""
    import helpers
    shape = tuple(shape)
    x, y = base.pair(shape, content)
    tx, ty = base._tensor(x, device), base._tensor(y, device)
    tw = base._tensor(wcases.weight(shape, 'soft'), device)
    ref = base.references(oracle, shape, content)
    worst = {}
    out = {}
    for name, value in (('streaming', 0), ('tiled', TILED_FORWARD | TILED_BACKWARD)):
        with loss_form(be, value):
            loss, means, scratch = be.l1_dssim_forward(tx, ty)
            grad = be.l1_dssim_backward(tx, ty, scratch)
            _, _, wscratch = be.l1_dssim_forward(tx, ty, weight=tw)
            wgrad = be.l1_dssim_backward(tx, ty, wscratch, weight=tw)
            out[name] = {'loss': float(loss), 'means': means.cpu(), 'maps': _maps(scratch, shape), 'grad': grad.cpu(), 'wmaps': _maps(wscratch, shape),
                         'wgrad': wgrad.cpu()}
    # the tiled backward kernel behind the streaming forward kernel (a), and the other way round (b): the same maps and, weighted, the same S
    for name, value in (('mixed_a', TILED_BACKWARD), ('mixed_b', TILED_FORWARD)):
        with loss_form(be, value):
            _, _, scratch = be.l1_dssim_forward(tx, ty)
            _, _, wscratch = be.l1_dssim_forward(tx, ty, weight=tw)
            out[name] = {'grad': be.l1_dssim_backward(tx, ty, scratch).cpu(), 'wgrad': be.l1_dssim_backward(tx, ty, wscratch, weight=tw).cpu()}
    for key in ('maps', 'wmaps', 'grad'):
        assert bool(torch.isfinite(out['streaming'][key]).all()), (shape, key)
        worst[key] = _ulp_apart(out['streaming'][key], out['tiled'][key])
    worst['grad_mixed'] = max(_ulp_apart(out['streaming']['grad'], out['mixed_a']['grad']), _ulp_apart(out['streaming']['grad'], out['mixed_b']['grad']))
    assert bool(torch.isfinite(out['streaming']['wgrad']).all()) and bool(torch.isfinite(out['tiled']['wgrad']).all()), (shape, 'wgrad')
    # weighted: streaming forward + {streaming, tiled} backward share one S; tiled forward + {tiled, streaming} backward share the other
    worst['wgrad_same_forward'] = max(_ulp_apart(out['streaming']['wgrad'], out['mixed_a']['wgrad']), _ulp_apart(out['tiled']['wgrad'], out['mixed_b']['wgrad']))
    t_loss, t_l1, t_ssim, _ = ref['truth']
    o_loss, o_l1, o_ssim, _ = ref['oracle']
    for name in ('streaming', 'tiled'):
        k = out[name]
        figures = [('loss', k['loss'], t_loss, o_loss), ('l1', float(k['means'][0]), t_l1, o_l1), ('ssim', float(k['means'][1]), t_ssim, o_ssim)]
        worst[name] = {n: abs(v - t) for n, v, t, _ in figures}
    helpers.log_note('loss_stream_vs_tiled', f'{content}_{shape_id(shape)}', **{k: str(v) for k, v in worst.items()})
    print('streaming against tiled, float32 steps apart and |scalar - truth|:', shape_id(shape), content, worst)
    for key in ('maps', 'wmaps', 'grad', 'grad_mixed', 'wgrad_same_forward'):
        assert worst[key] == 0, (shape, content, key, worst)
    for name in ('streaming', 'tiled'):
        k = out[name]
        for n, v, t, o in [('loss', k['loss'], t_loss, o_loss), ('l1', float(k['means'][0]), t_l1, o_l1), ('ssim', float(k['means'][1]), t_ssim, o_ssim)]:
            assert abs(v - t) <= max(base.LOSS_TOL, helpers.THREE_WAY_FACTOR * abs(o - t)), (shape, content, name, n, worst)
    return worst
