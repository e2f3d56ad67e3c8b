"""Shapes and checks shared by tests/test_k12_folds.py (CPU simulation) and tests/test_gpu_k12_folds.py (MI355X): the smallest scenes at which the helpers
that csrc/preprocess_backward.hip's K12 forms share (wave-block preamble, staged phase A, 16-byte Adam piece and scalar tail of csrc/fgs_adam.h) can go wrong.

N = 64 (one whole wave) and 65 (a ragged wave of ONE Gaussian, which is visible and reached), 64 x 48 pixels, K = 1, 4, 9, 16 bases, i.e. R = 0, 3, 8, 15
coefficients per channel: RT = 15 and the generic instantiation, the R == 0 return, last waves of 9 and of 45 floats (a tail of fewer than four), and
65 * R * 3 no multiple of four for the flat kernel.

Alignment: state at data_ptr() % 16 == 4 is run through the one form that has a scalar path for it, the fused single kernel (vector_ok = 0). The plain
backward reads its inputs element by element and writes gradients that the backend allocates itself (always aligned), so there is nothing to misalign;
the two-kernel fused form, the sharded owner pass and the Adam kernel take 16-byte pieces unconditionally, as they always have: unaligned state is not
an input they accept, so they run aligned only.

Bars: the simulation is deterministic, so forms are compared bit for bit there (the sharded pair, whose fused side sums the views in another order than
gradient tensor + Adam, at the bars of tests/test_sharded.py::test_fused_and_unfused_phase_c_agree). On hardware K11's float atomics make two backward
passes over the same scene differ in the last bits, so two forms are compared at 1e-5 of the tensor's max-abs value (the bar
tests/test_reached_blocks.py uses for the same comparison) and against the reference at the suite's 1e-4."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import helpers
from harness.scenes import View, make_s0
from unreached_cases import LRS, ORDER

SHAPES = [(n, k) for n in (64, 65) for k in (1, 4, 9, 16)]
TOL, FORM_TOL = 1e-4, 1e-5


@functools.lru_cache(maxsize=None)
def scene(n: int, K: int, owners: int = 1):
    """owners > 1: owners * n Gaussians, so that each strided shard (harness.sharded.shard_of) has n and ends with one of the last Gaussians."""
    p, v = make_s0(seed=17, n=n * owners, sh_bases=K)
    p['means'][:6 * owners, 2] = -10.0                         # behind the camera: invisible rows
    for i in range(owners):                                    # the last Gaussian (of every shard): small, in front of everything, mid-image
        p['means'][n * owners - 1 - i] = torch.tensor([0.02 + 0.1 * i, -0.03, -3.0])
    p['scales'][n * owners - owners:] = float(np.log(0.03))
    p['opacities'][n * owners - owners:] = 0.0
    view = View(v.w2c, v.position, 64, 48, 64.0, 64.0, 32.0, 24.0, 0.2, 1e4, torch.zeros(3))
    gi = torch.randn(3, 48, 64, generator=torch.Generator().manual_seed(3))
    return {k: t.contiguous() for k, t in p.items()}, view, gi


def close(a: torch.Tensor, b: torch.Tensor, exact: bool, what) -> None:
    if exact:
        assert torch.equal(a, b), what
    else:
        assert helpers.rel_inf(a.cpu().numpy(), b.cpu().numpy()) < FORM_TOL, what


def backward(be, device: str, n: int, K: int):
    params, view, gi = scene(n, K)
    _, RS = helpers.settings_pair(view, K, device=device)
    dp = {k: t.to(device) for k, t in params.items()}
    res = be.forward(*[dp[k] for k in helpers.NAMES], RS)
    grads = be.backward(None, gi.to(device), res.image, dp['means'], dp['scales'], dp['rotations'], dp['opacities'], dp['sh_coefficients_rest'],
                        res.buffers, RS, res.state)
    return dict(zip(helpers.GRAD_KEYS, grads))


def check_single_kernel_against_two_kernels_and_reference(be, oracle, device: str, n: int, K: int):
    """(a) backward_gradients_kernel == the dev build's two-kernel form (option 3 = 0); (d) both within 1e-4 of the reference; the ragged wave's
    only Gaussian has a gradient."""
    params, view, gi = scene(n, K)
    S, _ = helpers.settings_pair(view, K)
    f = oracle.forward(*helpers.np_params(params), S, bucket_size=64)
    g = oracle.backward(f, S, gi.numpy(), np.zeros((2, n), np.float32))
    one = backward(be, device, n, K)
    assert be.lib.fgs_debug_set_option(3, 0) == 0
    try:
        two = backward(be, device, n, K)
    finally:
        assert be.lib.fgs_debug_set_option(3, 1) == 0
    for k in helpers.GRAD_KEYS:
        if one[k].numel() == 0:
            continue
        close(one[k], two[k], device == 'cpu', (n, K, k))
        assert helpers.rel_inf(one[k].cpu().numpy().reshape(g[k].shape), g[k]) < TOL, (n, K, k)
        assert np.abs(g[k][n - 1]).max() > 0 and float(one[k].reshape(n, -1)[n - 1].abs().max()) > 0, (k, 'the last Gaussian was not reached')


def check_fused_equals_backward_then_adam(be, device: str, n: int, K: int, unaligned: bool, single_kernel: bool = True):
    """(b) the fused form == backward, then the Adam kernel (tests/helpers.py's comparison: two steps, parameters, both moments, the
    densification statistics). single_kernel False: the dev build's two-kernel form (option 3 = 0), whose flat SH-rest kernel ends in a tail."""
    params, view, _ = scene(n, K)
    same = torch.equal if device == 'cpu' else lambda a, b: helpers.rel_inf(a.cpu().numpy(), b.cpu().numpy()) < FORM_TOL
    if not single_kernel:
        assert be.lib.fgs_debug_set_option(3, 0) == 0
    try:
        helpers.fused_equals_backward_then_adam(be, params, view, K, False, unaligned, device, same, helpers.seeded_moments)
    finally:
        if not single_kernel:
            assert be.lib.fgs_debug_set_option(3, 1) == 0


def check_sharded_fused_equals_unfused(be, device: str, n: int, K: int):
    """(c) the sharded owner pass, two owners of n Gaussians x two views, two steps: K12 + Adam fused (sh_rest_adam_views_kernel) == gradient tensor
    (sh_rest_gradient_kernel<.., true>), then the Adam kernel; tests/test_sharded.py::test_fused_and_unfused_phase_c_agree at this module's shapes,
    from seeded moments (helpers.seeded_moments says why)."""
    from harness.distributed import SEGMENTS
    from harness.sharded import LocalShardGroup
    params, view, _ = scene(n, K, 2)
    w2c = view.w2c.clone()
    w2c[0, 3] = 0.3
    views = [view, dataclasses.replace(view, w2c=w2c, position=view.position - torch.tensor([0.3, 0.0, 0.0]))]
    RS = [helpers.settings_pair(v, K, device=device)[1] for v in views]
    targets = [torch.full((3, view.height, view.width), 0.3 + 0.2 * i, device=device) for i in range(2)]
    groups = [LocalShardGroup(be, {k: t.to(device) for k, t in params.items()}, dict(zip(ORDER, LRS)), 2, fused=f) for f in (True, False)]
    for grp in groups:
        for s, t in enumerate(grp.ranks):
            assert t.n == n
            for i, k in enumerate(SEGMENTS):
                o, cnt, shape = t.layout[k]
                m0, v0 = helpers.seeded_moments(params[k].shape, 11 + i)
                t.exp_avg[o:o + cnt].view(shape).copy_(m0[s::2])
                t.exp_avg_sq[o:o + cnt].view(shape).copy_(v0[s::2])
        for _ in range(2):
            grp.step(RS, targets)
    for a, b in zip(groups[0].ranks, groups[1].ranks):
        if device == 'cpu':
            assert torch.allclose(a.param_arena, b.param_arena, rtol=0, atol=1e-6)
            assert torch.allclose(a.exp_avg, b.exp_avg, rtol=1e-5, atol=1e-9) and torch.allclose(a.exp_avg_sq, b.exp_avg_sq, rtol=1e-5, atol=1e-12)
            assert torch.equal(a.densification_info, b.densification_info)
        else:
            for k in SEGMENTS:
                o, cnt, shape = a.layout[k]
                start = params[k][a.rank::2].reshape(-1).to(device)
                for x, y, what in ((a.param_arena[o:o + cnt] - start, b.param_arena[o:o + cnt] - start, 'step taken'),
                                   (a.exp_avg[o:o + cnt], b.exp_avg[o:o + cnt], 'exp_avg'), (a.exp_avg_sq[o:o + cnt], b.exp_avg_sq[o:o + cnt], 'exp_avg_sq')):
                    assert helpers.rel_inf(x.cpu().numpy(), y.cpu().numpy()) < FORM_TOL, (k, a.rank, what)
            assert helpers.rel_inf(a.densification_info.cpu().numpy(), b.densification_info.cpu().numpy()) < FORM_TOL
        lo, cnt, _ = a.layout['sh_coefficients_rest']
        last = a.param_arena[lo:lo + cnt].view(n, -1)[n - 1].cpu() - params['sh_coefficients_rest'][2 * n - 2 + a.rank].reshape(-1)
        assert K == 1 or float(last.abs().max()) > 0, 'the last Gaussian of the shard was not reached'
