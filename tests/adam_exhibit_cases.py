"""Cases shared by tests/test_k1_schemes.py (CPU simulation) and tests/test_gpu_k1_schemes.py (MI355X): K13's A/B exhibits of the dev library
(csrc/adam.hip: launch_adam_exhibit) -- option 2 = 0 with option 1 in {1, 2, 4} (plain loads and stores, 1 / 2 / 4 16-byte pieces per thread; unroll
applies to the plain-load kernels only) and option 8 in {0, 1} (workgroup order) -- against the form every library runs (option 2 = 1, 8 = 1).

adam_update of an element depends on that element alone, so one multi-group step leaves the same bits in the parameters and in both moments whatever
the switches say. No tolerance.

Groups of 1, 1027 and 4100 floats: every group gets a workgroup to itself; two tensor tails of 4 k + 3 floats and one of a single float; at 4 pieces
per thread the last group is one workgroup larger than a workgroup's 4096 floats."""
from __future__ import annotations

import numpy as np
import torch

SIZES = (1, 1027, 4100)
DEFAULTS = {1: 1, 2: 1, 8: 1}                                  # option -> the value the product's form corresponds to
EXHIBITS = ({2: 0, 1: 1}, {2: 0, 1: 2}, {2: 0, 1: 4}, {8: 0}, {8: 1})
IDS = ('plain-1', 'plain-2', 'plain-4', 'forward-order', 'reverse-order')


def step(be, device: str = 'cpu') -> list:
    """One adam_step_multi over fresh copies of the same three groups (non-zero moments, step 3): [params, exp_avgs, exp_avg_sqs] as numpy arrays."""
    gen = torch.Generator().manual_seed(41)
    grads, params, m, v = ([torch.randn(s, generator=gen).to(device) for s in SIZES] for _ in range(4))
    v = [x.abs() * 1e-3 for x in v]
    before = [p.clone() for p in params]
    be.adam_step_multi(grads, params, m, v, [3] * len(SIZES), [1e-2, 3e-3, 1e-4], 0.9, 0.999, 1e-15)
    assert all(not torch.equal(a, b) for a, b in zip(before, params))      # the step does move every group
    return [np.concatenate([t.cpu().numpy() for t in group]) for group in (params, m, v)]


def step_with(be, options: dict, device: str = 'cpu') -> list:
    """step under the given options (dev library), the defaults restored whatever happens."""
    try:
        for key, value in options.items():
            assert be.lib.fgs_debug_set_option(key, value) == 0
        return step(be, device)
    finally:
        for key, value in DEFAULTS.items():
            be.lib.fgs_debug_set_option(key, value)


def check_same(got: list, ref: list, label) -> None:
    for name, a, b in zip(('param', 'exp_avg', 'exp_avg_sq'), got, ref):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (label, name)

