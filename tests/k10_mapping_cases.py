"""Cases shared by tests/test_k10_mappings.py (CPU simulation) and tests/test_gpu_k10_mappings.py (MI355X): K10's tile -> workgroup mappings
(csrc/fgs_k10_mappings.h, fgs_debug_set_option(10, ..) of the dev library) and the one mapping the product library runs (csrc/api.hip: columns top-down).

A pixel's blend does not depend on which workgroup runs its tile, so whatever the mapping, every entry point of the unit returns the bits it returns
under the default mapping: the training forward (image, final_T, n_processed, bucket_offsets), the inference image, the maps of the inference blend
with auxiliary outputs and of the training blend with auxiliary outputs. No tolerance. The pruning-score kernel adds with float atomics, whose order
the mapping does change: it is held, per mapping, to the bar of tests/test_pruning_scores.py against the oracle (SCORE_BAR).

Sizes: the smallest at which a mapping can go wrong (16 x 12 tiles, 8 XCDs, a plan of 8 x 10 blocks).
  333 x 211  21 x 18 tiles  grid width no multiple of 8: the last strip of columns is narrower and padding workgroups exist
   16 x 12    1 x 1         one tile: seven empty strips, a plan of 79 empty blocks
  130 x 25    9 x 3         fewer tile rows than XCDs for the row-group mappings"""
from __future__ import annotations

import functools
import types

import numpy as np
import torch

import helpers
from harness.scenes import View, make_s0

DEFAULT = 252                                                  # columns top-down
MAPPINGS = (252, 251, 254, 253, 0, 255, 1, 2, 64)               # columns top-down / bottom-up, block plan, bands through the plan, bands, bands bottom first, row groups
SIZES = ((333, 211), (16, 12), (130, 25))
N = 300
SCORE_BASE = 0.5                                               # the scores accumulate on top of existing values
SCORE_BAR = {'cpu': 1e-5, 'cuda': 1e-4}                        # tests/test_pruning_scores.py: simulation, device


@functools.lru_cache(maxsize=None)
def scene(w: int, h: int):
    """make_s0(seed=5, n=300) in the lower half of a w x h image (a strong vertical work gradient), as in
    test_sim_parity.py::test_tile_plan_covers_every_tile_and_balances_the_xcds. Shared: treat as read-only."""
    p, v = make_s0(seed=5, n=N)
    p['means'][:, 1] = p['means'][:, 1].abs()
    return p, View(v.w2c, v.position, w, h, 0.8 * w, 0.8 * w, w / 2.0, h / 2.0, 0.2, 1e4, torch.tensor([0.2, 0.5, 0.7]))


@functools.lru_cache(maxsize=None)
def oracle_scores(w: int, h: int) -> np.ndarray:
    from oracle import oracle as O
    O.build()
    p, v = scene(w, h)
    S, _ = helpers.settings_pair(v)
    ref = np.full(N, SCORE_BASE, np.float32)
    O.pruning_scores(ref, *helpers.np_params(p), S)
    return ref


def run_all(be, w: int, h: int, device: str = 'cpu') -> dict:
    """Every launcher of blend_forward.hip once, under whatever mapping is set: name -> numpy array."""
    p, v = scene(w, h)
    _, RS = helpers.settings_pair(v, device=device)
    args = [p[k].to(device) for k in helpers.NAMES]
    out = {}
    res = be.forward(*args, RS)
    dec = helpers.decode_forward(be, res, N, w, h)
    out['image'], out['state'] = res.image.cpu().numpy(), np.asarray(res.state)
    for k in ('final_T_tiles', 'n_processed_tiles', 'bucket_offsets', 'max_n_processed'):
        out[k] = dec[k].copy()
    out['inference'] = be.inference(*args, RS, True, True).cpu().numpy()
    for k, t in be.inference_aux(*args, RS, False, False).items():
        out['inference_aux.' + k] = t.cpu().numpy()
    aux = be.forward_aux(*args, RS)
    plain = types.SimpleNamespace(buffers=aux.buffers, state=aux.state[:3] + (aux.state[3] & 1,))      # the selector without its depth-checkpoint flag
    dec = helpers.decode_forward(be, plain, N, w, h)
    out['forward_aux.image'], out['forward_aux.alpha'], out['forward_aux.depth'] = (t.cpu().numpy() for t in (aux.image, aux.alpha, aux.depth))
    out['forward_aux.final_T_tiles'], out['forward_aux.n_processed_tiles'] = dec['final_T_tiles'].copy(), dec['n_processed_tiles'].copy()
    scores = torch.full((N,), SCORE_BASE, device=device)
    be.pruning_scores(scores, *args, RS)
    out['scores'] = scores.cpu().numpy()
    return out


def run_all_mapped(be, mapping: int, w: int, h: int, device: str = 'cpu') -> dict:
    """run_all under option 10 = mapping (dev library), the default restored whatever happens."""
    assert be.lib.fgs_debug_set_option(10, mapping) == 0
    try:
        return run_all(be, w, h, device)
    finally:
        be.lib.fgs_debug_set_option(10, DEFAULT)


def check_same(got: dict, ref: dict, device: str, label) -> None:
    """Bit-identical to `ref` (the default mapping) in everything but the scores; the scores of BOTH within the bar of the oracle's."""
    assert set(got) == set(ref)
    for k in ref:
        if k != 'scores':
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (label, k)
    w, h = ref['image'].shape[2], ref['image'].shape[1]
    want = oracle_scores(w, h)
    assert (want > SCORE_BASE).any(), label                     # the case does score something
    for name, s in (('default', ref['scores']), ('mapped', got['scores'])):
        err = helpers.rel_inf(s - SCORE_BASE, want - SCORE_BASE)
        print(label, name, 'pruning scores against the oracle:', err)
        assert err < SCORE_BAR[device], (label, name, err)
