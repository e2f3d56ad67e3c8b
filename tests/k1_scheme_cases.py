"""Cases shared by tests/test_k1_schemes.py (CPU simulation) and tests/test_gpu_k1_schemes.py (MI355X): K1's two tile-counting schemes -- the flattened
count every library runs (csrc/preprocess.hip) and the reference's "n sequential candidates per lane" exhibit of the dev library
(csrc/fgs_k1_exhibits.h, fgs_debug_set_option(5, n)).

Both schemes count the same candidates with the same test, so whatever option 5 is set to (SCHEMES against DEFAULT), one training forward and one
inference forward return the same bits. Compared exactly: V, I, n_touched, the records of the visible Gaussians (screen_bounds, mean2d, conic_opacity,
color; rows of Gaussians K1 found invisible are never written), the depth-sorted keys and primitives, offsets, inst_keys, inst_prims, ranges,
bucket_offsets, n_processed_tiles, final_T_tiles, max_n_processed, the image and the inference image. No tolerance.
Not compared as bits:
  tile_plan      scratch that nothing writes under the default mapping.
  rec_hit_mask   for Gaussians whose box exceeds kHotFootprint (256) candidates it holds a hot-slot number, handed out in atomic order: for those rows
                 the slot words of the two runs are the same multiset; every other visible row is compared exactly.
  the pre-sort compaction buffers (depth_keys0 / prim_idx0)   on the device their order is that of K1's atomics: multisets there, exact on the simulation.
The scenes leave no two visible Gaussians with equal depth keys (sorted_lists asserts it), so the sorted lists are unique.

Scenes: the smallest that reach every path of the count.
  s0      make_s0(seed=3, n=300), 333 x 211 (21 x 18 tiles, partial tiles): V 300, I 2251, footprints <= 19 tiles -- sequential-only for n >= 16, mixed below
  big     helpers.many_big_footprints_scene(), 480 x 270: V 700, I 196 004, footprints up to 690 tiles -- the wave-cooperative loop starting at `first`,
          hot slots (169 of the 700 records)
  huge    make_s0(seed=7, n=200) with scales[:3] += 4, 640 x 480, focal 500: V 200, I 8215, three footprints of 1600 candidates > kHugeFootprint --
          preprocess_huge_kernel behind each scheme
  one     make_s0(seed=9, n=1), 16 x 12: one Gaussian, one tile"""
from __future__ import annotations

import functools

import numpy as np
import torch

import helpers
from harness.scenes import View, make_s0

DEFAULT = 0                                                    # the flattened count
SCHEMES = (1, 4, 16, 32)                                       # candidates each lane tests itself
SCENES = ('s0', 'big', 'huge', 'one')
PRODUCT_SCENES = ('s0', 'big', 'huge')
EXPECT = {'s0': (300, 2251), 'big': (700, 196004), 'huge': (200, 8215), 'one': (1, 1)}      # V, I
K_HOT_FOOTPRINT = 256                                          # csrc/fgs_config.h: kHotFootprint

EXACT = ('n_touched', 'offsets', 'depth_keys1', 'prim_idx1', 'inst_keys', 'inst_prims', 'ranges', 'bucket_offsets', 'n_processed_tiles',
         'final_T_tiles', 'max_n_processed', 'image', 'inference')
VISIBLE_ROWS = ('screen_bounds', 'mean2d', 'conic_opacity', 'color')
COMPACTION = ('depth_keys0', 'prim_idx0')


@functools.lru_cache(maxsize=None)
def scene(name: str):
    """Shared: treat as read-only."""
    if name == 's0':
        p, v = make_s0(seed=3, n=300)
        return p, View(v.w2c, v.position, 333, 211, 0.8 * 333, 0.8 * 333, 333 / 2, 211 / 2, 0.2, 1e4, torch.zeros(3))
    if name == 'big':
        return helpers.many_big_footprints_scene()
    if name == 'huge':
        p, v = make_s0(seed=7, n=200)
        p['scales'][:3] += 4.0
        return p, View(v.w2c, v.position, 640, 480, 500., 500., 320., 240., 0.2, 1e4, torch.zeros(3))
    p, v = make_s0(seed=9, n=1)
    return p, View(v.w2c, v.position, 16, 12, 12.8, 12.8, 8., 6., 0.2, 1e4, torch.zeros(3))


def run(be, name: str, device: str = 'cpu') -> dict:
    """One training forward and one inference forward under whatever scheme is set: name -> numpy array (or int)."""
    p, v = scene(name)
    n = p['means'].shape[0]
    _, RS = helpers.settings_pair(v, device=device)
    args = [p[k].to(device) for k in helpers.NAMES]
    res = be.forward(*args, RS)
    dec = helpers.decode_forward(be, res, n, v.width, v.height)
    out = {k: (np.array(x) if isinstance(x, np.ndarray) else x) for k, x in dec.items()}
    out['image'] = res.image.cpu().numpy()
    out['inference'] = be.inference(*args, RS, True, True).cpu().numpy()
    return out


def run_scheme(be, scheme: int, name: str, device: str = 'cpu') -> dict:
    """run under option 5 = scheme (dev library), the default restored whatever happens."""
    assert be.lib.fgs_debug_set_option(5, scheme) == 0
    try:
        return run(be, name, device)
    finally:
        be.lib.fgs_debug_set_option(5, DEFAULT)


def candidate_tiles(bounds: np.ndarray) -> np.ndarray:
    """Tiles of the box of screen bounds x_min, x_max, y_min, y_max (csrc/fgs_math.h: tile_rect)."""
    b = bounds.astype(np.int64)
    return ((b[:, 1] + 15) // 16 - b[:, 0] // 16) * ((b[:, 3] + 11) // 12 - b[:, 2] // 12)


def sorted_lists(ref: dict, name: str) -> None:
    """The premises of a scene, on the default scheme's output: its size, and depth keys that are strictly increasing -- buffer 1 is the sorted one
    (three 9-bit passes for near 0.2 / far 1e4) and no two visible Gaussians tie, so the sorted primitive list is unique."""
    assert (ref['V'], ref['I']) == EXPECT[name], (name, ref['V'], ref['I'])
    assert np.all(np.diff(ref['depth_keys1'].astype(np.int64)) > 0), name


def check_same(got: dict, ref: dict, device: str, label) -> None:
    assert got['V'] == ref['V'] and got['I'] == ref['I'], label
    for k in EXACT:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (label, k)
    visible = ref['n_touched'] > 0
    for k in VISIBLE_ROWS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k][visible], ref[k][visible]), (label, k)
    for k in COMPACTION:
        if device == 'cpu':
            assert np.array_equal(got[k], ref[k]), (label, k)
        else:
            assert np.array_equal(np.sort(got[k]), np.sort(ref[k])), (label, k)
    hot = visible & (candidate_tiles(ref['screen_bounds']) > K_HOT_FOOTPRINT)
    cold = visible & ~hot
    assert np.array_equal(got['rec_hit_mask'][cold], ref['rec_hit_mask'][cold]), (label, 'rec_hit_mask')
    assert np.array_equal(np.sort(got['rec_hit_mask'][hot]), np.sort(ref['rec_hit_mask'][hot])), (label, 'hot slots')
