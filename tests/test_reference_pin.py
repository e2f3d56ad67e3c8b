"""CPU, live pin: the oracle (oracle/fgs_oracle.c, a restatement) against the reference's own kernels and host code, compiled for the CPU by
oracle/build_ref.py on the stand-in CUDA headers of oracle/cuda_on_cpu and run through oracle/reference.py. Needs the reference tree (or a library
built from it earlier); skipped only when there is neither. With a tree present a library that cannot be built is a failure.

Both sides are fp32 with -ffp-contract=off on one libm, and the stand-in scheduler runs work-items in rank order, so the reference's atomics arrive in
the order the oracle's loops add: measured, every field of every scene below is bit-equal, the atomic sums included (rel_inf 0.0; the bar for them
stays the project's 1e-5). What this does NOT pin: nvcc's FMA contraction and NVIDIA's __expf (the arithmetic here is the reference's "as written"),
and the 32-bit-key path above 65 536 tiles (too slow on the emulator).
"""
import numpy as np
import pytest

import helpers
import ref_pin_cases as cases
from oracle import reference as R

pytestmark = pytest.mark.skipif(not R.available(), reason='neither oracle/_ref/libfgs_ref_cpu.so nor a reference tree')

SCENES = ['s0', 'tiny_aa'] + [f'partial_{w}x{h}' for w, h, _, _ in cases.PARTIAL] + ['tied_depth', 'large_footprints', 'on_the_cut'] + [f'fuzz_{s}' for s in range(8)]


def _settings(name):
    params, view, K, aa = cases.scene(name)
    S, _ = helpers.settings_pair(view, K, aa)
    return helpers.np_params(params), S


@pytest.mark.parametrize('name', SCENES)
def test_forward_and_backward_field_by_field(oracle, name):
    a, S = _settings(name)
    n = a[0].shape[0]
    r = R.forward(*a, S)
    f = oracle.forward(*a, S, bucket_size=32)
    assert r['end_bit'] == f['end_bit'] and r['T'] == f['T']
    cases.compare_structure(f, r, name)
    cases.compare_floats_bitwise(f, r, name)
    # The oracle has no selector. What is checked of it is that decoding the instance double buffer through the selector the reference RETURNED gave
    # the tile-sorted lists that matched above; which half that is follows from the pass count of the stand-in sort, not from CUB, and is not compared.
    assert r['_state'][:2] == (f['I'], f['B']) and r['_state'][2] in (0, 1)
    gi = cases.grad_image_of(f['image'].shape)
    dens_r, dens_o = np.zeros((2, n), np.float32), np.zeros((2, n), np.float32)
    gr = R.backward(r, S, gi, dens_r)
    go = oracle.backward(f, S, gi, dens_o)
    worst = cases.compare_atomic_sums(go, gr, name)
    worst.update(cases.compare_atomic_sums({'densification_info': dens_o}, {'densification_info': dens_r}, name, keys=('densification_info',)))
    for k in ('_grad_mean2d', '_grad_conic'):          # the blend backward's own atomic sums, before the preprocess backward consumes them
        assert helpers.rel_inf(go[k], gr[k]) < cases.ATOMIC_BAR, (name, k)


def test_the_scenes_reach_the_edges_they_are_here_for(oracle):
    """Culls at both planes, degenerate quaternions, lists longer than one 192-entry batch, early termination, the cooperative instance path, ties."""
    a, S = _settings('large_footprints')
    f = oracle.forward(*a, S)
    assert int((f['ranges'][:, 1] - f['ranges'][:, 0]).max()) > 192 and float(f['final_T'].min()) < 1e-4 and int((f['n_touched'] > 4).sum()) > 50
    a, S = _settings('tied_depth')
    f = oracle.forward(*a, S)
    assert len(np.unique(f['depth_keys'])) <= 3 < f['V']
    a, S = _settings('on_the_cut')
    f = oracle.forward(*a, S)
    k = len(cases.ON_THE_CUT)
    cut = np.float32(1.0) / np.float32(255.0)
    assert np.all(f['n_touched'][:k] > 0) and np.all(f['conic_opacity'][:k, 3] == cut) and np.all(f['mean2d'][:k] == 64.5)
    assert f['n_processed'][64 * 128 + 64] >= int(np.flatnonzero(np.isin(f['inst_prims'], np.arange(k))).max()) + 1 - int(f['ranges'][5 * 8 + 4, 0])
    culled = 0
    for s in range(8):
        a, S = _settings(f'fuzz_{s}')
        f = oracle.forward(*a, S)
        culled += a[0].shape[0] - f['V']
    assert culled > 100


@pytest.mark.parametrize('name', ['s0', 'tiny_aa', 'partial_130x25', 'fuzz_3'])
@pytest.mark.parametrize('to_chw,clamp', [(True, True), (True, False), (False, True), (False, False)])
def test_inference_every_layout_and_clamp(oracle, name, to_chw, clamp):
    a, S = _settings(name)
    r = R.inference(*a, S, to_chw=to_chw, clamp_output=clamp)
    f = oracle.forward(*a, S, inference=True, to_chw=to_chw, clamp_output=clamp)
    cases.compare_structure(f, r, name, blend=False)
    cases.compare_floats_bitwise(f, r, name, blend=False)


@pytest.mark.parametrize('name', ['s0', 'tiny_aa', 'partial_333x211', 'large_footprints', 'fuzz_5'])
def test_pruning_scores_accumulate_on_a_nonzero_vector(oracle, name):
    a, S = _settings(name)
    n = a[0].shape[0]
    base = cases.score_base_of(n)
    sr, so = base.copy(), base.copy()
    r = R.pruning_scores(sr, *a, S)
    f = oracle.pruning_scores(so, *a, S)
    cases.compare_structure(f, r, name, blend=False)
    assert np.abs(sr - base).max() > 0 and np.array_equal(sr[f['n_touched'] == 0], base[f['n_touched'] == 0])
    cases.compare_atomic_sums({'pruning_scores': so}, {'pruning_scores': sr}, name, keys=('pruning_scores',))
    cases.compare_atomic_sums({'pruning_scores_added': so - base}, {'pruning_scores_added': sr - base}, name, keys=('pruning_scores_added',), support=False)


def test_mcmc_relocation_and_noise(oracle):
    c = cases.mcmc_case()
    ro, rs = R.relocation_adjustment(c['old_opacities'], c['old_scales'], c['n_samples'])
    oo, os_ = oracle.relocation_adjustment(c['old_opacities'], c['old_scales'], c['n_samples'])
    assert cases.same_bits(oo, ro), helpers.rel_inf(oo, ro)
    fin = np.isfinite(rs).all(axis=1)
    assert np.array_equal(fin, np.isfinite(os_).all(axis=1)) and cases.same_bits(os_[fin], rs[fin]), helpers.rel_inf(os_[fin], rs[fin])
    m0 = c['means']
    mr, mo = m0.copy(), m0.copy()
    R.add_noise(c['raw_scales'], c['raw_rotations'], c['raw_opacities'], c['noise'], mr, float(c['current_lr']))
    oracle.add_noise(c['raw_scales'], c['raw_rotations'], c['raw_opacities'], c['noise'], mo, float(c['current_lr']))
    assert np.array_equal(mr[:4], m0[:4]) and np.abs(mr - m0).max() > 0
    assert cases.same_bits(mo, mr), helpers.rel_inf(mo - m0, mr - m0)
