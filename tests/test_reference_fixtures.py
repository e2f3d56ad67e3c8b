"""CPU, no reference tree needed: the committed fixtures tests/golden/ref_kernels_*.npz hold what the reference's own kernels computed (run on the CPU
by oracle/build_ref.py, written by tests/golden/make_ref_kernel_golden.py). The oracle must reproduce them at the bars of the live pin
(tests/test_reference_pin.py) -- this is what guards oracle/fgs_oracle.c wherever the suite runs -- and the CPU simulation of the HIP sources must
meet them at the bar it is held to against the oracle (integers exact, floats 1e-5).

Checked by hand on a scratch copy of oracle/fgs_oracle.c, not committed -- one comparison flipped at a time, then
test_oracle_reproduces_the_reference_kernels:
  forward blend  `alpha < 1/255 -> skip` to `<=`        fails on on_the_cut (image, 3.2e-3); the other four fixtures hold no pair ON the cut and pass
  forward blend  cut moved to 1.0001 / 255              fails on s0 and partial_333x211 (n_processed, one pixel each)
  preprocess     `opacity < 1/255` (antialiased) to `<=`  fails on on_the_cut (V 116 against 120)
  blend backward `alpha < 1/255 -> skip` to `<=`        fails on on_the_cut (the support of the gradients: four Gaussians lose their only pair)
  pruning scores `alpha < 1/255 -> skip` to `<=`        fails on on_the_cut (scores)
  sub-tile overlap test `<` to `<=`                     passes: the test is a conservative cull, a Gaussian it lets through fails the alpha cut
"""
import numpy as np
import pytest

import helpers
import ref_pin_cases as cases


@pytest.mark.parametrize('name', cases.CPU_FIXTURES)
def test_oracle_reproduces_the_reference_kernels(oracle, name):
    g, params, view, K, aa = cases.load_fixture(name)
    S, _ = helpers.settings_pair(view, K, aa)
    a = helpers.np_params(params)
    n = a[0].shape[0]
    f = oracle.forward(*a, S, bucket_size=32)
    assert f['end_bit'] == int(g['end_bit'])
    cases.compare_structure(f, g, name)
    cases.compare_floats_bitwise(f, g, name)
    dens = np.zeros((2, n), np.float32)
    go = oracle.backward(f, S, g['grad_image'], dens)
    go['densification_info'] = dens
    scores = cases.score_base_of(n)
    oracle.pruning_scores(scores, *a, S)
    go['pruning_scores'] = scores
    ref = {k: g[f'grad_{k}'] for k in helpers.GRAD_KEYS}
    ref.update(densification_info=g['densification_info'], pruning_scores=g['pruning_scores'])
    cases.compare_atomic_sums(go, ref, name, keys=tuple(ref))


@pytest.mark.parametrize('name', cases.CPU_FIXTURES)
def test_simulated_kernels_meet_the_reference_kernels(sim_backend, oracle, name):
    cases.check_backend_against_fixture(sim_backend, oracle, name, 'cpu', on_hardware=False)


@pytest.mark.parametrize('name', cases.CPU_FIXTURES)
def test_simulated_product_flavour_meets_the_reference_kernels(sim_product_backend, oracle, name):
    cases.check_backend_against_fixture(sim_product_backend, oracle, name, 'cpu', on_hardware=False)


def test_oracle_reproduces_the_reference_mcmc_kernels(oracle):
    """relocation_adjustment and add_noise as the reference's kernels computed them (tests/golden/ref_kernels_mcmc.npz), bit for bit: the tree-free guard
    of orc_relocation_adjustment / orc_add_noise. The numpy restatements they replaced missed this by one ulp in the new opacities (4.3e-5 of the new
    scales) and by 1.5e-6 of the noise displacement."""
    g = np.load(cases.fixture_path('mcmc'))
    new_op, new_sc = oracle.relocation_adjustment(g['old_opacities'], g['old_scales'], g['n_samples'])
    assert cases.same_bits(new_op, g['new_opacities']), helpers.rel_inf(new_op, g['new_opacities'])
    fin = np.isfinite(g['new_scales']).all(axis=1)
    assert 0 < int((~fin).sum()) < 8 and np.array_equal(fin, np.isfinite(new_sc).all(axis=1))          # opacity 0 and 1: 0 / 0 and x / 0, on both sides
    assert cases.same_bits(new_sc[fin], g['new_scales'][fin]), helpers.rel_inf(new_sc[fin], g['new_scales'][fin])
    means = g['means'].copy()
    oracle.add_noise(g['raw_scales'], g['raw_rotations'], g['raw_opacities'], g['noise'], means, float(g['current_lr']))
    assert np.array_equal(means[:4], g['means'][:4]) and cases.same_bits(means, g['moved_means'])          # the first four quaternions are degenerate
