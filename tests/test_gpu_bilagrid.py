"""Bilateral-grid colour correction on the MI355X: the comparisons of tests/test_bilagrid.py against the same fp64 reference (tests/bilagrid_cases.py:
definitions, cases, bars), plus `wide` and `crowd`, where many workgroups flush into the same cells (`crowd`: 324 into one), autograd through the public
operators, and the harness."""
import pytest

import bilagrid_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name', cases.GPU_CASES)
def test_slice_and_gradients_match_the_fp64_reference_on_device(hip_backend, name):
    """1. out, grad_image, grad_grid at rel_inf < 1e-4; `fine` runs the global-memory path, the others the LDS-staged one."""
    cases.check_parity(hip_backend, name, device=DEV)


@pytest.mark.parametrize('name', ['fine', 'coarse'])
def test_identity_grid_is_the_identity_on_device(hip_backend, name):
    cases.check_identity(hip_backend, name, device=DEV)


@pytest.mark.parametrize('name', cases.GPU_CASES)
def test_a_gradient_that_is_not_asked_for_changes_nothing_on_device(hip_backend, name):
    """3. grad_image bit-identical; grad_grid within 1e-5 between two runs (atomic order)."""
    cases.check_null_gradients(hip_backend, name, device=DEV, exact_grid=False)


@pytest.mark.parametrize('name', ['fine', 'wide'])
def test_stale_scratch_is_harmless_on_device(hip_backend, name):
    cases.check_stale_scratch(hip_backend, name, device=DEV, exact=False)


def test_total_variation_on_device(hip_backend):
    cases.check_tv(hip_backend, device=DEV)


def test_refusals_on_device(hip_backend):
    cases.check_refusals(hip_backend, device=DEV)


def test_public_operators_on_device(hip_backend):
    import FasterGSCudaBackend as B
    cases.check_operators(B, hip_backend, device=DEV, tol=1e-5)


def test_training_iteration_equals_the_step_composed_by_hand_on_device(hip_backend):
    cases.check_training_iteration(hip_backend, device=DEV, exact=False)


def test_grids_learn_a_fixed_colour_transform_on_device(hip_backend):
    """8b: 30 steps on make_s0(n=1000), the Gaussians frozen at the truth."""
    cases.check_training_run(device=DEV, steps=30, n=1000)


def test_checkpoint_round_trip_with_grids_on_device(hip_backend, tmp_path):
    cases.check_checkpoint_round_trip(tmp_path, device=DEV, exact=False)
