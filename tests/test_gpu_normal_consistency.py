"""The normal-consistency regulariser on the MI355X: the comparisons of tests/test_normal_consistency.py against the same fp64 reference
(tests/normal_cases.py: definitions, cases, bars), autograd through the public operators, and the harness."""
import pytest

import normal_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name', list(cases.IMAGE_CASES))
def test_image_space_matches_the_fp64_reference_on_device(hip_backend, name):
    """1. E, gN_r, gD, gA at rel_inf < 1e-4; identical valid masks; exact zeros where invalid."""
    cases.check_image_parity(hip_backend, name, device=DEV)


def test_degenerate_shapes_on_device(hip_backend):
    cases.check_degenerate_shapes(hip_backend, device=DEV)


@pytest.mark.parametrize('n', cases.GAUSSIAN_COUNTS)
def test_surface_features_match_the_fp64_reference_on_device(hip_backend, n):
    cases.check_gaussian_parity(hip_backend, n, device=DEV)


def test_no_gaussians_on_device(hip_backend):
    cases.check_no_gaussians(hip_backend, device=DEV)


def test_surface_feature_edges_on_device(hip_backend):
    cases.check_gaussian_edges(hip_backend, device=DEV)


def test_reproducible_and_complete_on_device(hip_backend):
    """4. No float atomics in either backward pass: two runs are bit-identical on the device as well."""
    cases.check_reproducible_and_complete(hip_backend, device=DEV)


def test_refusals_on_device(hip_backend):
    cases.check_refusals(hip_backend, device=DEV)


def test_public_operators_on_device(hip_backend):
    """6. At the bar the bilagrid operator test uses on the device (1e-5)."""
    import FasterGSCudaBackend as B
    cases.check_operators(B, hip_backend, device=DEV, tol=1e-5)


def test_training_iteration_equals_the_step_composed_by_hand_on_device(hip_backend):
    cases.check_training_iteration(hip_backend, device=DEV, exact=False)


def test_it_regularises_on_device(hip_backend):
    """8. The same scene, steps and learning rate as on the simulation, the same one-half bar."""
    cases.check_regularises(device=DEV)
