"""fgs_blend_geometry / fgs_backward_geometry, the public diff_rasterize_geometry and the harness on the MI355X: the comparisons of
tests/test_geometry.py against the same fp64 reference (tests/geometry_cases.py: definitions, upstream gradients, bars)."""
import pytest

import geometry_cases as cases
import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_one_case_walks_more_than_one_batch_on_device(hip_backend):
    cases.check_long_lists(hip_backend, DEV)


@pytest.mark.parametrize('name,mode', cases.PARITY)
def test_maps_image_and_gradients_match_the_fp64_reference_on_device(hip_backend, name, mode):
    """1. As on the simulation; the image is held at MAP_TOL against plain `forward` (equal-depth compaction order is the only licence)."""
    cases.check_against_reference(hip_backend, name, mode, device=DEV, exact_image=False)


@pytest.mark.parametrize('name,mode', cases.PARITY)
def test_the_one_walk_equals_the_two_it_replaces_on_device(hip_backend, name, mode):
    """2. The maps within MAP_TOL (the units are compiled apart: contraction may differ), the gradients within GRAD_TOL."""
    cases.check_replaced_operators(hip_backend, name, mode, device=DEV, exact=False)


@pytest.mark.parametrize('name,mode', cases.ALONE)
def test_terms_alone_on_device(hip_backend, name, mode):
    cases.check_terms_alone(hip_backend, name, mode, DEV)


def test_boundary_cases_on_device(hip_backend):
    cases.check_boundaries(hip_backend, DEV)


def test_refusals_on_device(hip_backend):
    cases.check_refusals(hip_backend, DEV)


def test_abi_refusals_on_device(hip_backend):
    _lib, _ = helpers.backend_modules()
    cases.check_abi_refusals(hip_backend.lib, _lib)


def test_autograd_through_diff_rasterize_geometry(hip_backend):
    """6. The public operator on the case with hot Gaussians."""
    import FasterGSCudaBackend as B
    cases.check_operator(B, hip_backend, 'hot', DEV)


def test_composed_graph_equals_the_two_renders_on_device(hip_backend):
    """7. At the bar tests/test_gpu_normal_consistency.py passes to check_operators on the device (1e-5)."""
    import FasterGSCudaBackend as B
    cases.check_composed(B, device=DEV, tol=1e-5)


def test_training_iteration_with_the_geometry_render_on_device(hip_backend):
    cases.check_training_iteration(device=DEV)


def test_it_regularises_on_device(hip_backend):
    cases.check_regularises(device=DEV)
