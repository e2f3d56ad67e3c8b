"""fgs_blend_geometry / fgs_backward_geometry on the CPU simulation of the product library (the unmodified .hip sources): the one render that carries
the depth-distortion map and the five-channel surface map of the training pass, the public diff_rasterize_geometry and the harness. Definitions,
reference, upstream gradients and bars: tests/geometry_cases.py. The same comparisons run on the MI355X in tests/test_gpu_geometry.py."""
import pytest
import torch

import aux_grad_cases as aux
import geometry_cases as cases
import helpers


@pytest.fixture(scope='module')
def be():
    return helpers.sim_backend(product=True)


@pytest.fixture
def operators_on_sim(be, monkeypatch):
    """The public operators, the optimizer and the harness (all unmodified) running on the simulation backend with CPU tensors."""
    import FasterGSCudaBackend as B
    import FasterGSCudaBackend.adam as A
    import FasterGSCudaBackend.normals as N
    import FasterGSCudaBackend.rasterization as R
    import harness.loss as L
    for module in (R, A, N, L):
        monkeypatch.setattr(module, 'default_backend', lambda: be)
    for module in (R, N):
        monkeypatch.setattr(module, '_require_gpu', lambda t: None)
    return B


@pytest.mark.parametrize('name', list(aux.CASES))
def test_reference_is_pinned(name):
    """First of all, for every case: with gM = 0 the reference is distortion_cases.reference, with gX = 0 it is feature_cases.reference, to 1e-12."""
    cases.check_reference_pins(name)


def test_one_case_walks_more_than_one_batch(be):
    cases.check_long_lists(be)


@pytest.mark.parametrize('name,mode', cases.PARITY)
def test_maps_image_and_gradients_match_the_fp64_reference(be, name, mode):
    """1. X, the five planes of M, the image bit-identical to plain `forward`, the six gradients and grad_surface_features, a rerun; X exactly 0 where
    fewer than two Gaussians were blended and all public planes 0 where none was."""
    cases.check_against_reference(be, name, mode)


@pytest.mark.parametrize('name,mode', cases.PARITY)
def test_the_one_walk_equals_the_two_it_replaces(be, name, mode):
    """2. Bit for bit in the maps, by linearity within GRAD_TOL in the gradients."""
    cases.check_replaced_operators(be, name, mode)


@pytest.mark.parametrize('name,mode', cases.ALONE)
def test_terms_alone(be, name, mode):
    """3. The distortion term alone, the feature term alone, neither."""
    cases.check_terms_alone(be, name, mode)


def test_boundary_cases(be):
    """4. Retained buffers, poisoned scratch, n = 0, an offset of every depth."""
    cases.check_boundaries(be)


def test_refusals(be):
    """5. Every refusal raises with its text."""
    cases.check_refusals(be)


def test_two_kernel_k12_is_refused(sim_backend):
    cases.check_two_kernel_k12_is_refused(sim_backend)


def test_abi_refusals(be):
    """5. The bare C entry points, on the simulation and on the product library where it is built."""
    _lib, _ = helpers.backend_modules()
    for lib in [be.lib] + ([_lib.bind(_lib.DEFAULT_LIBRARY)] if _lib.DEFAULT_LIBRARY.exists() else []):
        cases.check_abi_refusals(lib, _lib)


def test_autograd_through_the_public_operator(be, operators_on_sim):
    """6. diff_rasterize_geometry itself on the simulation: what tests/test_gpu_geometry.py runs on the device."""
    cases.check_operator(operators_on_sim, be, 'partial_tiles')


def test_composed_graph_equals_the_two_renders(be, operators_on_sim):
    """7. Distortion + normal consistency + depth L1 through one render against the same loss through the operators it replaces."""
    cases.check_composed(operators_on_sim)


def test_training_iteration_with_the_geometry_render(be, operators_on_sim):
    """8. The harness."""
    cases.check_training_iteration()


def test_it_regularises(be, operators_on_sim):
    """9. Thirty Adam steps on X.mean() + E.mean() alone."""
    cases.check_regularises()


def test_public_names():
    import inspect
    import FasterGSCudaBackend as B
    from harness import trainer as T
    assert 'diff_rasterize_geometry' in B.__all__
    assert callable(T.render_image_training_geometry)
    assert inspect.signature(T.training_iteration).parameters['geometry_render'].default is False
    assert inspect.signature(B.diff_rasterize_geometry).parameters['normalized'].default is True
    c = aux.case('partial_tiles')
    args = [c['params'][k] for k in helpers.NAMES]
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.diff_rasterize_geometry(*args, torch.empty(0), aux.settings_of(c), torch.zeros(args[0].shape[0], 5))
    _lib, _ = helpers.backend_modules()
    assert {'fgs_blend_geometry', 'fgs_backward_geometry'} <= set(_lib.EXPORTED_SYMBOLS)
