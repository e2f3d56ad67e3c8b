"""The normal-consistency regulariser on the CPU simulation of the product library (the unmodified .hip sources): fgs_surface_features,
fgs_normal_consistency, their backward passes, the public operators and the harness. Definitions, reference, cases and bars: tests/normal_cases.py.
The same comparisons run on the MI355X in tests/test_gpu_normal_consistency.py."""
import pytest
import torch

import helpers
import normal_cases as cases


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


def test_cases_are_well_conditioned():
    """First of all: 30 % .. 80 % of the interior pixels are valid, and the definitions in fp32 torch stay below 1e-5 of their fp64 evaluation."""
    cases.check_cases_are_well_conditioned()


@pytest.mark.parametrize('name', list(cases.IMAGE_CASES))
def test_image_space_matches_the_fp64_reference(be, name):
    """1. E, gN_r, gD, gA at rel_inf < 1e-4; `hole`: A = 0 over a block, no NaN, exact zeros; `exact`: min_alpha is a value A takes, identical masks."""
    cases.check_image_parity(be, name)


def test_degenerate_shapes(be):
    """2. 1 x 1, 2 x 5, 5 x 2: zeros; 3 x 3: one interior pixel; gE = 0: gM exactly 0."""
    cases.check_degenerate_shapes(be)


@pytest.mark.parametrize('n', cases.GAUSSIAN_COUNTS)
def test_surface_features_match_the_fp64_reference(be, n):
    """3. features, grad_rotations, grad_means at rel_inf < 1e-4; grad_rotations is orthogonal to the quaternion."""
    cases.check_gaussian_parity(be, n)


def test_no_gaussians(be):
    cases.check_no_gaussians(be)


def test_surface_feature_edges(be):
    """3. Scale ties, a . v = 0, a Gaussian behind the camera, a longer quaternion."""
    cases.check_gaussian_edges(be)


def test_reproducible_and_complete(be):
    """4. Two runs bit-identical, a gradient that is not requested leaves the other alone, NaN-filled outputs are overwritten."""
    cases.check_reproducible_and_complete(be)


def test_refusals(be):
    """5. On the simulation and on the product library where it is built (its refusals come before any launch)."""
    cases.check_refusals(be)


def test_abi_refusals_of_the_product_library():
    _lib, _backend = helpers.backend_modules()
    if _lib.DEFAULT_LIBRARY.exists():
        lib = _lib.bind(_lib.DEFAULT_LIBRARY)
        assert lib.fgs_normal_consistency(None, 4, 4, 1.0, 1.0, 0.0, 0.0, 0.5, None, None, None) == -1 and b'NULL' in lib.fgs_last_error()
        assert lib.fgs_surface_features(None, None, None, -1, None, None, None, None) == -1 and b'negative' in lib.fgs_last_error()
        assert lib.fgs_abi_version() == 3


def test_public_operators(be, operators_on_sim):
    """6. The composition against the fp32 torch restatement at 1e-5."""
    cases.check_operators(operators_on_sim, be)


def test_public_names():
    import inspect
    import FasterGSCudaBackend as B
    from FasterGSCudaBackend import _C
    from harness import trainer as T
    assert {'gaussian_surface_features', 'normal_consistency'} <= set(B.__all__) and not hasattr(_C, 'normal_consistency')
    assert callable(T.render_image_training_normals)
    sig = inspect.signature(T.training_iteration).parameters
    assert sig['normal_weight'].default == 0.0 and sig['normal_min_alpha'].default == 0.5
    assert inspect.signature(B.normal_consistency).parameters['min_alpha'].default == 0.5
    _lib, _ = helpers.backend_modules()
    assert {'fgs_surface_features', 'fgs_surface_features_backward', 'fgs_normal_consistency', 'fgs_normal_consistency_backward'} <= set(_lib.EXPORTED_SYMBOLS)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.normal_consistency(torch.zeros(5, 4, 4), cases.settings_for((4, 4), (4.0, 4.0, 2.0, 2.0)))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.gaussian_surface_features(torch.zeros(1, 3), torch.zeros(1, 3), torch.ones(1, 4), torch.eye(4), torch.zeros(3))


def test_training_iteration_equals_the_step_composed_by_hand(be, operators_on_sim):
    """7. Exact on the simulation; normal_weight = 0 is the plain step; the refused combinations raise."""
    cases.check_training_iteration(be)


def test_it_regularises(be, operators_on_sim):
    """8. Perturbed flat disks on a plane, rotations only: E.mean() falls below half of its start value."""
    cases.check_regularises()
