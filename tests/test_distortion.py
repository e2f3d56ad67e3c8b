"""fgs_blend_distortion / fgs_backward_distortion on the CPU simulation of the product library (the unmodified .hip sources): the differentiable
depth-distortion map of the training render. Definitions, reference, upstream gradients and bars: tests/distortion_cases.py. The same comparisons run
on the MI355X in tests/test_gpu_distortion.py."""
import pytest
import torch

import aux_grad_cases as aux
import distortion_cases as cases
import helpers


@pytest.fixture(scope='module')
def be():
    return helpers.sim_backend(product=True)


@pytest.fixture()
def operator_on_sim(be, monkeypatch):
    """The public operators (FasterGSCudaBackend.rasterization, unmodified) running on the simulation backend with CPU tensors."""
    import FasterGSCudaBackend as B
    import FasterGSCudaBackend.rasterization as R
    monkeypatch.setattr(R, 'default_backend', lambda: be)
    monkeypatch.setattr(R, '_require_gpu', lambda t: None)
    return B


@pytest.mark.parametrize('name', list(aux.CASES))
def test_reference_is_pinned(name):
    """First of all, for every case: gX = 0 reproduces aux_grad_cases.reference_rgb to 1e-12, and the prefix form equals the absolute-value form to
    1e-12 in both modes (t is ordered along the walk)."""
    cases.check_reference_pins(name)


@pytest.mark.parametrize('name,mode', cases.PARITY)
def test_map_image_and_gradients_match_the_fp64_reference(be, name, mode):
    """1. Map on the kept pixels, exact zeros where fewer than two Gaussians were blended, the image bit-identical to plain `forward`, the six gradients
    against fp64 with gC and gX both non-zero, and a rerun."""
    cases.check_against_reference(be, name, mode)


@pytest.mark.parametrize('name,mode', cases.ALONE)
def test_gradients_of_the_distortion_term_alone(be, name, mode):
    """1b. gC = 0: the term's own gradients against fp64, not beside the colour term's."""
    cases.check_term_alone(be, name, mode)


def test_state_planes(be):
    """2. Plane 1 = alpha; an offset of every depth leaves the linear X unchanged (the state is kept in a shifted t)."""
    cases.check_state(be)


def test_boundary_cases(be):
    """3. gX = None, gC = 0, retained buffers, poisoned scratch."""
    cases.check_boundaries(be)


def test_refusals_and_no_gaussians(be):
    """4. Every refusal raises with its text; n = 0 gives a zero map."""
    cases.check_errors_and_empty(be)


def test_abi_refusals(be):
    """4. The bare C entry points, on the simulation and on the product library where it is built."""
    _lib, _ = helpers.backend_modules()
    for lib in [be.lib] + ([_lib.bind(_lib.DEFAULT_LIBRARY)] if _lib.DEFAULT_LIBRARY.exists() else []):
        cases.check_abi_refusals(lib, _lib)


def test_autograd_through_the_public_operator(be, operator_on_sim):
    """5. diff_rasterize_distortion itself on the simulation: what tests/test_gpu_distortion.py runs on the device."""
    cases.check_operator(operator_on_sim, be, 'partial_tiles')


def test_public_names():
    import inspect
    import FasterGSCudaBackend as B
    from harness import trainer as T
    assert 'diff_rasterize_distortion' in B.__all__
    assert callable(T.render_image_training_distortion)
    sig = inspect.signature(T.training_iteration).parameters
    assert sig['distortion_weight'].default == 0.0 and sig['distortion_normalized'].default is True
    c = aux.case('partial_tiles')
    args = [c['params'][k] for k in helpers.NAMES]
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.diff_rasterize_distortion(*args, torch.empty(0), aux.settings_of(c))
    _lib, _ = helpers.backend_modules()
    assert {'fgs_blend_distortion', 'fgs_backward_distortion'} <= set(_lib.EXPORTED_SYMBOLS)
