"""fgs_blend_features / fgs_backward_features on the CPU simulation of the product library (the unmodified .hip sources): the differentiable
feature-channel blend of the training render. Definitions, reference, upstream gradients and bars: tests/feature_cases.py. The same comparisons run on
the MI355X in tests/test_gpu_feature_render.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import aux_grad_cases as aux
import feature_cases as cases
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
def test_reference_without_a_feature_gradient_is_the_trusted_one(name):
    """First of all, for every case: gF = 0 reproduces aux_grad_cases.reference_rgb to 1e-12."""
    cases.check_reference_without_feature_gradient(name)


@pytest.mark.parametrize('name,n_channels', cases.PARITY)
def test_map_image_and_gradients_match_the_fp64_reference(be, name, n_channels):
    """1. Map on the kept pixels, exact zeros where nothing was blended, the image bit-identical to plain `forward`, the six gradients and grad_features
    against fp64 with gC and gF both non-zero."""
    cases.check_against_reference(be, name, n_channels)


def test_identities(be):
    """2. Ones channel = alpha, z channel = expected depth (maps and gradients), three colour channels = the image."""
    cases.check_identities(be)


def test_workaround_parity(be):
    """3. grad_features = grad_sh0 / C0 of the three-channel diff_rasterize formulation this operator replaces."""
    cases.check_workaround_parity(be)


def test_detached_geometry_no_feature_gradient_and_retained_buffers(be):
    """4."""
    cases.check_detached_and_retained(be)


def test_maps_and_gradients_do_not_depend_on_stale_scratch_memory(be):
    """grad_features is handed over uninitialised and the buffers arrive poisoned: the entry point zeroes what its atomics add into."""
    c = aux.case('partial_tiles')
    f, gF = cases.features('partial_tiles', 5), cases.grad_map('partial_tiles', 5)
    clean = cases.run(be, c, f, c['gC'], gF)
    out = cases.run(helpers.poisoned(be), c, f, c['gC'], gF)
    for k in ('image', 'map', 'features') + helpers.GRAD_KEYS:
        assert helpers.rel_inf(out[k], clean[k]) < 1e-6, k


def test_refusals_and_no_gaussians(be):
    """5. Every refusal raises with its text; n = 0 gives a zero map."""
    cases.check_errors_and_empty(be)


def test_autograd_through_the_public_operator(be, operator_on_sim):
    """5. diff_rasterize_features itself on the simulation: what tests/test_gpu_feature_render.py runs on the device."""
    cases.check_operator(operator_on_sim, be, 'partial_tiles')


def test_abi_refusals(be):
    """The C entry points refuse by themselves, before anything is launched; the ABI version stays 3."""
    _lib, _ = helpers.backend_modules()
    st = _lib.ForwardState()
    S = _lib.Settings(1, 1, 1, 16, 15, 128, 128, 1.0, 1.0, 0.0, 0.0, 0.2, 100.0, 0)
    libs = [be.lib] + ([_lib.bind(_lib.DEFAULT_LIBRARY)] if _lib.DEFAULT_LIBRARY.exists() else [])
    for lib in libs:
        for bad in (0, 65, -1):
            assert lib.fgs_blend_features(1, bad, 1, 1, 1, 10, C.byref(S), C.byref(st), 1, None) == -1
            assert b'n_channels' in lib.fgs_last_error() and b'1..64' in lib.fgs_last_error()
        assert lib.fgs_blend_features(1, 4, 1, 1, 1, 10, C.byref(S), C.byref(st), None, None) == -1
        assert b'NULL feature_map' in lib.fgs_last_error()
        assert lib.fgs_blend_features(None, 4, 1, 1, 1, 10, C.byref(S), C.byref(st), 1, None) == -1
        assert b'NULL features' in lib.fgs_last_error()
        for bit, text in ((4, b'fgs_forward_async'), (8, b'record')):
            flagged = _lib.ForwardState(0, 0, 0, bit)
            assert lib.fgs_blend_features(1, 4, 1, 1, 1, 10, C.byref(S), C.byref(flagged), 1, None) == -1
            assert text in lib.fgs_last_error()
        assert lib.fgs_abi_version() == 3


def test_public_names():
    import FasterGSCudaBackend as B
    from harness.trainer import render_image_training_features      # noqa: F401
    assert 'diff_rasterize_features' in B.__all__
    c = aux.case('partial_tiles')
    args = [c['params'][k] for k in helpers.NAMES]
    f = torch.as_tensor(cases.features('partial_tiles', 5))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.diff_rasterize_features(*args, torch.empty(0), aux.settings_of(c), f)
    _lib, _ = helpers.backend_modules()
    assert {'fgs_blend_features', 'fgs_backward_features'} <= set(_lib.EXPORTED_SYMBOLS)
