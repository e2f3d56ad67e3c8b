"""The weighted L1 + DSSIM loss (per-pixel weights and masks; INTEGRATION.md 'Weighted loss') on the CPU simulation of the unmodified .hip sources: the fp64
model of the definition, the three call forms, the four invariants of the definition bit for bit, the C ABI's and the Backend's refusals, and the harness
(training_iteration(..., loss_weight=)). Definitions, reference, patterns and bars: tests/weighted_loss_cases.py; the same checks run on the MI355X in
tests/test_gpu_weighted_loss.py."""
import numpy as np
import pytest

import helpers
import weighted_loss_cases as cases

_id = lambda s: f'{s[0]}x{s[1]}'


@pytest.fixture(scope='module')
def be():
    return helpers.sim_backend(product=True)


@pytest.fixture
def operators_on_sim(be, monkeypatch):
    """The public operators, the optimizer and the harness (all unmodified) running on the simulation backend with CPU tensors."""
    import FasterGSCudaBackend.adam as A
    import FasterGSCudaBackend.bilagrid as G
    import FasterGSCudaBackend.rasterization as R
    import harness.loss as L
    for module in (R, A, G, L):
        monkeypatch.setattr(module, 'default_backend', lambda: be)
    for module in (R, G):
        monkeypatch.setattr(module, '_require_gpu', lambda t: None)


def test_patterns_are_what_they_claim():
    hole = cases.weight((33, 65), 'hole')
    rows, cols = np.where(hole == 0)
    assert cols.min() < 32 <= cols.max() and cols.max() - cols.min() + 1 > 11 and rows.max() - rows.min() + 1 > 11      # straddles x = 32, wider than a window
    one = cases.weight((70, 100), 'one_pixel')
    assert np.count_nonzero(one) == 1 and one[-1, -1] > 0
    for shape in cases.SHAPES:
        soft = cases.weight(shape, 'soft')
        assert soft.min() > 0 and soft.max() <= 2 and not cases.weight(shape, 'zeros').any()
        for pattern in cases.TRUTH_PATTERNS:
            assert cases.effective(cases.weight(shape, pattern)).sum() > 0


@pytest.mark.parametrize('pattern', cases.TRUTH_PATTERNS)
@pytest.mark.parametrize('shape', cases.SHAPES, ids=_id)
def test_sim_weighted_loss_matches_fp64(be, shape, pattern):
    cases.check_against_truth(be, 'cpu', shape, pattern, 'one_call')


def test_sim_weighted_loss_smooth_bright_three_way(be):
    cases.check_against_truth(be, 'cpu', (33, 65), 'soft', 'one_call', content='smooth_bright')


@pytest.mark.parametrize('shape', [(33, 65), (70, 100)], ids=_id)
def test_sim_weighted_three_forms_agree_bit_for_bit(be, shape):
    cases.check_forms_agree(be, 'cpu', shape)


def test_sim_weighted_upstream_scalars(be):
    cases.check_upstream_scalars(be, 'cpu')


@pytest.mark.parametrize('shape', cases.SHAPES, ids=_id)
def test_sim_ones_equal_the_unweighted_entry_points(be, shape):
    cases.check_ones_equal_unweighted(be, 'cpu', shape)


@pytest.mark.parametrize('pattern', ['hole', 'blocks', 'one_pixel'])
@pytest.mark.parametrize('shape', [(33, 65), (70, 100)], ids=_id)
def test_sim_ignored_pixels_get_no_gradient_and_are_never_read(be, shape, pattern):
    cases.check_ignored_pixels(be, 'cpu', shape, pattern, 'one_call')


def test_sim_ignored_pixels_split_form(be):
    cases.check_ignored_pixels(be, 'cpu', (38, 70), 'hole', 'split')


@pytest.mark.parametrize('shape', [(33, 65), (8, 300)], ids=_id)
def test_sim_scale_invariance(be, shape):
    cases.check_scale_invariance(be, 'cpu', shape)


@pytest.mark.parametrize('shape', [(5, 7), (33, 65)], ids=_id)
def test_sim_negative_and_nan_weights_count_as_zero(be, shape):
    cases.check_negative_nan(be, 'cpu', shape)


@pytest.mark.parametrize('shape', [(5, 7), (33, 65)], ids=_id)
def test_sim_all_zero_weights(be, shape):
    cases.check_zeros(be, 'cpu', shape)


@pytest.mark.parametrize('shape', [(33, 65), (70, 100)], ids=_id)
def test_sim_weighted_loss_does_not_read_scratch_it_did_not_write(be, shape):
    cases.check_scratch_independence(be, 'cpu', shape)


def test_sim_weighted_loss_is_reproducible(be):
    cases.check_reproducible(be, 'cpu', (70, 100))


@pytest.mark.parametrize('form', ['one_call', 'split'])
def test_sim_l1_term_alone_with_a_binary_mask(be, form):
    cases.check_l1_term_alone(be, 'cpu', (33, 65), form)


def test_sim_bool_and_integer_masks(be):
    cases.check_bool_mask(be, 'cpu')


def test_sim_refusals(be):
    cases.check_refusals(be, 'cpu', 'meta')


def test_sim_training_iteration_with_ones_is_the_unweighted_step(be, operators_on_sim):
    cases.check_training_iteration_ones('cpu', steps=2, exact_parameters=True)


def test_sim_training_iteration_hole_mask(be, operators_on_sim):
    cases.check_training_iteration_hole('cpu')


def test_sim_training_iteration_bilagrid_takes_the_weight(be, operators_on_sim):
    cases.check_training_iteration_bilagrid('cpu')
