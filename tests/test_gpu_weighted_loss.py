"""The weighted L1 + DSSIM loss kernels (csrc/loss.hip, WEIGHTED instantiations) on the MI355X: the cases, bars and checks of tests/weighted_loss_cases.py,
which tests/test_weighted_loss.py runs on the CPU simulation. Each case is a few launches of microseconds and the fp64 model on the host."""
import pytest

import weighted_loss_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_id = lambda s: f'{s[0]}x{s[1]}'


@pytest.mark.parametrize('pattern', cases.TRUTH_PATTERNS)
@pytest.mark.parametrize('shape', cases.SHAPES, ids=_id)
def test_gpu_weighted_loss_matches_fp64(hip_backend, shape, pattern):
    cases.check_against_truth(hip_backend, DEV, shape, pattern, 'one_call')


def test_gpu_weighted_loss_smooth_bright_three_way(hip_backend):
    cases.check_against_truth(hip_backend, DEV, (33, 65), 'soft', 'one_call', content='smooth_bright')


@pytest.mark.parametrize('shape', [(33, 65), (70, 100)], ids=_id)
def test_gpu_weighted_three_forms_agree_bit_for_bit(hip_backend, shape):
    cases.check_forms_agree(hip_backend, DEV, shape)


def test_gpu_weighted_upstream_scalars(hip_backend):
    cases.check_upstream_scalars(hip_backend, DEV)


@pytest.mark.parametrize('shape', cases.SHAPES + [cases.LARGE], ids=_id)
def test_gpu_ones_equal_the_unweighted_entry_points(hip_backend, shape):
    cases.check_ones_equal_unweighted(hip_backend, DEV, shape)


@pytest.mark.parametrize('pattern', ['hole', 'blocks', 'one_pixel'])
@pytest.mark.parametrize('shape', [(33, 65), (70, 100)], ids=_id)
def test_gpu_ignored_pixels_get_no_gradient_and_are_never_read(hip_backend, shape, pattern):
    cases.check_ignored_pixels(hip_backend, DEV, shape, pattern, 'one_call')


def test_gpu_ignored_pixels_split_form(hip_backend):
    cases.check_ignored_pixels(hip_backend, DEV, (38, 70), 'hole', 'split')


def test_gpu_weighted_loss_at_size(hip_backend):
    """360 x 640: 720 forward partials and 240 weight sums per reduction."""
    cases.check_against_truth(hip_backend, DEV, cases.LARGE, 'hole', 'one_call')
    cases.check_ignored_pixels(hip_backend, DEV, cases.LARGE, 'hole', 'one_call')


@pytest.mark.parametrize('shape', [(33, 65), (8, 300)], ids=_id)
def test_gpu_scale_invariance(hip_backend, shape):
    cases.check_scale_invariance(hip_backend, DEV, shape)


@pytest.mark.parametrize('shape', [(5, 7), (33, 65)], ids=_id)
def test_gpu_negative_and_nan_weights_count_as_zero(hip_backend, shape):
    cases.check_negative_nan(hip_backend, DEV, shape)


@pytest.mark.parametrize('shape', [(5, 7), (33, 65)], ids=_id)
def test_gpu_all_zero_weights(hip_backend, shape):
    cases.check_zeros(hip_backend, DEV, shape)


@pytest.mark.parametrize('shape', [(33, 65), (70, 100)], ids=_id)
def test_gpu_weighted_loss_does_not_read_scratch_it_did_not_write(hip_backend, shape):
    cases.check_scratch_independence(hip_backend, DEV, shape)


@pytest.mark.parametrize('shape', [(70, 100), cases.LARGE], ids=_id)
def test_gpu_weighted_loss_is_reproducible(hip_backend, shape):
    cases.check_reproducible(hip_backend, DEV, shape)


@pytest.mark.parametrize('form', ['one_call', 'split'])
def test_gpu_l1_term_alone_with_a_binary_mask(hip_backend, form):
    cases.check_l1_term_alone(hip_backend, DEV, (33, 65), form)


def test_gpu_bool_and_integer_masks(hip_backend):
    cases.check_bool_mask(hip_backend, DEV)


def test_gpu_refusals(hip_backend):
    cases.check_refusals(hip_backend, DEV, 'cpu')


def test_gpu_training_iteration_with_ones_gives_the_unweighted_loss(hip_backend):
    cases.check_training_iteration_ones(DEV, steps=1, exact_parameters=False)


def test_gpu_training_iteration_hole_mask(hip_backend):
    cases.check_training_iteration_hole(DEV)


def test_gpu_training_iteration_bilagrid_takes_the_weight(hip_backend):
    cases.check_training_iteration_bilagrid(DEV)
