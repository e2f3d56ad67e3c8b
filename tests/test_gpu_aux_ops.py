"""update_3d_filter / relocation_adjustment / add_noise (csrc/aux_ops.hip) on the MI355X against the 50-digit and fp64 models of tests/aux_op_cases.py,
three-way with the fp32 numpy restatement: the cases, bars and checks that tests/test_aux_ops.py runs on the CPU simulation. Every call is one launch of at
most 3100 lanes; the decimal model is evaluated once per process. Measured figures: profiles/aux_ops_tolerance_slack.txt."""
import pytest

import aux_op_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('n', cases.ROW_COUNTS)
def test_gpu_aux_ops_row_counts_and_guard_rows(hip_backend, oracle, n):
    cases.check_row_counts(hip_backend, oracle, DEV, n)


def test_gpu_relocation_matches_decimal_model(hip_backend, oracle):
    cases.check_relocation_against_model(hip_backend, oracle, DEV)


def test_gpu_relocation_clamp_and_dtypes(hip_backend, oracle):
    cases.check_relocation_clamp_and_dtypes(hip_backend, oracle, DEV)


def test_gpu_relocation_saturated_opacity_small_counts(hip_backend, oracle):
    cases.check_relocation_saturated_opacity(hip_backend, oracle, DEV)


def test_gpu_add_noise_matches_fp64_model(hip_backend, oracle):
    cases.check_add_noise_against_model(hip_backend, oracle, DEV)


def test_gpu_add_noise_thresholds_and_opaque_rows(hip_backend, oracle):
    cases.check_add_noise_thresholds(hip_backend, oracle, DEV)


def test_gpu_add_noise_public_wrapper_draws_the_seeded_noise(hip_backend):
    cases.check_public_add_noise(hip_backend, DEV)


@pytest.mark.parametrize('principal_point', cases.EXACT_PRINCIPAL_POINTS, ids=('centred', 'off-centre'))
def test_gpu_3d_filter_exact_boundaries(hip_backend, oracle, principal_point):
    cases.check_filter_exact_boundaries(hip_backend, oracle, DEV, principal_point)


def test_gpu_3d_filter_two_views_leave_the_minimum(hip_backend, oracle):
    cases.check_filter_two_views(hip_backend, oracle, DEV)


def test_gpu_3d_filter_random_scene_matches_fp64_model(hip_backend, oracle):
    cases.check_filter_random_scene(hip_backend, oracle, DEV)
