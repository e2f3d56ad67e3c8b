"""The folded helpers of K12 (csrc/preprocess_backward.hip, csrc/fgs_adam.h) at their smallest shapes, on the MI355X. Shapes, checks and bars:
tests/k12_fold_cases.py; the CPU-simulation twin is tests/test_k12_folds.py."""
import pytest

import k12_fold_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('n,K', cases.SHAPES)
def test_single_kernel_equals_two_kernels_and_reference(hip_dev_backend, oracle, n, K):
    cases.check_single_kernel_against_two_kernels_and_reference(hip_dev_backend, oracle, DEV, n, K)


@pytest.mark.parametrize('unaligned', [False, True])
@pytest.mark.parametrize('n,K', cases.SHAPES)
def test_fused_equals_backward_then_adam(hip_backend, n, K, unaligned):
    cases.check_fused_equals_backward_then_adam(hip_backend, DEV, n, K, unaligned)


@pytest.mark.parametrize('n,K', cases.SHAPES)
def test_two_kernel_fused_equals_backward_then_adam(hip_dev_backend, n, K):
    cases.check_fused_equals_backward_then_adam(hip_dev_backend, DEV, n, K, False, single_kernel=False)


@pytest.mark.parametrize('n,K', cases.SHAPES)
def test_sharded_fused_equals_unfused(hip_backend, n, K):
    cases.check_sharded_fused_equals_unfused(hip_backend, DEV, n, K)
