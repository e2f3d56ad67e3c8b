"""CPU-simulation twin of tests/test_gpu_k12_folds.py: the same shapes and checks (tests/k12_fold_cases.py) on the simulation build of the kernel sources."""
import pytest

import k12_fold_cases as cases


@pytest.mark.parametrize('n,K', cases.SHAPES)
def test_sim_single_kernel_equals_two_kernels_and_reference(sim_backend, oracle, n, K):
    cases.check_single_kernel_against_two_kernels_and_reference(sim_backend, oracle, 'cpu', n, K)


@pytest.mark.parametrize('unaligned', [False, True])
@pytest.mark.parametrize('n,K', cases.SHAPES)
def test_sim_fused_equals_backward_then_adam(sim_backend, n, K, unaligned):
    cases.check_fused_equals_backward_then_adam(sim_backend, 'cpu', n, K, unaligned)


@pytest.mark.parametrize('n,K', cases.SHAPES)
def test_sim_two_kernel_fused_equals_backward_then_adam(sim_backend, n, K):
    cases.check_fused_equals_backward_then_adam(sim_backend, 'cpu', n, K, False, single_kernel=False)


@pytest.mark.parametrize('n,K', cases.SHAPES)
def test_sim_sharded_fused_equals_unfused(sim_backend, n, K):
    cases.check_sharded_fused_equals_unfused(sim_backend, 'cpu', n, K)
