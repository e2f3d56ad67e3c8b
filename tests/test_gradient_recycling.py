"""The backward gradients kernel's promise going in (`prior_blocks`, include/fgs_hip.h: fgs_backward_recycled) and the autograd path that writes into the
arena of the previous pass, on the CPU simulation of the kernel sources. Scenes, checks and bars: tests/gradient_recycling_cases.py;
tests/test_gpu_gradient_recycling.py runs the same functions on the MI355X."""
import pytest

import gradient_recycling_cases as checks

DEV = 'cpu'


def test_sim_the_two_views_reach_different_blocks(sim_backend):
    checks.check_views_differ(sim_backend, DEV)


def test_sim_pass_with_a_promise_equals_the_plain_pass(sim_backend):
    checks.check_equal_to_plain(sim_backend, DEV)


@pytest.mark.parametrize('active,rest', checks.SH_CASES)
def test_sim_skipped_written_and_sentinel_blocks(sim_backend, active, rest):
    assert rest == active - 1
    checks.check_blocks(sim_backend, DEV, K=active)


def test_sim_blocks_of_unaligned_gradient_tensors(sim_backend):
    checks.check_blocks(sim_backend, DEV, odd=True)


def test_sim_single_block(sim_backend):
    checks.check_single_block(sim_backend, DEV)


def test_sim_refusals(sim_backend):
    checks.check_refusals(sim_backend, DEV)


def test_sim_two_kernel_form_ignores_the_promise(sim_backend):
    checks.check_two_kernel_form(sim_backend, DEV)


def test_sim_recycling_changes_no_result(sim_backend, monkeypatch):
    checks.check_recycling_changes_nothing(sim_backend, DEV, monkeypatch)


@pytest.mark.parametrize('name', sorted(checks.INTERFERENCE))
def test_sim_interference_is_seen(sim_backend, monkeypatch, name):
    checks.check_interference(sim_backend, DEV, monkeypatch, name)


def test_sim_growing_model_takes_new_memory(sim_backend, monkeypatch):
    checks.check_growing_model(sim_backend, DEV, monkeypatch)


def test_sim_second_model_takes_the_spare(sim_backend, monkeypatch):
    checks.check_second_model_takes_the_spare(sim_backend, DEV, monkeypatch)
