"""The backward gradients kernel's promise going in (`prior_blocks`) and the recycled gradient arena of the autograd path on the MI355X.
Scenes, checks and bars: tests/gradient_recycling_cases.py; tests/test_gradient_recycling.py runs the same functions on the CPU simulation."""
import pytest

import gradient_recycling_cases as checks

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_the_two_views_reach_different_blocks(hip_backend):
    checks.check_views_differ(hip_backend, DEV)


def test_pass_with_a_promise_equals_the_plain_pass(hip_backend):
    checks.check_equal_to_plain(hip_backend, DEV)


@pytest.mark.parametrize('active,rest', checks.SH_CASES)
def test_skipped_written_and_sentinel_blocks(hip_backend, active, rest):
    assert rest == active - 1
    checks.check_blocks(hip_backend, DEV, K=active)


def test_blocks_of_unaligned_gradient_tensors(hip_backend):
    checks.check_blocks(hip_backend, DEV, odd=True)


def test_single_block(hip_backend):
    checks.check_single_block(hip_backend, DEV)


def test_refusals(hip_backend):
    checks.check_refusals(hip_backend, DEV)


def test_recycling_changes_no_result(hip_backend, monkeypatch):
    checks.check_recycling_changes_nothing(hip_backend, DEV, monkeypatch)


@pytest.mark.parametrize('name', sorted(checks.INTERFERENCE))
def test_interference_is_seen(hip_backend, monkeypatch, name):
    checks.check_interference(hip_backend, DEV, monkeypatch, name)


def test_growing_model_takes_new_memory(hip_backend, monkeypatch):
    checks.check_growing_model(hip_backend, DEV, monkeypatch)


def test_second_model_takes_the_spare(hip_backend, monkeypatch):
    checks.check_second_model_takes_the_spare(hip_backend, DEV, monkeypatch)
