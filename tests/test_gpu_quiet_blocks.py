"""Quiet-block flags of the optimizer (include/fgs_hip.h: fgs_adam_step_multi_quiet, fgs_adam_quiet_scan) on the MI355X.
Shapes, checks and bars: tests/test_quiet_blocks.py, which runs the same functions on the CPU simulation."""
import pytest

import test_quiet_blocks as checks

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('n', [1483, 64, 1])
def test_quiet_entry_equals_the_live_entry(hip_backend, n):
    checks.check_equivalence(hip_backend, DEV, n)


def test_scan_matches_a_torch_reduction(hip_backend):
    checks.check_scan(hip_backend, DEV)


def test_eps_zero_and_missing_live_flags_skip_nothing(hip_backend):
    checks.check_eps_zero(hip_backend, DEV)


def test_first_step_flags_are_ones_and_equal_the_scan(hip_backend, monkeypatch):
    checks.check_first_step(hip_backend, DEV, monkeypatch)


def test_foreign_writes_of_the_moments_rescan(hip_backend, monkeypatch):
    checks.check_invalidation(hip_backend, DEV, monkeypatch)


def test_hand_set_gradients_take_the_plain_step(hip_backend, monkeypatch):
    checks.check_hand_set_gradients(hip_backend, DEV, monkeypatch)


def test_sentinel_steps_a_quiet_block(hip_backend, monkeypatch):
    checks.check_sentinel(hip_backend, DEV, monkeypatch)
