"""Reached-block flags of the backward gradients kernel and their hand-over to the optimizer (include/fgs_hip.h: fgs_backward_reached) on the MI355X.
Scenes, checks and bars: tests/test_reached_blocks.py, which runs the same functions on the CPU simulation."""
import pytest

import test_reached_blocks as checks

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_flags_are_exact(hip_backend):
    checks.check_flags(hip_backend, DEV)


def test_rows_of_unreached_blocks_are_zero(hip_backend):
    checks.check_promise(hip_backend, DEV)


def test_adam_is_bit_exact_with_the_reached_flags(hip_backend):
    checks.check_adam(hip_backend, DEV)


def test_hot_gaussian_flags_its_block(hip_backend):
    checks.check_hot(hip_backend, DEV)


def test_depth_pass_keeps_the_promise(hip_backend):
    checks.check_depth(hip_backend, DEV)


def test_bounds_and_single_arrays(hip_backend):
    checks.check_bounds(hip_backend, DEV)


def test_handover_through_autograd(hip_backend, monkeypatch):
    checks.check_autograd(hip_backend, DEV, monkeypatch)
