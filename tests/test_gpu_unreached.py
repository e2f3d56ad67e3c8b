"""The backward gradients kernel and the fused backward + Adam kernel skip visible Gaussians that K11 never reached (csrc/preprocess_backward.hip:
gaussian_backward), on the MI355X. Scenes, premises and bars: tests/unreached_cases.py; the CPU-simulation twin is tests/test_unreached.py."""
import pytest

import unreached_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_wall_scene_gradients_zeros_statistics_and_flags(hip_backend):
    cases.check_backward(hip_backend, DEV)


def test_hot_gaussian_is_tested_behind_the_fold(hip_backend, oracle):
    cases.check_hot(hip_backend, oracle, DEV)


def test_optimizers_match_the_oracle_steps(hip_backend, monkeypatch):
    cases.check_optimizers(hip_backend, DEV, monkeypatch)


def test_depth_only_pass_keeps_its_gradients(hip_backend):
    cases.check_depth_only(hip_backend, DEV)
