"""The validation branches and call forms of the torch glue (FasterGSCudaBackend/_backend.py) at their smallest shapes, on the MI355X. Shapes, checks and
bars: tests/glue_cases.py; the CPU-simulation twin is tests/test_glue.py. Here the refusals also get a flag array and a gradient that live on the host."""
import pytest

import glue_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_parameter_refusals(hip_backend):
    cases.check_parameter_refusals(hip_backend, DEV)


def test_block_flag_refusals(hip_backend):
    cases.check_block_flag_refusals(hip_backend, DEV, other_device='cpu')


def test_gradient_and_densification_refusals(hip_backend):
    cases.check_gradient_and_densification_refusals(hip_backend, DEV, other_device='cpu')


def test_record_refusals(hip_backend):
    cases.check_record_refusals(hip_backend, DEV)


def test_accepted_forms(hip_backend):
    cases.check_accepted_forms(hip_backend, DEV)


@pytest.mark.parametrize('kind', cases.KINDS)
def test_backward_forms(hip_backend, kind):
    cases.check_backward_forms(hip_backend, DEV, kind)


@pytest.mark.parametrize('kind', cases.KINDS)
def test_loss_and_inference_forms(hip_backend, kind):
    cases.check_loss_and_inference_forms(hip_backend, DEV, kind)
