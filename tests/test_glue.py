"""CPU-simulation twin of tests/test_gpu_glue.py: the same shapes and checks (tests/glue_cases.py) through the glue bound to the simulation of the product
flavour of the kernel sources. The one branch it cannot reach is a tensor on another device than the parameters'."""
import pytest

import glue_cases as cases

DEV = 'cpu'


def test_sim_parameter_refusals(sim_product_backend):
    cases.check_parameter_refusals(sim_product_backend, DEV)


def test_sim_block_flag_refusals(sim_product_backend):
    cases.check_block_flag_refusals(sim_product_backend, DEV)


def test_sim_gradient_and_densification_refusals(sim_product_backend):
    cases.check_gradient_and_densification_refusals(sim_product_backend, DEV)


def test_sim_record_refusals(sim_product_backend):
    cases.check_record_refusals(sim_product_backend, DEV)


def test_sim_accepted_forms(sim_product_backend):
    cases.check_accepted_forms(sim_product_backend, DEV)


@pytest.mark.parametrize('kind', cases.KINDS)
def test_sim_backward_forms(sim_product_backend, kind):
    cases.check_backward_forms(sim_product_backend, DEV, kind)


@pytest.mark.parametrize('kind', cases.KINDS)
def test_sim_loss_and_inference_forms(sim_product_backend, kind):
    cases.check_loss_and_inference_forms(sim_product_backend, DEV, kind)
