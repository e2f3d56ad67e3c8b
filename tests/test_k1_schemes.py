"""K1's tile-counting schemes and K13's exhibits on the CPU simulation (dev flavour of the sources), and the product flavour's one scheme against it:
definitions, scenes and claims in tests/k1_scheme_cases.py and tests/adam_exhibit_cases.py."""
import functools

import pytest

import adam_exhibit_cases as adam
import k1_scheme_cases as cases


@functools.lru_cache(maxsize=None)
def _default(be, name):
    ref = cases.run_scheme(be, cases.DEFAULT, name)             # computed once per scene, shared by the cases below: read-only
    cases.sorted_lists(ref, name)
    return ref


@pytest.mark.parametrize('scheme', cases.SCHEMES)
@pytest.mark.parametrize('name', cases.SCENES)
def test_every_scheme_counts_what_the_flattened_count_counts(sim_backend, name, scheme):
    cases.check_same(cases.run_scheme(sim_backend, scheme, name), _default(sim_backend, name), 'cpu', (name, scheme))


@pytest.mark.parametrize('name', cases.PRODUCT_SCENES)
def test_product_flavour_counts_what_the_dev_default_counts(sim_product_backend, sim_backend, name):
    """The product flavour's preprocess_body has the flattened count alone (csrc/preprocess.hip)."""
    assert not hasattr(sim_product_backend.lib, 'fgs_debug_set_option')
    cases.check_same(cases.run(sim_product_backend, name), _default(sim_backend, name), 'cpu', (name, 'product'))


def test_option_5_refuses_what_is_no_scheme(sim_backend):
    for value in (33, -1):
        assert sim_backend.lib.fgs_debug_set_option(5, value) != 0
    cases.check_same(cases.run(sim_backend, 'one'), _default(sim_backend, 'one'), 'cpu', 'after the refusals')      # and left the default in place


@functools.lru_cache(maxsize=None)
def _adam_default(be):
    return adam.step_with(be, {})


@pytest.mark.parametrize('options', adam.EXHIBITS, ids=adam.IDS)
def test_every_adam_exhibit_steps_what_the_default_steps(sim_backend, options):
    adam.check_same(adam.step_with(sim_backend, options), _adam_default(sim_backend), options)


def test_product_flavour_steps_what_the_dev_default_steps(sim_product_backend, sim_backend):
    adam.check_same(adam.step(sim_product_backend), _adam_default(sim_backend), 'product')
