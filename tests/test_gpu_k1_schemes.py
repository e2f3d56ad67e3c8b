"""K1's tile-counting schemes and K13's exhibits on the MI355X (libfgs_hip_dev.so), and the product library's one scheme against the dev library's
default: definitions, scenes and claims in tests/k1_scheme_cases.py and tests/adam_exhibit_cases.py. Each K1 case is two passes over at most 700 Gaussians."""
import functools

import pytest

import adam_exhibit_cases as adam
import k1_scheme_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@functools.lru_cache(maxsize=None)
def _default(be, name):
    ref = cases.run_scheme(be, cases.DEFAULT, name, device=DEV)     # computed once per scene, shared by the cases below: read-only
    cases.sorted_lists(ref, name)
    return ref


@pytest.mark.parametrize('scheme', cases.SCHEMES)
@pytest.mark.parametrize('name', cases.SCENES)
def test_every_scheme_counts_what_the_flattened_count_counts_on_device(hip_dev_backend, name, scheme):
    cases.check_same(cases.run_scheme(hip_dev_backend, scheme, name, device=DEV), _default(hip_dev_backend, name), DEV, (name, scheme))


@pytest.mark.parametrize('name', cases.PRODUCT_SCENES)
def test_product_library_counts_what_the_dev_default_counts_on_device(hip_backend, hip_dev_backend, name):
    assert not hasattr(hip_backend.lib, 'fgs_debug_set_option')
    cases.check_same(cases.run(hip_backend, name, device=DEV), _default(hip_dev_backend, name), DEV, (name, 'product'))


def test_option_5_refuses_what_is_no_scheme_on_device(hip_dev_backend):
    for value in (33, -1):
        assert hip_dev_backend.lib.fgs_debug_set_option(5, value) != 0
    cases.check_same(cases.run(hip_dev_backend, 'one', device=DEV), _default(hip_dev_backend, 'one'), DEV, 'after the refusals')


@functools.lru_cache(maxsize=None)
def _adam_default(be):
    return adam.step_with(be, {}, device=DEV)


@pytest.mark.parametrize('options', adam.EXHIBITS, ids=adam.IDS)
def test_every_adam_exhibit_steps_what_the_default_steps_on_device(hip_dev_backend, options):
    adam.check_same(adam.step_with(hip_dev_backend, options, device=DEV), _adam_default(hip_dev_backend), options)


def test_product_library_steps_what_the_dev_default_steps_on_device(hip_backend, hip_dev_backend):
    adam.check_same(adam.step(hip_backend, device=DEV), _adam_default(hip_dev_backend), 'product')
