"""K13's span workgroups (csrc/adam.hip) on the MI355X: the product library and the dev library at C = 2, 16 and 32 against the oracle's dense step
(rel_inf < 1e-6) and, bit for bit, against the dev library at C = 1. Cases, shapes and bars: tests/adam_span_cases.py, which tests/test_adam_spans.py
runs on the CPU simulation."""
import pytest

import adam_span_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_parent = {}


def parent(hip_dev_backend, what, n=None):
    """(b), computed once: the dev library at C = 1."""
    if (what, n) not in _parent:
        _parent[(what, n)] = cases.run_flagless(hip_dev_backend, DEV, 1) if what == 'flagless' else cases.run_model(hip_dev_backend, DEV, n, 1)
    return _parent[(what, n)]


def test_flagless_groups_product(hip_backend, hip_dev_backend, oracle):
    got = cases.run_flagless(hip_backend, DEV)
    cases.close_to_oracle(got, cases.flagless_oracle(oracle), 'oracle')
    cases.same_bits(got, parent(hip_dev_backend, 'flagless'), 'C = 1')


@pytest.mark.parametrize('c', [1, 2, 16, 32])
def test_flagless_groups_dev_option(hip_dev_backend, oracle, c):
    got = cases.run_flagless(hip_dev_backend, DEV, c)
    cases.close_to_oracle(got, cases.flagless_oracle(oracle), 'oracle')
    cases.same_bits(got, parent(hip_dev_backend, 'flagless'), 'C = 1')


@pytest.mark.parametrize('n', [1483, 33291])
def test_model_with_flags_product(hip_backend, hip_dev_backend, oracle, n):
    cases.check_model(cases.run_model(hip_backend, DEV, n), n, cases.model_expected(oracle, n), False, parent(hip_dev_backend, 'model', n))


@pytest.mark.parametrize('n', [1483, 33291])
@pytest.mark.parametrize('c', [1, 2, 16, 32])
def test_model_with_flags_dev_option(hip_dev_backend, oracle, n, c):
    cases.check_model(cases.run_model(hip_dev_backend, DEV, n, c), n, cases.model_expected(oracle, n), False, parent(hip_dev_backend, 'model', n))


def test_all_quiet_launch_changes_no_byte(hip_backend, hip_dev_backend):
    cases.check_all_quiet(hip_backend, DEV)
    for c in (1, 2, 16, 32):
        cases.check_all_quiet(hip_dev_backend, DEV, c)


def test_span_option_range(hip_dev_backend):
    cases.check_option_range(hip_dev_backend)
