"""K13's span workgroups (csrc/adam.hip) on the CPU simulation of the kernel sources: the product flavour (C a constant) and the dev flavour at C = 2,
16 and 32 against the oracle's dense step and against the dev flavour at C = 1. Cases, shapes and bars: tests/adam_span_cases.py;
tests/test_gpu_adam_spans.py runs the same functions on the MI355X."""
import pytest

import adam_span_cases as cases

DEV = 'cpu'
_parent = {}


def parent(sim_backend, what, n=None):
    """(b), computed once: the dev flavour at C = 1."""
    if (what, n) not in _parent:
        _parent[(what, n)] = cases.run_flagless(sim_backend, DEV, 1) if what == 'flagless' else cases.run_model(sim_backend, DEV, n, 1)
    return _parent[(what, n)]


def test_the_cases_bite_for_every_span_length():
    cases.check_cases_bite()


def test_sim_flagless_groups_product(sim_product_backend, sim_backend, oracle):
    got = cases.run_flagless(sim_product_backend, DEV)
    cases.same_bits(got, cases.flagless_oracle(oracle), 'oracle')
    cases.same_bits(got, parent(sim_backend, 'flagless'), 'C = 1')


@pytest.mark.parametrize('c', [1, 2, 16, 32])
def test_sim_flagless_groups_dev_option(sim_backend, oracle, c):
    got = cases.run_flagless(sim_backend, DEV, c)
    cases.same_bits(got, cases.flagless_oracle(oracle), 'oracle')
    cases.same_bits(got, parent(sim_backend, 'flagless'), 'C = 1')


@pytest.mark.parametrize('n', [1483, 33291])
def test_sim_model_with_flags_product(sim_product_backend, sim_backend, oracle, n):
    cases.check_model(cases.run_model(sim_product_backend, DEV, n), n, cases.model_expected(oracle, n), True, parent(sim_backend, 'model', n))


@pytest.mark.parametrize('n', [1483, 33291])
@pytest.mark.parametrize('c', [1, 2, 16, 32])
def test_sim_model_with_flags_dev_option(sim_backend, oracle, n, c):
    cases.check_model(cases.run_model(sim_backend, DEV, n, c), n, cases.model_expected(oracle, n), True, parent(sim_backend, 'model', n))


def test_sim_all_quiet_launch_changes_no_byte(sim_product_backend, sim_backend):
    cases.check_all_quiet(sim_product_backend, DEV)
    for c in (1, 2, 16, 32):
        cases.check_all_quiet(sim_backend, DEV, c)


def test_sim_span_option_range(sim_backend):
    cases.check_option_range(sim_backend)
