"""K10's tile -> workgroup mappings on the CPU simulation (dev flavour of the sources), and the product flavour's one mapping against it:
definitions, sizes and bars in tests/k10_mapping_cases.py."""
import functools

import pytest

import k10_mapping_cases as cases


@functools.lru_cache(maxsize=None)
def _default(be, size):
    return cases.run_all_mapped(be, cases.DEFAULT, *size)       # computed once per size, shared by the cases below: read-only


@pytest.mark.parametrize('mapping', cases.MAPPINGS)
@pytest.mark.parametrize('size', cases.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_mapping_blends_what_the_default_blends(sim_backend, size, mapping):
    got = cases.run_all_mapped(sim_backend, mapping, *size)
    cases.check_same(got, _default(sim_backend, size), 'cpu', (size, mapping))


@pytest.mark.parametrize('size', cases.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_product_flavour_blends_what_the_dev_default_blends(sim_product_backend, sim_backend, size):
    """The product flavour always passes the columns mapping (api.hip: bucket_scan_and_mapping) and has a scan-only K8+K9 kernel (binning.hip)."""
    assert not hasattr(sim_product_backend.lib, 'fgs_debug_set_option')
    cases.check_same(cases.run_all(sim_product_backend, *size), _default(sim_backend, size), 'cpu', (size, 'product'))
