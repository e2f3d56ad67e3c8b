"""K10's tile -> workgroup mappings on the MI355X (libfgs_hip_dev.so), and the product library's one mapping against the dev library's default:
definitions, sizes and bars in tests/k10_mapping_cases.py. Each case is five passes over 300 Gaussians."""
import functools

import pytest

import k10_mapping_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@functools.lru_cache(maxsize=None)
def _default(be, size):
    return cases.run_all_mapped(be, cases.DEFAULT, *size, device=DEV)       # computed once per size, shared by the cases below: read-only


@pytest.mark.parametrize('mapping', cases.MAPPINGS)
@pytest.mark.parametrize('size', cases.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_mapping_blends_what_the_default_blends_on_device(hip_dev_backend, size, mapping):
    got = cases.run_all_mapped(hip_dev_backend, mapping, *size, device=DEV)
    cases.check_same(got, _default(hip_dev_backend, size), DEV, (size, mapping))


@pytest.mark.parametrize('size', cases.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_product_library_blends_what_the_dev_default_blends_on_device(hip_backend, hip_dev_backend, size):
    assert not hasattr(hip_backend.lib, 'fgs_debug_set_option')
    cases.check_same(cases.run_all(hip_backend, *size, device=DEV), _default(hip_dev_backend, size), DEV, (size, 'product'))
