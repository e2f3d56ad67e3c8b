"""CPU test of the TSDF entries' argument checks in the BUILT library (libfgs_hip.so), beside tests/test_abi.py: every refusal comes back as an
fgs_status with a text before anything touches a GPU. The cases: tests/tsdf_cases.py::refusal_cases."""
import subprocess
from pathlib import Path

import pytest

import helpers
import tsdf_cases as cases

REPO = Path(__file__).resolve().parent.parent
LIB = REPO / 'faster-gaussian-splatting_amd' / 'libfgs_hip.so'


@pytest.fixture(scope='module')
def hip_lib():
    if not LIB.exists():
        subprocess.run(['make', '-C', str(LIB.parent / 'csrc'), '-j8'], check=True)
    _lib, _ = helpers.backend_modules()
    return _lib.bind(LIB)


def test_tsdf_refusals_without_gpu(hip_lib):
    out = dict((what, text) for what, _, text in cases.refusal_cases(hip_lib))
    assert 'at least 2' in out['extent 1'] and '2^28' in out['2^28 + 2 points'] and 'views' in out['V = 0'] and 'views' in out['V = 9']
    assert 'NULL' in out['emit NULL vertices'] and 'NULL' in out['emit NULL faces']
