"""GPU: the HIP library against what the reference's own kernels computed -- the committed fixtures tests/golden/ref_kernels_*.npz (written in the
build container by tests/golden/make_ref_kernel_golden.py from the reference run on the CPU; arithmetic "as written", not as nvcc contracts it).
Counts, n_touched, instance keys and primitives and ranges exact; image, gradients, densification_info and pruning scores within 1e-4 of the tensor's
maximum, on the two partial-tile fixtures outside helpers.flip_masks. Four small scenes; reads tests/golden/ and builds the oracle (for the masks),
nothing else."""
import pytest

import ref_pin_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', cases.FIXTURES)
def test_hip_kernels_meet_the_reference_kernels(hip_backend, oracle, name):
    cases.check_backend_against_fixture(hip_backend, oracle, name, 'cuda', on_hardware=True)
