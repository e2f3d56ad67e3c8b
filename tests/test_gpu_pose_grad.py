"""fgs_backward_pose, Backend.backward_pose, diff_rasterize_pose and harness.pose.refine_pose on the MI355X: the comparisons of tests/test_pose_grad.py
against the same fp64 reference (tests/pose_grad_cases.py: definitions, upstream gradients, bars). Where the simulation compares bit for bit the device
holds rel_inf < 1e-5: two runs differ by the order of K11's float atomics, nothing else -- the pose reduction itself has none."""
import pytest

import pose_grad_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name', list(cases.CASES))
def test_camera_gradients_match_the_fp64_reference_on_device(hip_backend, name):
    """Check 1: grad_w2c (12 entries) and grad_cam_position (3), each at rel_inf < 1e-4 against fp64, with gA = gD = 0 and with all three upstream gradients."""
    cases.check_camera_gradients(hip_backend, name, device=DEV)


@pytest.mark.parametrize('name', ['partial_tiles', 'ragged'])
def test_parameter_gradients_are_unchanged_on_device(hip_backend, name):
    """Check 2: the six gradients and both flag arrays of fgs_backward_pose against fgs_backward_reached on the same buffers; NULL camera outputs."""
    cases.check_parameter_gradients_unchanged(hip_backend, name, device=DEV, exact=False)


def test_recycled_path_delivers_its_partials_on_device(hip_backend):
    """Check 3: valid prior_blocks, two blocks take K12's early return."""
    cases.check_recycled_path(hip_backend, device=DEV, exact=False)


def test_result_does_not_depend_on_the_scratch_on_device(hip_backend):
    """Check 4: scratch full of 0xFF bytes; then zero upstream gradients on the same scratch give 15 values equal to 0.0f."""
    cases.check_scratch_independence(hip_backend, device=DEV, exact=False)


def test_degenerate_inputs_on_device(hip_backend):
    """Check 5: n = 0, one SH basis, a depth-only loss."""
    cases.check_degenerate_inputs(hip_backend, device=DEV)


def test_translation_identity_over_many_partials_on_device(hip_backend):
    """Check 6: 60 001 Gaussians, 938 wave partials in 235 workgroups, no dense reference: grad_w2c[:,3] == W sum_i grad_means[i] within the rounding bound."""
    cases.check_translation_identity(hip_backend, device=DEV)


def test_public_operator_on_device(hip_backend):
    """Check 7: diff_rasterize_pose through autograd."""
    import FasterGSCudaBackend as B
    cases.check_public_operator(B, hip_backend, DEV)


def test_it_refines_a_pose_on_device(hip_backend):
    """Check 8: 30 Adam steps on a PoseDelta from a degree and 1 % off: rotation error, translation error and image L1 all end below where they started."""
    cases.check_refinement(DEV, steps=30)
