"""TSDF fusion and mesh extraction on the MI355X: the checks of tests/test_tsdf.py against the same fp64 models (tests/tsdf_cases.py: definitions, cases,
bars), through libfgs_hip.so, the public operators and harness/mesh.py."""
import pytest

import tsdf_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_integration_matches_the_fp64_model_on_device(hip_backend):
    cases.check_integration_against_model(hip_backend, DEV)


def test_batched_views_equal_single_view_calls_on_device(hip_backend):
    cases.check_batched_equals_single(hip_backend, DEV)


def test_untouched_points_and_the_weight_cap_on_device(hip_backend):
    cases.check_untouched_and_cap(hip_backend, DEV)


def test_pixel_convention_is_the_rasterizers_on_device(hip_backend):
    cases.check_pixel_convention(hip_backend, DEV)


def test_sphere_on_device(hip_backend):
    cases.check_sphere(hip_backend, DEV)


def test_torus_and_two_spheres_on_device(hip_backend):
    cases.check_genus(hip_backend, DEV)


def test_lattice_valued_field_keeps_its_degenerate_triangles_on_device(hip_backend):
    cases.check_lattice_valued(hip_backend, DEV)


def test_half_valid_volume_on_device(hip_backend):
    cases.check_half_valid(hip_backend, DEV)


def test_edge_cases_on_device(hip_backend):
    cases.check_edge_cases(hip_backend, DEV)


def test_harness_and_file_round_trip_on_device(hip_backend, tmp_path):
    cases.check_harness_round_trip(hip_backend, tmp_path, DEV)


def test_public_operators_refuse_cpu_tensors_on_device(hip_backend):
    import torch
    import FasterGSCudaBackend as B
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.tsdf_extract_mesh(torch.zeros(2, 2, 2, 2), None, (0.0, 0.0, 0.0), 0.1)


def test_end_to_end_sphere_of_disks_on_device(hip_backend):
    cases.check_end_to_end(DEV)
