"""TSDF fusion and mesh extraction on the CPU simulation of the product library (the unmodified .hip sources): fgs_tsdf_integrate, fgs_tsdf_mesh_count /
_emit, the public operators and harness/mesh.py. Definitions, fp64 models, cases and bars: tests/tsdf_cases.py. The same checks run on the MI355X in
tests/test_gpu_tsdf.py; the refusals of the built library are in tests/test_tsdf_abi.py."""
import numpy as np
import pytest
import torch

import helpers
import tsdf_cases as cases


@pytest.fixture(scope='module')
def be():
    return helpers.sim_backend(product=True)


@pytest.fixture
def operators_on_sim(be, monkeypatch):
    """The public operators and the harness (all unmodified) running on the simulation backend with CPU tensors."""
    import FasterGSCudaBackend as B
    import FasterGSCudaBackend.rasterization as R
    import FasterGSCudaBackend.tsdf as T
    for module in (R, T):
        monkeypatch.setattr(module, 'default_backend', lambda: be)
        monkeypatch.setattr(module, '_require_gpu', lambda t: None)
    return B


def test_models_agree_with_themselves():
    """Before anything runs: the flagged share of the integration case is below its bar on the model alone, and the restated extraction gives a closed,
    outward-oriented sphere (the restatement decides orientation on the geometry, not by the kernel's rule)."""
    _, _, touched, flagged = cases.integration_reference()
    assert flagged.mean() < cases.FLAGGED_BAR and touched.any() and not touched.all()
    ref = cases.mesh_reference('sphere')
    closed, n_edges, boundary = cases.edge_report(ref['faces'])
    assert closed and len(ref['vertices']) - n_edges + len(ref['faces']) == 2 and cases.signed_volume(ref['vertices'], ref['faces']) > 0
    assert len(cases.TETS) == 6 and len({frozenset(t) for t in cases.TETS}) == 6


def test_integration_matches_the_fp64_model(be):
    cases.check_integration_against_model(be)


def test_batched_views_equal_single_view_calls(be):
    cases.check_batched_equals_single(be)


def test_untouched_points_and_the_weight_cap(be):
    cases.check_untouched_and_cap(be)


def test_pixel_convention_is_the_rasterizers(be):
    cases.check_pixel_convention(be)


def test_sphere(be):
    cases.check_sphere(be)


def test_torus_and_two_spheres(be):
    cases.check_genus(be)


def test_lattice_valued_field_keeps_its_degenerate_triangles(be):
    cases.check_lattice_valued(be)


def test_half_valid_volume(be):
    cases.check_half_valid(be)


def test_edge_cases(be):
    cases.check_edge_cases(be)


def test_refusals_on_the_simulation(be):
    cases.refusal_cases(be.lib)


def test_harness_and_file_round_trip(be, operators_on_sim, tmp_path):
    cases.check_harness_round_trip(be, tmp_path)


def test_public_names_and_cpu_refusal():
    import FasterGSCudaBackend as B
    from FasterGSCudaBackend import _C
    from harness.mesh import TSDFVolume, extract_mesh, load_mesh_ply, save_mesh_ply      # noqa: F401
    assert {'tsdf_integrate', 'tsdf_extract_mesh'} <= set(B.__all__) and not hasattr(_C, 'tsdf_integrate')
    vol = TSDFVolume((0.0, 0.0, 0.0), 0.1, (4, 3, 2), 0.3, device='cpu')
    assert vol.tsdf_weight.shape == (2, 3, 4, 2) and vol.color.shape == (3, 2, 3, 4) and not vol.tsdf_weight.any()
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.tsdf_extract_mesh(vol.tsdf_weight, vol.color, vol.origin, vol.voxel_size)
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.tsdf_integrate(vol.tsdf_weight, None, vol.origin, 0.1, 0.3, [None], [torch.zeros(2, 2)])


def test_end_to_end_sphere_of_disks(be, operators_on_sim):
    """11. measured on the simulation: see tsdf_cases.END_TO_END_MEASURED."""
    cases.check_end_to_end()
