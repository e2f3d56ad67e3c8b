"""Bilateral-grid colour correction on the CPU simulation of the product library (the unmodified .hip sources): fgs_bilagrid_slice, its backward pass, the
total-variation kernel, the public operators and the harness module. Definitions, reference, cases and bars: tests/bilagrid_cases.py. The same comparisons
run on the MI355X in tests/test_gpu_bilagrid.py."""
import numpy as np
import pytest
import torch

import bilagrid_cases as cases
import helpers


@pytest.fixture(scope='module')
def be():
    return helpers.sim_backend(product=True)


@pytest.fixture
def operators_on_sim(be, monkeypatch):
    """The public operators, the optimizer and the harness (all unmodified) running on the simulation backend with CPU tensors."""
    import FasterGSCudaBackend as B
    import FasterGSCudaBackend.adam as A
    import FasterGSCudaBackend.bilagrid as G
    import FasterGSCudaBackend.rasterization as R
    import harness.loss as L
    for module in (R, A, G, L):
        monkeypatch.setattr(module, 'default_backend', lambda: be)
    for module in (R, G):
        monkeypatch.setattr(module, '_require_gpu', lambda t: None)
    return B


@pytest.mark.parametrize('name', cases.CPU_CASES)
def test_restated_definition_equals_grid_sample(name):
    """First of all: the trilinear restatement the kernels implement (corner indices clamped, an extent-1 axis on its only plane, no guide gradient where it
    is clamped), evaluated in fp64 numpy, equals the grid_sample reference in values and gradients to 1e-12."""
    c, ref = cases.case(name), cases.reference(name)
    C, G, gO = (c[k].numpy().astype(np.float64) for k in ('image', 'grid', 'gO'))
    (gw, gh, gl), (w, h) = c['extents'], c['size']
    u = (np.arange(w) + 0.5) / w * (gw - 1)
    v = (np.arange(h) + 0.5) / h * (gh - 1)
    raw = cases.guide64(C)
    z = np.clip(raw, 0, 1) * (gl - 1)
    def axis(t, n):
        i0 = np.minimum(np.floor(t).astype(int), n - 1)
        return i0, np.minimum(i0 + 1, n - 1), t - i0
    (x0, x1, fx), (y0, y1, fy), (z0, z1, fz) = axis(u, gw), axis(v, gh), axis(z, gl)
    X0, X1, FX = (np.broadcast_to(a[None, :], (h, w)) for a in (x0, x1, fx))
    Y0, Y1, FY = (np.broadcast_to(a[:, None], (h, w)) for a in (y0, y1, fy))
    M, dM, gG = np.zeros((12, h, w)), np.zeros((12, h, w)), np.zeros_like(G)
    val = np.stack([gO[i] * (C[j] if j < 3 else 1.0) for i in range(3) for j in range(4)])
    for zi, wz, dz in ((z0, 1 - fz, -1.0), (z1, fz, 1.0)):
        for yi, wy in ((Y0, 1 - FY), (Y1, FY)):
            for xi, wx in ((X0, 1 - FX), (X1, FX)):
                M += wz * wy * wx * G[:, zi, yi, xi]
                dM += dz * wy * wx * G[:, zi, yi, xi]
                for ch in range(12):
                    np.add.at(gG[ch], (zi, yi, xi), wz * wy * wx * val[ch])
    M4 = M.reshape(3, 4, h, w)
    out = (M4[:, :3] * C[None]).sum(1) + M4[:, 3]
    inside = (raw > 0) & (raw < 1)
    through = (dM * val).sum(0) * (gl - 1) * inside
    gC = np.stack([(M4[:, j] * gO).sum(0) + cases.LUMA[j] * through for j in range(3)])
    for got, k in ((out, 'out'), (gC, 'grad_image'), (gG, 'grad_grid')):
        assert helpers.rel_inf(got, ref[k]) < 1e-12, (name, k)
    assert 0.0 < c['clamped'] < 0.15


@pytest.mark.parametrize('name', cases.CPU_CASES)
def test_slice_and_gradients_match_the_fp64_reference(be, name):
    """1. out, grad_image, grad_grid at rel_inf < 1e-4; `fine` runs the global-memory path, the others the LDS-staged one."""
    cases.check_parity(be, name)


@pytest.mark.parametrize('name', ['fine', 'coarse'])
def test_identity_grid_is_the_identity(be, name):
    cases.check_identity(be, name)


@pytest.mark.parametrize('name', cases.CPU_CASES)
def test_a_gradient_that_is_not_asked_for_changes_nothing(be, name):
    """3. NULL grad_grid / grad_image: the other one bit-identical to the full call."""
    cases.check_null_gradients(be, name)


@pytest.mark.parametrize('name', ['fine', 'coarse'])
def test_stale_scratch_is_harmless(be, name):
    cases.check_stale_scratch(be, name)


def test_row_alignment_paths_agree(be):
    """The float4 rows (width % 4 == 0, 16-byte aligned tensors) and the scalar rows with a tail give the same numbers: `coarse` again from tensors that
    start 4 bytes past a 16-byte boundary."""
    c = cases.case('coarse')
    def odd(t):
        base = torch.empty(t.numel() + 8, dtype=t.dtype)
        shift = (1 - base.data_ptr() // 4) % 4
        o = base[shift:shift + t.numel()].view(t.shape)
        o.copy_(t)
        assert o.data_ptr() % 16 == 4
        return o
    aligned = cases.run(be, c)
    shifted = cases.run(be, dict(c, image=odd(c['image']), gO=odd(c['gO'])))
    for k in ('out', 'grad_image', 'grad_grid'):
        assert np.array_equal(aligned[k], shifted[k]), k


def test_total_variation(be):
    cases.check_tv(be)


def test_refusals(be):
    cases.check_refusals(be)


def test_public_operators(be, operators_on_sim):
    cases.check_operators(operators_on_sim, be)


def test_public_names():
    import inspect
    import FasterGSCudaBackend as B
    from FasterGSCudaBackend import _C
    from harness.bilagrid import BilateralGrids
    from harness.trainer import render_image_corrected, training_iteration      # noqa: F401
    assert {'bilagrid_slice', 'bilagrid_tv_loss'} <= set(B.__all__) and not hasattr(_C, 'bilagrid_slice')
    sig = inspect.signature(training_iteration).parameters
    assert sig['bilagrid'].default is None and sig['view_index'].default is None and sig['tv_weight'].default == 10.0
    m = BilateralGrids(3, shape=(4, 3, 2), device='cpu')
    assert len(m.grids) == 3 and all(torch.equal(g, cases.identity_grid(4, 3, 2)) for g in m.grids)
    m.training_setup()
    assert m.optimizer.param_groups[0]['lr'] == 2e-3
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.bilagrid_slice(torch.zeros(3, 4, 4), m.grids[0])


def test_training_iteration_equals_the_step_composed_by_hand(be, operators_on_sim):
    cases.check_training_iteration(be)


def test_grids_learn_a_fixed_colour_transform(be, operators_on_sim):
    """8b at a size the simulation walks in seconds: 30 steps, 100 Gaussians at 52 x 39 (four pixel tiles, the last column and row partial)."""
    cases.check_training_run(steps=30, n=100, size=(52, 39))


def test_checkpoint_round_trip_with_grids(be, operators_on_sim, tmp_path):
    cases.check_checkpoint_round_trip(tmp_path)
