"""fgs_blend_distortion / fgs_backward_distortion and the public diff_rasterize_distortion on the MI355X: the comparisons of tests/test_distortion.py
against the same fp64 reference (tests/distortion_cases.py: definitions, upstream gradients, bars), autograd through the public operator, and a short
run that minimises the distortion alone."""
import numpy as np
import pytest
import torch

import aux_grad_cases as aux
import distortion_cases as cases
import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name,mode', cases.PARITY)
def test_map_image_and_gradients_match_the_fp64_reference_on_device(hip_backend, name, mode):
    """1. As on the simulation; the image is held at MAP_TOL against plain `forward` (equal-depth compaction order is the only licence)."""
    cases.check_against_reference(hip_backend, name, mode, device=DEV, exact_image=False)


@pytest.mark.parametrize('name,mode', cases.ALONE)
def test_gradients_of_the_distortion_term_alone_on_device(hip_backend, name, mode):
    cases.check_term_alone(hip_backend, name, mode, DEV)


def test_state_planes_on_device(hip_backend):
    cases.check_state(hip_backend, DEV)


def test_boundary_cases_on_device(hip_backend):
    cases.check_boundaries(hip_backend, DEV)


def test_refusals_and_no_gaussians_on_device(hip_backend):
    cases.check_errors_and_empty(hip_backend, DEV)


def test_abi_refusals_on_device(hip_backend):
    _lib, _ = helpers.backend_modules()
    cases.check_abi_refusals(hip_backend.lib, _lib)


def test_autograd_through_diff_rasterize_distortion(hip_backend):
    """5. The public operator: outputs and gradients equal to the backend's in both modes; a non-contiguous gX; an unused map is the plain pass; an
    unused image; torch.no_grad()."""
    import FasterGSCudaBackend as B
    cases.check_operator(B, hip_backend, 'hot', DEV)


def test_minimising_the_distortion_alone_lowers_it(hip_backend):
    """6. `stacked`: 30 Adam steps on distortion.mean() alone, over means, scales, rotations and opacities."""
    import FasterGSCudaBackend as B
    c = aux.case('stacked')
    RS = aux.settings_of(c, DEV)
    leaves = [c['params'][k].to(DEV).clone().requires_grad_(True) for k in helpers.NAMES]
    opt = torch.optim.Adam(leaves[:4], lr=2e-3)
    losses = []
    for _ in range(30):
        _, dmap = B.diff_rasterize_distortion(*leaves, torch.empty(0), RS)
        loss = dmap.mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print('distortion', losses[0], '->', losses[-1])
    assert all(np.isfinite(losses)) and losses[0] > 0 and losses[-1] < losses[0], losses


def test_training_iteration_with_the_distortion_term(hip_backend):
    """The harness: distortion_weight adds weight * distortion.mean() to the loss of the step and the step still trains; the default is the plain
    iteration; depth supervision and absgrad in the same render are refused."""
    from harness import trainer as T
    from harness.scenes import make_s0
    dev = torch.device(DEV)
    params, view = make_s0(n=1000)
    view = view.to(dev)
    truth = T.Gaussians(params, dev)
    target = T.render_image_benchmark(truth, view).clone()
    with torch.no_grad():
        _, dmap = T.render_image_training_distortion(truth, view, False, view.background_color)
    mean = float(dmap.mean())
    assert dmap.shape == (view.height, view.width) and mean > 0

    def first_loss(**kw):
        g = T.Gaussians({k: v.clone() for k, v in params.items()}, dev)
        g.training_setup(training_cameras_extent=4.0)
        losses = [float(T.training_iteration(g, view, target, it, **kw)) for it in range(3)]
        assert all(np.isfinite(losses))
        return losses[0], g
    plain, _ = first_loss()
    default, _ = first_loss(distortion_weight=0.0)
    with_term, g = first_loss(distortion_weight=10.0)
    assert default == plain
    assert abs((with_term - plain) - 10.0 * mean) <= 1e-4 * (abs(plain) + 10.0 * mean), (with_term, plain, mean)
    assert g.densification_info[0].max() > 0                       # the statistic of the step is still updated
    with pytest.raises(ValueError, match='does not combine'):
        T.training_iteration(g, view, target, 3, distortion_weight=1.0, absgrad=True)
    with pytest.raises(ValueError, match='does not combine'):
        T.training_iteration(g, view, target, 3, distortion_weight=1.0, depth_target=target[0], depth_weight=1.0)
