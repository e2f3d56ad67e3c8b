"""fgs_blend_features / fgs_backward_features and the public diff_rasterize_features on the MI355X: the comparisons of tests/test_feature_render.py
against the same fp64 reference (tests/feature_cases.py: definitions, upstream gradients, bars), autograd through the public operator, and a short
feature-fitting run of the harness."""
import numpy as np
import pytest
import torch

import aux_grad_cases as aux
import feature_cases as cases
import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name,n_channels', cases.PARITY)
def test_map_image_and_gradients_match_the_fp64_reference_on_device(hip_backend, name, n_channels):
    """1. As on the simulation; the image is held at MAP_TOL against plain `forward` (equal-depth compaction order is the only licence)."""
    cases.check_against_reference(hip_backend, name, n_channels, device=DEV, exact_image=False)


def test_identities_on_device(hip_backend):
    cases.check_identities(hip_backend, DEV)


def test_workaround_parity_on_device(hip_backend):
    cases.check_workaround_parity(hip_backend, DEV)


def test_detached_geometry_no_feature_gradient_and_retained_buffers_on_device(hip_backend):
    cases.check_detached_and_retained(hip_backend, DEV)


def test_refusals_and_no_gaussians_on_device(hip_backend):
    cases.check_errors_and_empty(hip_backend, DEV)


def test_autograd_through_diff_rasterize_features(hip_backend):
    """5. The public operator: outputs and gradients equal to the backend's; a non-contiguous gF; features that do not require grad; an unused map is
    the plain pass; an unused image; detach_geometry; torch.no_grad()."""
    import FasterGSCudaBackend as B
    cases.check_operator(B, hip_backend, 'hot', DEV)


def test_feature_fitting_reduces_the_feature_loss(hip_backend):
    """s0 at its own size: 20 Adam steps on 8 feature channels against random target channels, geometry detached -- the feature loss falls."""
    from harness import trainer as T
    from harness.scenes import make_s0
    dev = torch.device(DEV)
    params, view = make_s0(n=1000)
    view = view.to(dev)
    g = T.Gaussians(params, dev)
    gen = torch.Generator().manual_seed(9)
    target = torch.randn((8, view.height, view.width), generator=gen).to(dev)
    feats = torch.zeros((1000, 8), device=dev, requires_grad=True)
    opt = torch.optim.Adam([feats], lr=0.05)
    losses = []
    for _ in range(20):
        _, fmap = T.render_image_training_features(g, view, False, view.background_color, feats, detach_geometry=True)
        loss = ((fmap - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print('feature loss', losses[0], '->', losses[-1])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
