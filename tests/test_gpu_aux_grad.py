"""fgs_forward_aux / fgs_backward_aux and the public diff_rasterize_aux on the MI355X: the comparisons of tests/test_aux_grad.py against the same fp64
reference (tests/aux_grad_cases.py: definitions, upstream gradients, bars), autograd through the public operator, and a short depth-supervised
training run of the harness."""
import numpy as np
import pytest
import torch

import aux_grad_cases as cases
import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name', list(cases.CASES))
def test_maps_image_and_gradients_match_the_fp64_reference_on_device(hip_backend, name):
    """Forward maps at the aux render's 1e-4 bar, the image at diff_rasterize's (1e-4: equal-depth compaction order is the only licence), each of the six
    gradient tensors at rel_inf < 1e-4 against fp64 -- the plain RGB path's figure on the same scene is printed beside it."""
    cases.check_against_reference(hip_backend, name, device=DEV, exact_image=False)


def _leaves(c):
    return [c['params'][k].to(DEV).requires_grad_(True) for k in helpers.NAMES]


def test_autograd_through_diff_rasterize_aux(hip_backend):
    """The public operator: outputs, gradients equal to the backend's, (a) unused maps = diff_rasterize's gradients, (d) a second backward over the
    retained graph equals the first, (c) a depth-only loss leaves the SH gradients exactly zero."""
    import FasterGSCudaBackend as B
    c = cases.case('hot')
    RS = cases.settings_of(c, DEV)
    gC, gA, gD = (torch.as_tensor(c[k]).to(DEV) for k in ('gC', 'gA', 'gD'))
    direct = cases.run(hip_backend, c, c['gC'], c['gA'], c['gD'], DEV)

    leaves = _leaves(c)
    image, alpha, depth = B.diff_rasterize_aux(*leaves, torch.empty(0), RS)
    assert image.shape == (3, c['view'].height, c['view'].width) and alpha.shape == depth.shape == image.shape[1:]
    loss = (image * gC).sum() + (alpha * gA).sum() + (depth * gD).sum()
    first = torch.autograd.grad(loss, leaves, retain_graph=True)
    second = torch.autograd.grad(loss, leaves)
    for k, g1, g2 in zip(helpers.GRAD_KEYS, first, second):
        assert helpers.rel_inf(g1.cpu().numpy(), direct[k]) < 1e-5, k             # two runs differ by the order of K11's atomics only
        assert helpers.rel_inf(g2.cpu().numpy(), g1.cpu().numpy()) < 1e-5, k

    # a non-contiguous incoming gradient (a transposed view) is made contiguous
    leaves = _leaves(c)
    image, alpha, depth = B.diff_rasterize_aux(*leaves, torch.empty(0), RS)
    gD_t = gD.t().contiguous().t()
    assert not gD_t.is_contiguous()
    strided = torch.autograd.grad((image * gC).sum() + (alpha * gA).sum() + (depth * gD_t).sum(), leaves)
    for k, g in zip(helpers.GRAD_KEYS, strided):
        assert helpers.rel_inf(g.cpu().numpy(), direct[k]) < 1e-5, k

    # (a) the maps are not part of the loss: their gradients arrive as None and the pass is the plain one
    leaves = _leaves(c)
    image, _, _ = B.diff_rasterize_aux(*leaves, torch.empty(0), RS)
    unused = torch.autograd.grad((image * gC).sum(), leaves)
    leaves = _leaves(c)
    plain = torch.autograd.grad((B.diff_rasterize(*leaves, torch.empty(0), RS) * gC).sum(), leaves)
    for k, g, p in zip(helpers.GRAD_KEYS, unused, plain):
        assert helpers.rel_inf(g.cpu().numpy(), p.cpu().numpy()) < 1e-6, k

    # (c) depth only; and a single requested map
    leaves = _leaves(c)
    image, alpha, depth = B.diff_rasterize_aux(*leaves, torch.empty(0), RS, alpha=False, depth=True)
    assert alpha is None and torch.equal(depth.detach().cpu(), torch.as_tensor(direct['depth']))
    only_depth = torch.autograd.grad((depth * gD).sum(), leaves)
    assert not only_depth[4].any() and not only_depth[5].any() and float(only_depth[0].abs().max()) > 0


def test_second_backward_and_plain_backward_on_device(hip_backend):
    """(d) through the backend on retained buffers, (e) the plain fgs_backward on buffers of fgs_forward_aux."""
    c = cases.case('stacked')
    first = cases.run(hip_backend, c, c['gC'], c['gA'], c['gD'], DEV)
    second = cases.run(hip_backend, c, c['gC'], c['gA'], c['gD'], DEV, res=first['res'])
    plain_on_aux = cases.run(hip_backend, c, c['gC'], None, None, DEV, res=first['res'])
    plain = cases.run_plain(hip_backend, c, c['gC'], DEV)
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(second[k], first[k]) < 1e-5, k
        assert helpers.rel_inf(plain_on_aux[k], plain[k]) < 1e-5, k


def test_errors_and_no_gaussians_on_device(hip_backend):
    """(f) a depth gradient on plain-forward buffers, (g) n = 0."""
    c = cases.case('partial_tiles')
    RS = cases.settings_of(c, DEV)
    p = [c['params'][k].to(DEV) for k in helpers.NAMES]
    plain = hip_backend.forward(*p, RS)
    gi, gm = torch.as_tensor(c['gC']).to(DEV), torch.as_tensor(c['gD']).to(DEV)
    with pytest.raises(RuntimeError, match='depth checkpoints'):
        hip_backend.backward_aux(None, gi, None, gm, plain.image, gm, p[0], p[1], p[2], p[3], p[5], plain.buffers, RS, plain.state)
    empty = [t[:0].contiguous() for t in p]
    res = hip_backend.forward_aux(*empty, RS)
    assert not res.alpha.any() and not res.depth.any() and torch.equal(res.image.cpu(), torch.zeros(3, c['view'].height, c['view'].width))


def test_depth_supervision_reduces_the_depth_error(hip_backend):
    """s0 at its own size: 30 plain training steps with depth_weight > 0 against the depth rendered from the generating parameters, starting from
    perturbed means -- the depth L1 at the end is below its value at the start."""
    from harness import trainer as T
    from harness.scenes import make_s0
    dev = torch.device(DEV)
    params, view = make_s0(n=1000)
    view = view.to(dev)
    truth = T.Gaussians(params, dev)
    with torch.no_grad():
        target, a, d = T.render_image_training_aux(truth, view, False, view.background_color)
    valid = a > 0.5
    depth_target = torch.where(valid, d / a.clamp_min(1e-8), torch.zeros_like(d))
    gen = torch.Generator().manual_seed(5)
    start = {k: v.clone() for k, v in params.items()}
    start['means'] = start['means'] + 0.05 * torch.randn(start['means'].shape, generator=gen)
    g = T.Gaussians(start, dev)
    g.training_setup(training_cameras_extent=4.0)

    def depth_error():
        with torch.no_grad():
            _, a, d = T.render_image_training_aux(g, view, False, view.background_color)
        return float(T.depth_l1_loss(a, d, depth_target, valid))

    before = depth_error()
    losses = [float(T.training_iteration(g, view, target, it, depth_target=depth_target, depth_weight=1.0, depth_valid=valid)) for it in range(30)]
    after = depth_error()
    print('depth L1', before, '->', after)
    assert all(np.isfinite(losses)) and after < before, (before, after)
