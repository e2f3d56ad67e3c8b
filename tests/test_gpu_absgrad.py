"""fgs_backward_absgrad, Backend.backward_absgrad and the public diff_rasterize_absgrad on the MI355X: the comparisons of tests/test_absgrad.py against the
same fp64 reference (tests/absgrad_cases.py: definitions, cases, bars), autograd through the public operator, and a short training run of the harness
whose density control reads the absolute statistic."""
import numpy as np
import pytest
import torch

import absgrad_cases as cases
import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('maps', [False, True], ids=['rgb', 'maps'])
@pytest.mark.parametrize('name', cases.CASE_NAMES)
def test_statistic_matches_the_fp64_reference_on_device(hip_backend, name, maps):
    """1. Row 1 at rel_inf < 1e-4 against fp64, row 0 exactly the visibility: ABS without DEPTH and ABS with DEPTH."""
    cases.check_parity(hip_backend, name, maps, device=DEV)


@pytest.mark.parametrize('maps', [False, True], ids=['rgb', 'maps'])
@pytest.mark.parametrize('name', ['partial_tiles', 'hot'])
def test_nothing_else_moves_on_device(hip_backend, name, maps):
    """2. Gradients and densification_info within 1e-5 of backward_aux / backward on the same forward buffers (two runs differ by the order of K11's
    atomics only); the block flags are equal."""
    cases.check_nothing_else_moves(hip_backend, name, maps, device=DEV, exact=False)


def test_identities_on_device(hip_backend):
    """3. abs >= signed for every Gaussian of every case; `lone`."""
    cases.check_identities(hip_backend, device=DEV)


def test_accumulation_and_stale_scratch_on_device(hip_backend):
    """4. Retained buffers double both rows, a non-zero tensor is added to; scratch that arrives as 0xFF bytes gives the same statistic."""
    cases.check_accumulation(hip_backend, device=DEV, tol=1e-5)
    clean = cases.run_once(hip_backend, 'hot', True, DEV)
    dirty = cases.run(helpers.poisoned(hip_backend), cases.case('hot'), True, DEV)
    for k in ('abs', 'dens') + helpers.GRAD_KEYS:
        assert helpers.rel_inf(dirty[k], clean[k]) < 1e-5, k


def test_refusals_and_no_gaussians_on_device(hip_backend):
    """5. The refusals through the backend on device tensors; n = 0 writes nothing."""
    c = cases.case('partial_tiles')
    RS = cases.settings_of(c, DEV)
    p = [c['params'][k].to(DEV) for k in helpers.NAMES]
    n = p[0].shape[0]
    gi = torch.as_tensor(c['gC']).to(DEV)
    info = torch.zeros(2, n, device=DEV)
    tail = lambda r: (r.image, None, p[0], p[1], p[2], p[3], p[5], r.buffers, RS, r.state)
    res = hip_backend.forward(*p, RS)
    with pytest.raises(RuntimeError, match='aliases densification_info'):
        hip_backend.backward_absgrad(info, info, gi, None, None, *tail(res))
    with pytest.raises(RuntimeError, match="fgs_forward_async's"):
        hip_backend.backward_absgrad(None, info, gi, None, None, *tail(hip_backend.forward(*p, RS, instance_capacity=1 << 20)))
    with pytest.raises(RuntimeError, match='sharded / record paths'):
        hip_backend.backward_absgrad(None, info, gi, None, None, *tail(res._replace(state=res.state[:3] + (res.state[3] | 8,))))
    assert not info.any()
    assert hip_backend.lib.fgs_abi_version() == 3
    empty = [t[:0].contiguous() for t in p]
    r0 = hip_backend.forward(*empty, RS)
    grads = hip_backend.backward_absgrad(None, torch.zeros(2, 0, device=DEV), torch.ones_like(r0.image), None, None, r0.image, None, empty[0], empty[1],
                                         empty[2], empty[3], empty[5], r0.buffers, RS, r0.state)
    assert all(g.shape[0] == 0 for g in grads)


def test_autograd_through_diff_rasterize_absgrad(hip_backend):
    """6. The public operator on the device."""
    import FasterGSCudaBackend as B
    cases.check_operator(B, hip_backend, device=DEV, tol=1e-5)


def test_training_with_the_absolute_statistic(hip_backend):
    """7. s0 with n = 1000 at its own size: 40 training_iteration(..., absgrad=True) steps under a compressed schedule with 'absgrad': True. The losses
    stay finite, density control ran on the absolute tensor, the model grew, and g.densification_info was never written."""
    from harness import densify as D
    from harness import trainer as T
    from harness.scenes import make_s0
    dev = torch.device(DEV)
    params, view = make_s0(n=1000)
    view = view.to(dev)
    truth = T.Gaussians(params, dev)
    with torch.no_grad():
        target = T.render_image_training(truth, view, False, view.background_color)
    gen = torch.Generator().manual_seed(5)
    start = {k: v.clone() for k, v in params.items()}
    start['means'] = start['means'] + 0.05 * torch.randn(start['means'].shape, generator=gen)
    g = T.Gaussians(start, dev)
    g.training_setup(training_cameras_extent=4.0)
    schedule = dict(D.GARDEN_SCHEDULE, densification_start=10, densification_interval=10, densification_end=35, opacity_reset_interval=1000,
                    morton_interval=20, morton_end=40, sh_interval=1000, absgrad=True)
    assert schedule['absgrad_threshold'] == 8e-4
    dgen = torch.Generator().manual_seed(6)
    losses, controls, seen = [], [], []
    for it in range(40):
        if it in (10, 20, 30):          # what density control is about to read
            seen.append((g.abs_densification_info.clone(), g.densification_info.clone()))
        stats = D.run_callbacks(g, it, schedule, dgen)
        if stats:
            controls.append(stats)
        losses.append(float(T.training_iteration(g, view, target, it, densification_end=schedule['densification_end'], absgrad=True)))
    print('absgrad training: losses', losses[0], '->', losses[-1], 'controls', controls)
    assert all(np.isfinite(losses))
    assert len(controls) == 3 and len(seen) == 3
    for info, signed in seen:
        assert float(info[0].max()) == 10.0 and float(info[1].max()) > 0          # ten passes accumulated the absolute statistic ...
        assert not signed.any()                                                      # ... and none touched the signed one
    assert sum(s['cloned'] + s['split'] for s in controls) > 0 and g.means.shape[0] > 1000
    assert g.densification_info is None or not g.densification_info.any()
