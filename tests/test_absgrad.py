"""fgs_backward_absgrad on the CPU simulation of the product library (the unmodified .hip sources): the absolute-gradient densification statistic that
K11 sums beside the signed one. Definitions, reference, cases and bars: tests/absgrad_cases.py. The same comparisons run on the MI355X in
tests/test_gpu_absgrad.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import absgrad_cases as cases
import helpers


@pytest.fixture(scope='module')
def be():
    return helpers.sim_backend(product=True)


@pytest.fixture
def operator_on_sim(be, monkeypatch):
    """The public operators (FasterGSCudaBackend.rasterization, unmodified) running on the simulation backend with CPU tensors."""
    import FasterGSCudaBackend as B
    import FasterGSCudaBackend.rasterization as R
    monkeypatch.setattr(R, 'default_backend', lambda: be)
    monkeypatch.setattr(R, '_require_gpu', lambda t: None)
    return B


@pytest.mark.parametrize('name', cases.CASE_NAMES)
def test_reference_is_the_trusted_one(name):
    """First of all, for every case: the six gradients of the restated reference equal aux_autograd_reference's to 1e-12."""
    cases.check_reference_is_the_trusted_one(name)


def test_the_scenes_reach_every_path():
    """Reference side only: a hot Gaussian that is blended in `hot` (replicas and the fold), Gaussians that are visible yet unreached in `partial_tiles`
    (row 0 counts them, row 1 stays 0), `lone` on a pixel corner and inside the image."""
    hot = cases.case('hot')['f']
    sb = hot['screen_bounds'].astype(np.int64)
    tiles = ((sb[:, 1] + 15) // 16 - sb[:, 0] // 16) * ((sb[:, 3] + 11) // 12 - sb[:, 2] // 12)
    blended = np.zeros(hot['N'], bool)
    blended[hot['inst_prims']] = True
    assert ((tiles > cases.aux.HOT_FOOTPRINT) & blended).sum() >= 1
    ref = cases.reference('partial_tiles', True)
    assert ((cases.case('partial_tiles')['f']['n_touched'] > 0) & (ref['abs'] == 0)).sum() >= 10
    lone = cases.case('lone')
    assert lone['f']['mean2d'][0].tolist() == [16.0, 12.0] and lone['view'].width == 32 and lone['view'].height == 24
    assert float(lone['gC'][:, lone['keep']].min()) == float(lone['gC'].max()) > 0


@pytest.mark.parametrize('maps', [False, True], ids=['rgb', 'maps'])
@pytest.mark.parametrize('name', cases.CASE_NAMES)
def test_statistic_matches_the_fp64_reference(be, name, maps):
    """1. ABS without DEPTH (image gradient only) and ABS with DEPTH (gA, gD as well)."""
    cases.check_parity(be, name, maps)


@pytest.mark.parametrize('maps', [False, True], ids=['rgb', 'maps'])
@pytest.mark.parametrize('name', ['partial_tiles', 'hot'])
def test_nothing_else_moves(be, name, maps):
    """2. Bit-identical gradients, densification_info and block flags with and without the statistic."""
    cases.check_nothing_else_moves(be, name, maps, exact=True)


def test_identities(be):
    """3. abs >= signed everywhere; `lone`: signed / abs < 0.01 on the reference, and the library matches it."""
    cases.check_identities(be)


def test_accumulation_and_retained_buffers(be):
    """4. Two passes over retained buffers double both rows; a non-zero tensor is added to."""
    cases.check_accumulation(be)


def test_stale_scratch_memory(be):
    """4. Scratch and forward buffers that arrive as 0xFF bytes: the same statistic (acc_abs and its replicas are cleared by the pass itself)."""
    for name, maps in (('hot', True), ('partial_tiles', False)):
        clean, dirty = cases.run_once(be, name, maps), cases.run(helpers.poisoned(be), cases.case(name), maps)
        for k in ('abs', 'dens') + helpers.GRAD_KEYS:
            assert np.array_equal(dirty[k], clean[k]), (name, maps, k)


def test_two_kernel_form_of_k12():
    """The dev library's two-kernel K12: the statistic never enters K12, so it is the same."""
    dev = helpers.sim_backend()
    c = cases.case('partial_tiles')
    one = cases.run(dev, c, True)
    assert dev.lib.fgs_debug_set_option(3, 0) == 0
    try:
        two = cases.run(dev, c, True)
    finally:
        assert dev.lib.fgs_debug_set_option(3, 1) == 0
    assert np.array_equal(two['abs'], one['abs']) and np.array_equal(two['dens'], one['dens'])


def test_refusals_and_no_gaussians(be):
    """5. Every refusal raises with its text, through the backend and from the C entry by itself before any launch; n = 0 writes nothing."""
    _lib, _ = helpers.backend_modules()
    st = _lib.ForwardState()
    S = _lib.Settings(1, 1, 1, 16, 15, 128, 128, 1.0, 1.0, 0.0, 0.0, 0.2, 100.0, 0)
    libs = [be.lib] + ([_lib.bind(_lib.DEFAULT_LIBRARY)] if _lib.DEFAULT_LIBRARY.exists() else [])
    for lib in libs:
        call = lambda state, dens, info: lib.fgs_backward_absgrad(1, 1, None, None, None, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, dens, 1, 10, C.byref(S),
                                                                  C.byref(state), None, None, None, info, None)
        for bit, text in ((4, b'fgs_forward_async'), (8, b'record')):
            assert call(_lib.ForwardState(0, 0, 0, bit), None, 4096) == -1
            assert text in lib.fgs_last_error() and b'abs_densification_info' in lib.fgs_last_error()
        for dens in (4096, 4096 + 40, 4096 - 40):
            assert call(st, dens, 4096) == -1
            assert b'aliases densification_info' in lib.fgs_last_error()
        assert lib.fgs_abi_version() == 3
        assert lib.fgs_backward_absgrad_scratch_bytes(-1, 128, 128) == 0 and lib.fgs_backward_absgrad_scratch_bytes(10, 0, 128) == 0
        for n in (0, 1, 1000):
            assert lib.fgs_backward_absgrad_scratch_bytes(n, 128, 96) >= lib.fgs_backward_aux_scratch_bytes(n, 128, 96) + 8 * n
    assert {'fgs_backward_absgrad', 'fgs_backward_absgrad_scratch_bytes'} <= set(_lib.EXPORTED_SYMBOLS)

    c = cases.case('partial_tiles')
    RS = cases.settings_of(c)
    p = [c['params'][k] for k in helpers.NAMES]
    n = p[0].shape[0]
    gi = torch.as_tensor(c['gC'])
    info = torch.zeros(2, n)
    tail = lambda r: (r.image, None, p[0], p[1], p[2], p[3], p[5], r.buffers, RS, r.state)
    res = be.forward(*p, RS)
    with pytest.raises(RuntimeError, match='aliases densification_info'):
        be.backward_absgrad(info, info, gi, None, None, *tail(res))
    with pytest.raises(RuntimeError, match='abs_densification_info must be a contiguous float32'):
        be.backward_absgrad(None, torch.zeros(2, n + 1), gi, None, None, *tail(res))
    with pytest.raises(RuntimeError, match="fgs_forward_async's"):
        be.backward_absgrad(None, info, gi, None, None, *tail(be.forward(*p, RS, instance_capacity=1 << 20)))
    flagged = res._replace(state=res.state[:3] + (res.state[3] | 8,))
    with pytest.raises(RuntimeError, match='sharded / record paths'):
        be.backward_absgrad(None, info, gi, None, None, *tail(flagged))
    assert not info.any()
    # None / an empty tensor: backward_aux exactly
    for nothing in (None, torch.empty(0)):
        grads = be.backward_absgrad(None, nothing, gi, None, None, *tail(res))
        plain = be.backward(None, gi, res.image, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
        assert all(torch.equal(a, b) for a, b in zip(grads, plain))
    # n = 0
    empty = [t[:0].contiguous() for t in p]
    r0 = be.forward(*empty, RS)
    none = torch.zeros(2, 0)
    grads = helpers.poisoned(be).backward_absgrad(None, none, torch.ones_like(r0.image), None, None, r0.image, None, empty[0], empty[1], empty[2], empty[3],
                                                 empty[5], r0.buffers, RS, r0.state)
    assert all(g.shape[0] == 0 for g in grads)


def test_autograd_through_the_public_operator(be, operator_on_sim):
    """6. diff_rasterize_absgrad itself on the simulation: what tests/test_gpu_absgrad.py runs on the device."""
    cases.check_operator(operator_on_sim, be)


def test_public_names():
    import FasterGSCudaBackend as B
    from harness.densify import GARDEN_SCHEDULE
    from harness.trainer import Gaussians, render_image_training_absgrad, training_iteration      # noqa: F401
    import inspect
    assert 'diff_rasterize_absgrad' in B.__all__
    assert GARDEN_SCHEDULE['absgrad'] is False and GARDEN_SCHEDULE['absgrad_threshold'] == 8e-4
    assert inspect.signature(training_iteration).parameters['absgrad'].default is False
    c = cases.case('partial_tiles')
    args = [c['params'][k] for k in helpers.NAMES]
    assert Gaussians(c['params'], 'cpu').abs_densification_info is None
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.diff_rasterize_absgrad(*args, torch.empty(0), cases.settings_of(c), torch.zeros(2, args[0].shape[0]))


def test_density_control_reads_the_absolute_statistic(be):
    """The harness on the simulation: with the schedule key on, fgs_adc_plan gets g.abs_densification_info and the signed tensor is not looked at; prune and
    sort carry the tensor."""
    from harness import densify as D
    from harness.trainer import Gaussians
    c = cases.case('partial_tiles')
    out = cases.run_once(be, 'partial_tiles', False)
    n = out['abs'].shape[1]

    def model():
        g = Gaussians({k: v.clone() for k, v in c['params'].items()}, 'cpu')
        g.training_setup(training_cameras_extent=4.0)
        g.abs_densification_info = torch.as_tensor(out['abs']).clone()
        return g

    threshold = float(np.median(out['abs'][1][out['abs'][1] > 0]))
    g = model()
    g.densification_info = torch.full((2, n), float('nan'))              # never read with the key on
    stats = D.adaptive_density_control(g, threshold, 0.005, False, generator=torch.Generator().manual_seed(1), ops_backend=be, absgrad=True)
    assert stats['cloned'] + stats['split'] > 0 and stats['total'] > n and g.abs_densification_info is None
    g2 = model()
    g2.densification_info = torch.as_tensor(out['abs']).clone()
    ref = D.adaptive_density_control(g2, threshold, 0.005, False, generator=torch.Generator().manual_seed(1), ops_backend=be)
    assert {k: stats[k] for k in ('cloned', 'split', 'pruned', 'total')} == {k: ref[k] for k in ('cloned', 'split', 'pruned', 'total')}
    assert torch.equal(g.means, g2.means)
    g3 = model()
    keep = torch.arange(n) % 3 != 0
    D.prune(g3, ~keep, ops_backend=be)
    assert torch.equal(g3.abs_densification_info, torch.as_tensor(out['abs'])[:, keep])
    order = torch.randperm(int(keep.sum()), generator=torch.Generator().manual_seed(2))
    expected = g3.abs_densification_info[:, order].clone()
    D.sort(g3, order, ops_backend=be)
    assert torch.equal(g3.abs_densification_info, expected)
    D.reset_densification_info(g3)
    assert g3.abs_densification_info.shape == (2, int(keep.sum())) and not g3.abs_densification_info.any()
