"""fgs_forward_aux / fgs_backward_aux on the CPU simulation of the product library (the unmodified .hip sources): differentiable accumulated opacity and
expected depth of the training render. Definitions, reference, upstream gradients and bars: tests/aux_grad_cases.py. The same comparisons run on the
MI355X in tests/test_gpu_aux_grad.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import aux_grad_cases as cases
import helpers


@pytest.fixture(scope='module')
def be():
    return helpers.sim_backend(product=True)


def test_reference_reproduces_the_trusted_one_without_map_gradients():
    """gA = gD = 0: the new fp64 reference IS oracle/torch_check.py: autograd_reference (image and all six gradients)."""
    from oracle.torch_check import autograd_reference
    for name in ('partial_tiles', 'stacked'):
        c = cases.case(name)
        mine = cases.reference_rgb(name)
        theirs = autograd_reference(cases.named_params(c['params']), c['S'], c['f'], c['gC'])
        assert np.abs(mine['image'] - theirs['image']).max() < 1e-12
        for k in helpers.GRAD_KEYS:
            assert helpers.rel_inf(mine[k], theirs[k]) < 1e-12, (name, k)
        assert np.abs(mine['alpha'] - (1.0 - c['f']['final_T'].reshape(mine['alpha'].shape)))[c['keep']].max() < 1e-5


def test_the_scenes_reach_every_path():
    """Conditions on the scenes (reference side only): zeroed pixels within the cap everywhere, a hot Gaussian in `hot`, several buckets per tile and early
    termination in `stacked`, partial tiles, the antialiasing and the single-SH-base case."""
    for name in cases.CASES:
        c = cases.case(name)
        assert float((~c['keep']).mean()) <= cases.MAX_ZEROED, name
    hot = cases.case('hot')
    f, view = hot['f'], hot['view']
    assert (view.width + 15) // 16 >= 20 and (view.height + 11) // 12 >= 20 and f['N'] <= 150
    sb = f['screen_bounds'].astype(np.int64)
    tiles = ((sb[:, 1] + 15) // 16 - sb[:, 0] // 16) * ((sb[:, 3] + 11) // 12 - sb[:, 2] // 12)
    blended = np.zeros(f['N'], bool)
    blended[f['inst_prims']] = True
    assert ((tiles > cases.HOT_FOOTPRINT) & blended).sum() >= 1 and ((tiles <= cases.HOT_FOOTPRINT) & blended).sum() >= 1
    st = cases.case('stacked')
    lengths = (st['f']['ranges'][:, 1] - st['f']['ranges'][:, 0]).astype(np.int64)
    assert lengths.max() > 3 * 192 and st['f']['n_processed'].max() > 64            # several buckets per tile are walked: ckpt_d planes that matter
    assert (st['f']['final_T'] < 1e-4).any()                                         # early termination
    assert cases.CASES['partial_tiles'][2] is True and cases.CASES['stacked'][1] == 1
    pt = cases.case('partial_tiles')['view']
    assert pt.width % 16 and pt.height % 12


@pytest.mark.parametrize('name', list(cases.CASES))
def test_maps_image_and_gradients_match_the_fp64_reference(be, name):
    cases.check_against_reference(be, name)


_RUNS = {}


def _full(be, name='partial_tiles'):
    if name not in _RUNS:
        c = cases.case(name)
        _RUNS[name] = cases.run(be, c, c['gC'], c['gA'], c['gD'])
    return _RUNS[name]


def test_no_map_gradients_is_the_plain_backward(be):
    """(a) gA = gD = None: the gradients of the plain path, on buffers the aux forward pass filled."""
    c = cases.case('partial_tiles')
    out = cases.run(be, c, c['gC'], None, None)
    plain = cases.run_plain(be, c, c['gC'])
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(out[k], plain[k]) < 1e-6, k


@pytest.mark.parametrize('name', ['partial_tiles', 'stacked'])
def test_gradients_are_linear_in_the_upstream_gradients(be, name):
    """(b) the pass for (gC, gA, gD) equals the sum of three passes with one of them at a time."""
    c = cases.case(name)
    full = _full(be, name)
    zC, zM = np.zeros_like(c['gC']), np.zeros_like(c['gA'])
    parts = [cases.run(be, c, c['gC'], None, None), cases.run(be, c, zC, c['gA'], None), cases.run(be, c, zC, zM, c['gD'])]
    for k in helpers.GRAD_KEYS:
        total = parts[0][k].astype(np.float64) + parts[1][k] + parts[2][k]
        assert helpers.rel_inf(full[k], total) < 1e-5, (name, k)


def test_depth_gradient_alone_leaves_the_colours_alone(be):
    """(c) only gD non-zero: the SH gradients are exactly zero, the geometry ones are not."""
    c = cases.case('partial_tiles')
    out = cases.run(be, c, np.zeros_like(c['gC']), None, c['gD'])
    assert not out['sh0'].any() and not out['sh_rest'].any()
    for k in ('means', 'scales', 'rotations', 'opacities'):
        assert np.abs(out[k]).max() > 0, k


def test_second_backward_over_the_same_buffers(be):
    """(d) a retained graph differentiated twice: acc_z and the accumulator records are cleared by every depth pass."""
    c = cases.case('hot')
    first = cases.run(be, c, c['gC'], c['gA'], c['gD'])
    second = cases.run(be, c, c['gC'], c['gA'], c['gD'], res=first['res'])
    for k in helpers.GRAD_KEYS:
        assert helpers.rel_inf(second[k], first[k]) < 1e-6, k


def test_plain_backward_on_aux_forward_buffers(be):
    """(e) fgs_backward on buffers filled by fgs_forward_aux equals the plain path (the plain blob layouts are prefixes of the aux ones)."""
    c = cases.case('stacked')
    RS = cases.settings_of(c)
    p = [c['params'][k] for k in helpers.NAMES]
    res = be.forward_aux(*p, RS)
    gi = torch.as_tensor(c['gC'])
    grads = be.backward(None, gi, res.image, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
    plain = cases.run_plain(be, c, c['gC'])
    assert np.array_equal(res.image.numpy(), plain['image'])
    for k, g in zip(helpers.GRAD_KEYS, grads):
        assert helpers.rel_inf(g.numpy(), plain[k]) < 1e-6, k
    n, v = p[0].shape[0], c['view']
    assert 'ckpt_d' not in be.blob_layout(3, n, v.width, v.height, res.state[1], res.state[2])      # fgs_blob_layout answers for the plain pass


def test_single_map_requests(be):
    """Either map pointer may be NULL: the other map and the image do not change."""
    c = cases.case('partial_tiles')
    RS = cases.settings_of(c)
    p = [c['params'][k] for k in helpers.NAMES]
    both = _full(be)
    only_a, only_d = be.forward_aux(*p, RS, alpha=True, depth=False), be.forward_aux(*p, RS, alpha=False, depth=True)
    assert only_a.depth is None and only_d.alpha is None
    assert np.array_equal(only_a.alpha.numpy(), both['alpha']) and np.array_equal(only_d.depth.numpy(), both['depth'])
    assert np.array_equal(only_a.image.numpy(), both['image']) and np.array_equal(only_d.image.numpy(), both['image'])


def test_maps_do_not_depend_on_stale_scratch_memory(be):
    c = cases.case('stacked')
    out = cases.run(helpers.poisoned(be), c, c['gC'], c['gA'], c['gD'])
    clean = _full(be, 'stacked')
    for k in ('image', 'alpha', 'depth') + helpers.GRAD_KEYS:
        assert helpers.rel_inf(out[k], clean[k]) < 1e-6, k


def test_abi_error_cases(be):
    """(f) both map pointers NULL; a depth gradient on buffers of a plain forward pass; the out-of-scope combinations."""
    _lib, _ = helpers.backend_modules()
    st = _lib.ForwardState()
    cb = _lib.RESIZE_FN(lambda u, w, n: 0)
    S = _lib.Settings(1, 1, 1, 16, 15, 128, 128, 1.0, 1.0, 0.0, 0.0, 0.2, 100.0, 0)
    libs = [be.lib] + ([_lib.bind(_lib.DEFAULT_LIBRARY)] if _lib.DEFAULT_LIBRARY.exists() else [])
    for lib in libs:
        assert lib.fgs_forward_aux(None, None, None, None, None, None, 0, C.byref(S), 1, None, None, cb, None, C.byref(st), None) == -1
        assert b'alpha' in lib.fgs_last_error() and b'depth_expected' in lib.fgs_last_error() and b'NULL' in lib.fgs_last_error()
        assert lib.fgs_abi_version() == 3
    c = cases.case('partial_tiles')
    RS = cases.settings_of(c)
    p = [c['params'][k] for k in helpers.NAMES]
    plain = be.forward(*p, RS)
    gi, gm = torch.as_tensor(c['gC']), torch.as_tensor(c['gD'])
    with pytest.raises(RuntimeError, match='depth checkpoints'):
        be.backward_aux(None, gi, None, gm, plain.image, gm, p[0], p[1], p[2], p[3], p[5], plain.buffers, RS, plain.state)
    # an alpha gradient needs no depth checkpoint: plain-forward buffers serve
    aux = _full(be)
    only_alpha = be.backward_aux(None, gi, torch.as_tensor(c['gA']), None, plain.image, None, p[0], p[1], p[2], p[3], p[5], plain.buffers, RS, plain.state)
    ref = cases.run(be, c, c['gC'], c['gA'], None, res=aux['res'])
    for k, g in zip(helpers.GRAD_KEYS, only_alpha):
        assert helpers.rel_inf(g.numpy(), ref[k]) < 1e-6, k
    with pytest.raises(RuntimeError, match='asynchronous'):
        be.forward_aux(*p, RS, instance_capacity=1 << 20)
    with pytest.raises(RuntimeError, match='neither alpha nor depth'):
        be.forward_aux(*p, RS, alpha=False, depth=False)
    with pytest.raises(RuntimeError, match='takes no alpha / depth gradients'):
        be.backward_adam_fused(None, gi, plain.image, [], [], [], plain.buffers, RS, plain.state, 1, [], grad_depth=gm)
    with pytest.raises(RuntimeError, match='takes no alpha / depth gradients'):
        be.backward_to_records(gi, plain.image, plain.buffers, RS, plain.state, 15, grad_alpha=gm)


def test_no_gaussians(be):
    """(g) n = 0: background, zero maps, and a backward pass that returns empty gradients."""
    c = cases.case('partial_tiles')
    view = c['view']
    bg = (0.3, 0.1, 0.9)
    _, RS = helpers.settings_pair(view, bg=bg)
    empty = [c['params'][k][:0].contiguous() for k in helpers.NAMES]
    res = be.forward_aux(*empty, RS)
    assert torch.equal(res.image, torch.tensor(bg).view(3, 1, 1).expand(3, view.height, view.width))
    assert res.alpha.shape == res.depth.shape == (view.height, view.width) and not res.alpha.any() and not res.depth.any()
    grads = be.backward_aux(None, torch.ones_like(res.image), torch.ones_like(res.alpha), torch.ones_like(res.depth), res.image, res.depth,
                            empty[0], empty[1], empty[2], empty[3], empty[5], res.buffers, RS, res.state)
    assert all(g.shape[0] == 0 for g in grads)


def test_public_names():
    import FasterGSCudaBackend as B
    from harness.trainer import render_image_training_aux, training_iteration      # noqa: F401
    assert 'diff_rasterize_aux' in B.__all__
    c = cases.case('partial_tiles')
    args = [c['params'][k] for k in helpers.NAMES]
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.diff_rasterize_aux(*args, torch.empty(0), cases.settings_of(c))
    with pytest.raises(ValueError, match='neither alpha nor depth'):
        B.diff_rasterize_aux(*args, torch.empty(0), cases.settings_of(c), alpha=False, depth=False)
