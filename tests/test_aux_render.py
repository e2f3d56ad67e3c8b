"""fgs_inference_aux on the CPU simulation of the product library (helpers.sim_backend(product=True): the unmodified .hip sources): the colour is
bit-identical to fgs_inference in every output layout and for every combination of requested maps, and accumulated opacity, expected depth and
median depth agree with the references of tests/aux_render_cases.py (definitions, bars and exclusion caps there). The same comparisons run on the
MI355X in tests/test_gpu_aux_render.py."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import aux_render_cases as cases
import helpers


@pytest.fixture(scope='module')
def be():
    return helpers.sim_backend(product=True)


def _colourful(ref):
    """The scene with colours pushed outside [0, 1] (the clamp matters) -- for the colour comparisons only."""
    params = dict(ref['params'])
    params['sh_coefficients_0'] = params['sh_coefficients_0'] * 3.0
    return dict(ref, params=params)


@pytest.mark.parametrize('name', list(cases.SCENES))
def test_maps_match_the_references(be, name):
    ref = cases.reference(name)
    out = cases.render(be, ref)
    assert out['alpha'].shape == out['depth'].shape == out['depth_median'].shape == (ref['view'].height, ref['view'].width)
    cases.check_maps(out, ref, name)


def test_the_scenes_reach_every_path_of_the_walk():
    """Conditions on the scenes themselves (reference side only): what each of them is there for."""
    st = cases.reference('stacked')
    f, npr = st['f'], st['n_processed']
    lengths = (f['ranges'][:, 1] - f['ranges'][:, 0]).astype(np.int64)
    assert lengths.max() > 3 * 192 and npr.max() > 3 * 192                      # a list of more than three batches, walked into the fourth
    assert not npr[:8].any() and not npr[-8:].any() and not npr[:, :8].any() and not npr[:, -8:].any()   # the empty border
    # the pixel under the front Gaussian of the opaque stack (primitive 700): terminated early, its median is that first Gaussian
    x, y = (int(v) for v in f['mean2d'][700])
    tile = (y // 12) * f['grid'][0] + x // 16
    assert 0 < npr[y, x] < lengths[tile] and 1.0 - st['alpha'][y, x] < 1e-4
    assert st['median'][y, x] == st['z'][700] and st['z'][700] == st['z'][f['inst_prims'][f['ranges'][tile, 0]:f['ranges'][tile, 1]]].min()
    # the middle of the faint stack becomes more than half opaque dozens of entries in: the median is neither the first nor the last Gaussian blended
    cy, cx = 48, 64
    assert st['alpha'][cy, cx] > 0.5 and st['z'].max() > st['median'][cy, cx] > st['z'][:700].min()
    pt = cases.reference('partial_tiles')
    assert pt['view'].width % 16 and pt['view'].height % 12 and pt['n_processed'][:, -1].any() and pt['n_processed'][-1].any()   # live partial tiles
    # pixels that stay more than half transparent: the median is the last Gaussian blended (non-zero wherever anything was blended)
    s0 = cases.reference('s0')
    faint = (s0['alpha'] < 0.5) & (s0['n_processed'] > 0)
    assert faint.any() and (s0['median'][faint] > 0).all()


_RUNS = {}


def _reference_run(be):
    """All three maps of the partial-tiles scene as it stands (CHW, black background), rendered once for the tests that compare against them."""
    if 'maps' not in _RUNS:
        _RUNS['maps'] = cases.render(be, cases.reference('partial_tiles'))
    return _RUNS['maps']


LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]            # (to_chw, clamp_output)
MAP_REQUESTS = [w for w in itertools.product((False, True), repeat=3) if any(w)]  # (alpha, expected depth, median depth) wanted: NULL / non-NULL pointers


@pytest.mark.parametrize('to_chw,clamp', LAYOUTS)
def test_colour_is_bit_identical_to_plain_inference(be, to_chw, clamp):
    """Both layouts x clamp on and off x every combination of NULL / non-NULL map pointers; and a map depends neither on the layout of the colour nor on
    which other maps were asked for (every map is held to the one of the black-background reference run)."""
    ref = _colourful(cases.reference('partial_tiles'))
    bg = (0.3, 0.1, 0.9)
    _, RS = helpers.settings_pair(ref['view'], bg=bg)
    plain = be.inference(*[ref['params'][k] for k in helpers.NAMES], RS, to_chw, clamp).numpy()
    assert plain.shape == ((3, 50, 70) if to_chw else (50, 70, 3)) and (clamp or plain.max() > 1.0)
    maps = _reference_run(be)
    for want in MAP_REQUESTS:
        out = cases.render(be, ref, to_chw=to_chw, clamp=clamp, alpha=want[0], depth_expected=want[1], depth_median=want[2], bg=bg)
        assert set(out) == {'rgb'} | {k for k, w in zip(('alpha', 'depth', 'depth_median'), want) if w}
        assert np.array_equal(out['rgb'], plain), want
        for k in set(out) - {'rgb'}:
            assert np.array_equal(out[k], maps[k]), (want, k)


@pytest.mark.parametrize('name', ['s0', 'stacked'])
def test_colour_is_bit_identical_on_the_other_scenes(be, name):
    ref = _colourful(cases.reference(name))
    _, RS = helpers.settings_pair(ref['view'], bg=(0.3, 0.1, 0.9))
    plain = be.inference(*[ref['params'][k] for k in helpers.NAMES], RS, True, True).numpy()
    assert np.array_equal(cases.render(be, ref, bg=(0.3, 0.1, 0.9))['rgb'], plain)


def test_the_background_is_no_part_of_the_maps(be):
    ref = cases.reference('partial_tiles')
    black, coloured = _reference_run(be), cases.render(be, ref, bg=(0.3, 0.1, 0.9))
    assert not np.array_equal(black['rgb'], coloured['rgb'])
    for k in ('alpha', 'depth', 'depth_median'):
        assert np.array_equal(black[k], coloured[k]), k


def test_no_gaussians(be):
    p, view = cases.partial_tiles_scene()
    empty = {k: v[:0].contiguous() for k, v in p.items()}
    bg = (0.3, 0.1, 0.9)
    _, RS = helpers.settings_pair(view, bg=bg)
    for to_chw in (True, False):
        out = be.inference_aux(*[empty[k] for k in helpers.NAMES], RS, to_chw, True)
        rgb = out['rgb'] if to_chw else out['rgb'].permute(2, 0, 1)
        assert torch.equal(rgb, torch.tensor(bg).view(3, 1, 1).expand(3, view.height, view.width))
        for k in ('alpha', 'depth', 'depth_median'):
            assert out[k].shape == (view.height, view.width) and not out[k].any(), k


def test_maps_do_not_depend_on_stale_scratch_memory(be):
    """Freshly (re)sized scratch buffers full of 0xFF bytes: the staged z must come from the means, never from what the record's last word held."""
    ref = cases.reference('stacked')
    _, RS = helpers.settings_pair(ref['view'])
    out = helpers.poisoned(be).inference_aux(*[ref['params'][k] for k in helpers.NAMES], RS, True, True)
    clean = cases.render(be, ref)
    for k in ('rgb', 'alpha', 'depth', 'depth_median'):
        assert np.array_equal(out[k].numpy(), clean[k]), k


def _call_with_no_map(lib, _lib):
    st = _lib.ForwardState()
    cb = _lib.RESIZE_FN(lambda u, w, n: 0)
    S = _lib.Settings(1, 1, 1, 16, 15, 128, 128, 1.0, 1.0, 0.0, 0.0, 0.2, 100.0, 0)
    return lib.fgs_inference_aux(None, None, None, None, None, None, 0, C.byref(S), 1, 1, 1, None, None, None, cb, None, C.byref(st), None)


def test_all_three_maps_null_is_an_invalid_argument(be):
    """... in the simulation and in libfgs_hip.so itself (the check comes before anything touches a device)."""
    _lib, _ = helpers.backend_modules()
    libs = [be.lib]
    if _lib.DEFAULT_LIBRARY.exists():
        libs.append(_lib.bind(_lib.DEFAULT_LIBRARY))
    for lib in libs:
        assert _call_with_no_map(lib, _lib) == -1
        message = lib.fgs_last_error()
        assert b'alpha' in message and b'depth_expected' in message and b'depth_median' in message and b'NULL' in message, message


def test_rasterize_aux_rejects_cpu_tensors_and_bad_requests():
    import FasterGSCudaBackend as B
    from harness.trainer import render_image_aux            # noqa: F401  (importable next to render_image_benchmark)
    ref = cases.reference('partial_tiles')
    _, RS = helpers.settings_pair(ref['view'])
    args = [ref['params'][k] for k in helpers.NAMES]
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.rasterize_aux(*args, RS, True)
    with pytest.raises(RuntimeError, match='no CPU implementation') as plain:
        B.rasterize(*args, RS, True)
    with pytest.raises(RuntimeError) as aux:
        B.rasterize_aux(*args, RS, False, depth='both', normalize_depth=True)
    assert str(aux.value) == str(plain.value)
    with pytest.raises(ValueError, match='depth must be'):
        B.rasterize_aux(*args, RS, True, depth='mean')
    with pytest.raises(ValueError, match='no auxiliary map'):
        B.rasterize_aux(*args, RS, True, alpha=False, depth=None)
    assert 'rasterize_aux' in B.__all__
