"""fgs_inference_aux on the MI355X: the comparisons of tests/test_aux_render.py against the same references (tests/aux_render_cases.py: definitions,
bars, exclusion caps), the colour bit-identical to fgs_inference for the full product of layouts and map requests, and the public `rasterize_aux`."""
import itertools

import numpy as np
import pytest
import torch

import aux_render_cases as cases
import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BG = (0.3, 0.1, 0.9)


@pytest.mark.parametrize('name', list(cases.SCENES))
def test_maps_match_the_references_on_device(hip_backend, name):
    ref = cases.reference(name)
    out = cases.render(hip_backend, ref, device=DEV)
    cases.check_maps(out, ref, name + ' (device)')
    # Every median is the float behind some Gaussian's depth key, bit for bit (also inside the excluded pixels: a flip picks another Gaussian, not another
    # float): blend_forward.hip is built with FMA contraction and K1 without, so this is what notices view_depth losing its contract-off pragma
    blended = out['depth_median'][ref['n_processed'] > 0]
    assert np.isin(blended, ref['z']).all(), int((~np.isin(blended, ref['z'])).sum())
    colourful = dict(ref, params=dict(ref['params'], sh_coefficients_0=ref['params']['sh_coefficients_0'] * 3.0))
    _, RS = helpers.settings_pair(ref['view'], bg=BG, device=DEV)
    plain = hip_backend.inference(*[colourful['params'][k].to(DEV) for k in helpers.NAMES], RS, True, True).cpu().numpy()
    coloured = cases.render(hip_backend, colourful, device=DEV, bg=BG)
    assert np.array_equal(coloured['rgb'], plain)
    for k in ('alpha', 'depth', 'depth_median'):                       # neither the colours nor the background are part of the maps
        assert np.array_equal(coloured[k], out[k]), k


def test_colour_is_bit_identical_for_every_layout_and_request(hip_backend):
    ref = cases.reference('partial_tiles')
    ref = dict(ref, params=dict(ref['params'], sh_coefficients_0=ref['params']['sh_coefficients_0'] * 3.0))
    _, RS = helpers.settings_pair(ref['view'], bg=BG, device=DEV)
    dp = [ref['params'][k].to(DEV) for k in helpers.NAMES]
    full = cases.render(hip_backend, ref, device=DEV, bg=BG)
    for to_chw, clamp in itertools.product((True, False), repeat=2):
        plain = hip_backend.inference(*dp, RS, to_chw, clamp).cpu().numpy()
        for want in itertools.product((False, True), repeat=3):
            if not any(want):
                continue
            out = cases.render(hip_backend, ref, device=DEV, to_chw=to_chw, clamp=clamp, alpha=want[0], depth_expected=want[1], depth_median=want[2], bg=BG)
            assert set(out) == {'rgb'} | {k for k, w in zip(('alpha', 'depth', 'depth_median'), want) if w}
            assert np.array_equal(out['rgb'], plain), (to_chw, clamp, want)
            for k in set(out) - {'rgb'}:
                assert np.array_equal(out[k], full[k]), (to_chw, clamp, want, k)


def test_no_gaussians_on_device(hip_backend):
    p, view = cases.partial_tiles_scene()
    _, RS = helpers.settings_pair(view, bg=BG, device=DEV)
    out = hip_backend.inference_aux(*[p[k][:0].contiguous().to(DEV) for k in helpers.NAMES], RS, True, True)
    assert torch.equal(out['rgb'].cpu(), torch.tensor(BG).view(3, 1, 1).expand(3, view.height, view.width))
    assert all(not out[k].any() for k in ('alpha', 'depth', 'depth_median'))


def test_rasterize_aux_agrees_with_rasterize_on_a_garden_scene():
    """The public operators on make_garden_like(60 000) at 320 x 240: bit-identical colour, and the maps hang together (the normalised expected depth of a
    pixel lies between the nearest and the farthest depth, the median is one of the Gaussians' depths, alpha is in [0, 1])."""
    import FasterGSCudaBackend as B
    from harness.scenes import look_at_view, make_garden_like
    params = {k: v.to(DEV) for k, v in make_garden_like(60_000).items()}
    view = look_at_view((5.0, -1.5, 0.0), (0.0, 0.0, 0.0), 320, 240, 237.0)
    _, RS = helpers.settings_pair(view, device=DEV)
    args = [params[k] for k in helpers.NAMES]
    for to_chw in (True, False):
        out = B.rasterize_aux(*args, RS, to_chw, depth='both')
        assert set(out) == {'rgb', 'alpha', 'depth', 'depth_median'}
        assert torch.equal(out['rgb'], B.rasterize(*args, RS, to_chw))
    alpha, depth, median = out['alpha'], out['depth'], out['depth_median']
    assert alpha.shape == depth.shape == median.shape == (240, 320)
    assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0 and float(alpha.max()) > 0.99
    m, r = params['means'].cpu(), view.w2c[2]
    z = (((r[0] * m[:, 0] + r[1] * m[:, 1]) + r[2] * m[:, 2]) + r[3]).to(DEV)      # view_depth's fp32 operations in its order, each rounded on its own
    hit = alpha > 1e-3
    mean_depth = B.rasterize_aux(*args, RS, True, alpha=False, depth='expected', normalize_depth=True)
    assert set(mean_depth) == {'rgb', 'depth'} and torch.equal(mean_depth['depth'], depth / alpha.clamp_min(1e-8))
    assert float(mean_depth['depth'][hit].min()) > 0.2 and float(mean_depth['depth'][hit].max()) <= float(z.max()) * (1.0 + 1e-5)
    assert bool(torch.isin(median[hit], z).all())                       # the median is the depth of one of the Gaussians, bit for bit
    only_median = B.rasterize_aux(*args, RS, True, alpha=False, depth='median')
    assert set(only_median) == {'rgb', 'depth_median'} and torch.equal(only_median['depth_median'], median)
