"""fgs_backward_pose, Backend.backward_pose and diff_rasterize_pose on the CPU simulation of the product library (the unmodified .hip sources): the
gradient of the training render with respect to the camera (w2c rows 0..2, cam_position). Definitions, reference, upstream gradients and bars:
tests/pose_grad_cases.py. The same comparisons run on the MI355X in tests/test_gpu_pose_grad.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import aux_grad_cases as aux
import helpers
import pose_grad_cases as cases


@pytest.fixture(scope='module')
def be():
    return helpers.sim_backend(product=True)


@pytest.fixture()
def operator_on_sim(be, monkeypatch):
    """The public operators (FasterGSCudaBackend.rasterization, unmodified) running on the simulation backend with CPU tensors."""
    import FasterGSCudaBackend as B
    import FasterGSCudaBackend.rasterization as R
    monkeypatch.setattr(R, 'default_backend', lambda: be)
    monkeypatch.setattr(R, '_require_gpu', lambda t: None)
    return B


# ---- the reference, pinned twice ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['partial_tiles', 'stacked'])
def test_reference_with_detached_camera_is_the_trusted_one(name):
    """Camera leaves detached: the restatement gives aux_autograd_reference's maps and six gradients (same operations, same order)."""
    c = cases.case(name)
    mine = cases.pose_autograd_reference(c['named'], c['S'], c['f'], c['gC'], c['gA'], c['gD'], camera_leaves=False)
    theirs = aux.aux_autograd_reference(c['named'], c['S'], c['f'], c['gC'], c['gA'], c['gD'])
    with_leaves = cases.reference(name)
    for k in ('image', 'alpha', 'depth') + helpers.GRAD_KEYS:
        assert helpers.rel_inf(mine[k], theirs[k]) < 1e-12, (name, k)
        assert helpers.rel_inf(with_leaves[k], theirs[k]) < 1e-12, (name, k)
    assert 'w2c' not in mine and with_leaves['w2c'].shape == (3, 4) and with_leaves['cam'].shape == (3,)


def test_reference_camera_gradients_agree_with_central_differences():
    """gA = gD = 0: the 15 camera gradients of the restatement against fp64 central differences of oracle/torch_check.py: autograd_reference(loss_only=True)
    under perturbed settings (discrete structure held fixed, as in test_oracle.py's parameter differences).
    The loss is only piecewise smooth -- a pair that crosses alpha = 1/255 or T = 1e-4 between the two evaluations adds a jump autograd does not see -- so gC
    is zero on every pixel that owns a pair within 1e-2 (relative) of either threshold: a step h moves log(alpha) by at most
    h * |d expo / d mean2d| * |d mean2d / d entry| <= h * sqrt(2 * 5.5 / 0.3) * focal * |m| / z ~ 250 h, far inside the band. Without proper antialiasing:
    with it the reference DETACHES the opacity factor, which central differences cannot.
    Step: truncation h^2 |f'''| / 6 against rounding eps |L| / h, with each derivative of L in a camera entry ~ focal |m| / z ~ 40 times the one before
    and |L| ~ |f'| here: balance at h ~ (3 * 1.1e-16 / 1600) ^ (1/3) ~ 6e-7 ... 6e-6 depending on the entry; h = 2e-6. Both terms are then below
    1e-8 of |f'| (truncation 4e-12 * 1600 / 6, rounding 1.1e-16 * 1e3 summands / 2e-6); the bar is 1e-6 of the largest entry, two decades above."""
    from harness.scenes import View, make_s0
    from oracle import oracle as O
    from oracle.torch_check import autograd_reference
    O.build()
    p, v = make_s0(seed=21, n=16)
    p['means'][:, :2] *= 0.4
    v = View(v.w2c, v.position, 48, 36, 40.0, 40.0, 24.0, 18.0, 0.2, 1e4, torch.tensor([0.1, 0.3, 0.6]))
    S, _ = helpers.settings_pair(v, 16, False)
    named = aux.named_params(p)
    f = O.forward(*helpers.np_params(p), S, bucket_size=64)
    assert f['V'] >= 8
    near_threshold = helpers.flip_masks(O, f, S, eps=1e-2, eps_T=1e-2)['pixel']
    here = cases.pose_autograd_reference(named, S, f, None, None, None, forward_only=True)
    S2 = cases.moved(S, cases.rigid_motion(7, np.deg2rad(0.3), 0.008))
    there = cases.pose_autograd_reference(named, S2, O.forward(*helpers.np_params(p), S2, bucket_size=64), None, None, None, forward_only=True)
    gC = here['image'] - there['image']
    gC[:, near_threshold] = 0.0
    assert float(near_threshold.mean()) < 0.01 and np.abs(gC).max() > 0
    zero = np.zeros((v.height, v.width))
    ref = cases.pose_autograd_reference(named, S, f, gC, zero, zero)
    S64 = dataclasses.replace(S, w2c=np.asarray(S.w2c, np.float64)[:3, :4].copy(), cam_position=np.asarray(S.cam_position, np.float64).copy())
    h = 2e-6
    fd = {'w2c': np.zeros((3, 4)), 'cam': np.zeros(3)}
    for key, field in (('w2c', 'w2c'), ('cam', 'cam_position')):
        base = getattr(S64, field)
        for idx in np.ndindex(*fd[key].shape):
            vals = []
            for sign in (1.0, -1.0):
                moved = base.copy()
                moved[idx] += sign * h
                vals.append(autograd_reference(named, dataclasses.replace(S64, **{field: moved}), f, gC, loss_only=True))
            fd[key][idx] = (vals[0] - vals[1]) / (2.0 * h)
    report = {k: helpers.rel_inf(ref[k], fd[k]) for k in fd}
    print('restated reference vs central differences (h = 2e-6):', report, 'largest entries', {k: float(np.abs(fd[k]).max()) for k in fd})
    assert all(np.abs(fd[k]).max() > 0 for k in fd)
    assert report['w2c'] < 1e-6 and report['cam'] < 1e-6, report


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_scenes_reach_every_path():
    """Reference side only: the zeroed-pixel cap everywhere; a partial last wave in the only workgroup; reached Gaussians beyond the clip range in x and
    in y (counted from the reference's projection and compositing weights); the antialiasing, the one-basis and the hot case inherited."""
    for name in cases.CASES:
        c = cases.case(name)
        assert float((~c['keep']).mean()) <= cases.MAX_ZEROED, name
    n = cases.case('ragged')['f']['N']
    assert n < 256 and n % 64 != 0
    c = cases.case('clipped')
    (l, r, t, b), xy, reached = c['clip'], c['xy'], c['reached']
    out_x, out_y = reached & ((xy[:, 0] < l) | (xy[:, 0] > r)), reached & ((xy[:, 1] < t) | (xy[:, 1] > b))
    print('clipped: reached', int(reached.sum()), 'beyond the clip range in x', int(out_x.sum()), 'in y', int(out_y.sum()))
    assert out_x.sum() >= 1 and out_y.sum() >= 1 and c['aa'] is True
    assert cases.CASES['stacked'][1] == 1 and cases.CASES['partial_tiles'][2] is True and set(aux.CASES) < set(cases.CASES)


@pytest.mark.parametrize('name', list(cases.CASES))
def test_scenes_are_well_conditioned_in_float32(name):
    """Precondition of the bar: the SAME torch graph evaluated in float32 stays inside 1e-4 of its fp64 value on every scene, with and without map gradients."""
    for maps in (False, True):
        r64, r32 = cases.reference(name, maps), cases.reference(name, maps, torch.float32)
        report = {k: helpers.rel_inf(r32[k], r64[k]) for k in cases.CAMERA_KEYS}
        print('float32 graph vs fp64', name, 'maps' if maps else 'rgb', report)
        assert all(v < cases.GRAD_TOL for v in report.values()), (name, maps, report)
        assert np.abs(r64['w2c']).max() > 0 and (cases.CASES[name][1] == 1 or np.abs(r64['cam']).max() > 0)


# ---- the required checks ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.CASES))
def test_camera_gradients_match_the_fp64_reference(be, name):
    cases.check_camera_gradients(be, name)


@pytest.mark.parametrize('name', ['partial_tiles', 'ragged'])
def test_parameter_gradients_are_unchanged(be, name):
    cases.check_parameter_gradients_unchanged(be, name, exact=True)


def test_recycled_path_delivers_its_partials(be):
    cases.check_recycled_path(be, exact=True)


def test_result_does_not_depend_on_the_scratch(be):
    cases.check_scratch_independence(be, exact=True)


def test_degenerate_inputs(be):
    cases.check_degenerate_inputs(be)


def test_translation_identity_over_many_partials(be):
    cases.check_translation_identity(be)


def test_public_operator(be, operator_on_sim):
    cases.check_public_operator(operator_on_sim, be, 'cpu')


def test_it_refines_a_pose(operator_on_sim):
    cases.check_refinement('cpu', steps=24)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_surface(be):
    """The two exports, the scratch sizes, the argument errors fgs_backward_recycled reports, the public names."""
    _lib, _ = helpers.backend_modules()
    assert {'fgs_backward_pose', 'fgs_backward_pose_scratch_bytes'} <= set(_lib.EXPORTED_SYMBOLS)
    libs = [be.lib] + ([_lib.bind(_lib.DEFAULT_LIBRARY)] if _lib.DEFAULT_LIBRARY.exists() else [])
    for lib in libs:
        assert lib.fgs_abi_version() == 3
        aux_bytes, pose_bytes = lib.fgs_backward_aux_scratch_bytes(1000, 128, 128), lib.fgs_backward_pose_scratch_bytes(1000, 128, 128)
        assert pose_bytes >= aux_bytes + 16 * 64 + 128 * 16 * 8 and lib.fgs_backward_pose_scratch_bytes(-1, 128, 128) == 0
        assert lib.fgs_backward_pose_scratch_bytes(0, 128, 128) >= lib.fgs_backward_aux_scratch_bytes(0, 128, 128)
    c = cases.case('partial_tiles')
    n = c['f']['N']
    flags = torch.zeros((n + 63) // 64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='prior_blocks without reached_blocks'):
        cases.run(be, c, c['gC'], None, None, prior_blocks=flags)
    with pytest.raises(RuntimeError, match='aliases'):
        cases.run(be, c, c['gC'], None, None, prior_blocks=flags, reached_blocks=flags)
    st = _lib.ForwardState()
    S = _lib.Settings(1, 1, 1, 16, 15, 128, 128, 1.0, 1.0, 0.0, 0.0, 0.2, 100.0, 0)
    assert be.lib.fgs_backward_pose(*([None] * 22), 0, C.byref(S), C.byref(st), None, None, None, None, None, None) == -1
    assert b'NULL scratch buffer' in be.lib.fgs_last_error()
    import FasterGSCudaBackend as B
    from harness.pose import PoseDelta, refine_pose      # noqa: F401
    assert 'diff_rasterize_pose' in B.__all__
    args = [c['params'][k] for k in helpers.NAMES]
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        B.diff_rasterize_pose(*args, torch.empty(0), cases.settings_of(c))
    with pytest.raises(ValueError, match=r'w2c must be \[4,4\] or \[3,4\]'):
        B.diff_rasterize_pose(*args, torch.empty(0), cases.settings_of(c), w2c=torch.eye(3))
    w, cam = PoseDelta()(torch.eye(4))
    assert torch.equal(w, torch.eye(4)) and not cam.any()
