"""Normal-consistency regulariser (csrc/normal_consistency.hip): definitions, the fp64 reference, the seeded cases and the bars that
tests/test_normal_consistency.py (CPU simulation of the product sources) and tests/test_gpu_normal_consistency.py (MI355X) share.

Reference: the two definitions of INTEGRATION.md 'Normal consistency' written in torch with autograd -- `surface_features_of` (per Gaussian) and
`consistency_of` (per pixel) -- evaluated in fp64; no gradient is derived by hand. The same two functions evaluated in fp32 are the "fp32 restatement":
what any fp32 evaluation of the definitions loses against fp64, measured before the kernels are held to a bar, and the stand-in for the two operators in
the composition test (6).

Bar: the project's, helpers.rel_inf < 1e-4 per output tensor against fp64 (aux_grad_cases.GRAD_TOL). The depth normal divides differences of
neighbouring depths by their length, which amplifies the rounding of D / A by about f / 2 pixels of slope, so the views keep f <= 60; a case whose
fp32 restatement itself exceeds 1e-5 would be ill-conditioned and is replaced, not given a wider bar (test_cases_are_well_conditioned holds them to that).

rel_inf against fp64 as measured (FIGURES below holds the same numbers as data; they are recorded, the assertions are the two bars above):

    image case   (E, gN_r, gD, gA)   fp32 restatement (CPU)            kernels, simulation               kernels, MI355X
    small        37 x 29, f = 40     6.3e-7 9.6e-7 7.7e-7 6.8e-7       6.3e-7 9.6e-7 1.2e-6 9.7e-7       6.3e-7 9.6e-7 1.3e-6 1.1e-6
    multi        67 x 45, f = 60     1.1e-6 1.9e-6 1.9e-6 1.8e-6       1.1e-6 1.9e-6 1.6e-6 1.6e-6       1.1e-6 1.9e-6 1.7e-6 1.8e-6
    hole         67 x 45, f = 60     8.7e-7 1.8e-6 1.1e-6 1.2e-6       9.4e-7 1.8e-6 1.1e-6 1.2e-6       8.7e-7 1.8e-6 1.1e-6 1.3e-6
    exact        37 x 29, f = 40     5.7e-7 9.8e-7 7.5e-7 7.3e-7       5.7e-7 1.1e-6 5.9e-7 6.0e-7       5.7e-7 1.1e-6 4.8e-7 5.1e-7
    surface features, N = 1 .. 257 (features, grad_rotations; grad_means is exact):
                                     <= 6.2e-8, <= 2.5e-7              <= 6.7e-8, <= 3.4e-7              <= 5.3e-8, <= 3.0e-7
    composition (6), largest of E, the map and the six gradients against the fp32 restatement: simulation 6.1e-7, MI355X 6.2e-7 (bar 1e-5).
    regularisation (8): E.mean() 0.003937 -> 0.000492 in 8 Adam steps at lr 0.03, a factor of 0.125, on the simulation and on the MI355X (bar 0.5).

The kernels are no farther from fp64 than the fp32 torch restatement is: no figure uses more than a fiftieth of the bar.

Inputs are seeded. Image cases: d = a tilted plane plus noise, A drawn so that between 30 % and 80 % of the interior pixels are valid (asserted), N_r a
random direction of length <= A, D = d A rounded to fp32; gE = N(0, 1) / (H W). Gaussian cases: unnormalised quaternions, log-scales whose two
smallest differ by at least 0.05, |a . v| >= 1e-3 |v| (both asserted): no Gaussian sits on a discontinuity of the argmin or of the sign.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import aux_grad_cases as aux
import helpers

TOL = aux.GRAD_TOL              # 1e-4: every output tensor against fp64
RESTATEMENT_TOL = 1e-5          # an fp32 evaluation of the definitions beyond it: the case is ill-conditioned
OPERATOR_TOL_SIM = 1e-5         # composition against the fp32 restatement (the bar of the bilagrid operator test)
RUN_TO_RUN = 1e-5               # device: two runs of the rasterizer's backward pass differ by the order of its float atomics (test_gpu_bilagrid.py)
MIN_CROSS_SQ = 1e-30

# What was measured (rel_inf against fp64; recorded, not asserted -- the assertions are TOL and RESTATEMENT_TOL).
# restatement: the definitions in fp32 torch on the CPU; simulation: the kernels compiled by g++ (no FMA contraction); device: MI355X.
FIGURES = {
    'restatement': {'small': (6.3e-7, 9.6e-7, 7.7e-7, 6.8e-7), 'multi': (1.1e-6, 1.9e-6, 1.9e-6, 1.8e-6), 'hole': (8.7e-7, 1.8e-6, 1.1e-6, 1.2e-6),
                    'exact': (5.7e-7, 9.8e-7, 7.5e-7, 7.3e-7), 'surface_features': (6.2e-8, 2.5e-7, 0.0)},
    'simulation': {'small': (6.3e-7, 9.6e-7, 1.2e-6, 9.7e-7), 'multi': (1.1e-6, 1.9e-6, 1.6e-6, 1.6e-6), 'hole': (9.4e-7, 1.8e-6, 1.1e-6, 1.2e-6),
                   'exact': (5.7e-7, 1.1e-6, 5.9e-7, 6.0e-7), 'surface_features': (6.7e-8, 3.4e-7, 0.0), 'composition': 6.1e-7},
    'device': {'small': (6.3e-7, 9.6e-7, 1.3e-6, 1.1e-6), 'multi': (1.1e-6, 1.9e-6, 1.7e-6, 1.8e-6), 'hole': (8.7e-7, 1.8e-6, 1.1e-6, 1.3e-6),
               'exact': (5.7e-7, 1.1e-6, 4.8e-7, 5.1e-7), 'surface_features': (5.3e-8, 3.0e-7, 0.0), 'composition': 6.2e-7},
    'regularises': {'steps': 8, 'lr': 0.03, 'start': 0.003937, 'end': 0.000492, 'factor': 0.125},      # the same on the simulation and on the MI355X
}

# name: ((W, H), (fx, fy, cx, cy), min_alpha, what is special)
IMAGE_CASES = {
    'small': ((37, 29), (40.0, 38.0, 17.3, 15.9), 0.5, None),          # one or two workgroups per axis, partial tiles
    'multi': ((67, 45), (60.0, 57.0, 35.2, 20.6), 0.5, None),          # 3 x 6 workgroups of 32 x 8 pixels: both halos cross workgroup borders
    'hole': ((67, 45), (60.0, 57.0, 35.2, 20.6), 0.5, 'hole'),         # A = D = 0 over a block
    'exact': ((37, 29), (40.0, 38.0, 17.3, 15.9), 0.5, 'exact'),       # A takes min_alpha exactly at a third of the pixels
}
GAUSSIAN_COUNTS = (1, 63, 64, 65, 257)


# ---- the definitions, in torch, in the dtype asked for ----------------------------------------------------------------------------------------------------
def smallest_axis(scales: torch.Tensor) -> torch.Tensor:
    """Index of the smallest of the three log-scales, the lowest index on an exact tie."""
    k = torch.zeros(scales.shape[0], dtype=torch.long, device=scales.device)
    smallest = scales[:, 0]
    k = torch.where(scales[:, 1] < smallest, torch.ones_like(k), k)
    smallest = torch.minimum(smallest, scales[:, 1])
    return torch.where(scales[:, 2] < smallest, torch.full_like(k, 2), k)


def rotation_of(q: torch.Tensor) -> torch.Tensor:
    """[N,3,3] of raw quaternions (r, x, y, z): quat_to_rotation of csrc/fgs_math.h, normalisation included."""
    r, x, y, z = (q / q.norm(dim=1, keepdim=True)).unbind(dim=1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def surface_features_of(means, scales, rotations, w2c, cam_position, dtype=torch.float64) -> torch.Tensor:
    """Definition 1: [N,5] rows (n_cam, z, 1), differentiable in rotations and means."""
    means, rotations, w2c, cam = means.to(dtype), rotations.to(dtype), w2c.detach().to(dtype), cam_position.detach().to(dtype)
    n = means.shape[0]
    R = rotation_of(rotations)
    a = R[torch.arange(n, device=means.device), :, smallest_axis(scales.detach())]
    along = (a * (means - cam[None, :])).sum(dim=1).detach()
    s = torch.where(along > 0, -torch.ones_like(along), torch.ones_like(along))
    n_cam = (s[:, None] * a) @ w2c[:3, :3].T
    z = means @ w2c[2, :3] + w2c[2, 3]
    return torch.cat([n_cam, z[:, None], torch.ones_like(z)[:, None]], dim=1)


def consistency_of(surface_map, intrinsics, min_alpha, dtype=torch.float64):
    """Definition 2: (E [H,W], n_d [3,H,W], valid [H,W]) of a map [5,H,W] = (N_r, D, A). min_alpha and the intrinsics are taken as the fp32 numbers the
    C ABI receives; the comparison A >= min_alpha is made on the fp32 input, so it is the same in every dtype."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in intrinsics)
    ok = surface_map[4].detach() >= torch.tensor(min_alpha, dtype=torch.float32, device=surface_map.device)
    M = surface_map.to(dtype)
    Nr, D, A = M[:3], M[3], M[4]
    H, W = D.shape
    if W < 3 or H < 3:
        zero = (M * 0).sum(dim=0)
        return zero, torch.zeros_like(M[:3]), torch.zeros_like(ok)
    d = torch.where(ok, D / torch.where(ok, A, torch.ones_like(A)), torch.zeros_like(D))
    xs = ((torch.arange(W, dtype=dtype, device=M.device) + 0.5 - cx) / fx)[None, :]
    ys = ((torch.arange(H, dtype=dtype, device=M.device) + 0.5 - cy) / fy)[:, None]
    P = torch.stack([xs * d, ys * d, d])
    gx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    gy = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = torch.cross(gy, gx, dim=0)
    len_sq = (c * c).sum(dim=0)
    valid = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1] & (len_sq.detach() > MIN_CROSS_SQ)
    n_d = torch.where(valid[None], c / torch.sqrt(torch.where(valid, len_sq, torch.ones_like(len_sq)))[None], torch.zeros_like(c))
    E = torch.where(valid, A[1:-1, 1:-1] - (Nr[:, 1:-1, 1:-1] * n_d).sum(dim=0), torch.zeros_like(len_sq))
    everywhere = torch.zeros_like(ok)
    everywhere[1:-1, 1:-1] = valid
    return F.pad(E, (1, 1, 1, 1)), F.pad(n_d.detach(), (1, 1, 1, 1)), everywhere


def settings_for(size, intrinsics, device='cpu'):
    """RasterizerSettings that carry an image size and intrinsics (the operators read nothing else from them)."""
    _, _backend = helpers.backend_modules()
    (w, h), (fx, fy, cx, cy) = size, intrinsics
    return _backend.RasterizerSettings(torch.eye(4, device=device), torch.zeros(3, device=device), torch.zeros(3, device=device), 1, w, h, fx, fy, cx, cy,
                                       0.2, 1.0e4, False)


# ---- image cases --------------------------------------------------------------------------------------------------------------------------------------------
def make_map(size, intrinsics, seed: int, special=None) -> torch.Tensor:
    (w, h), gen = size, torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=gen)
    xs, ys = torch.arange(w, dtype=torch.float32)[None, :], torch.arange(h, dtype=torch.float32)[:, None]
    d = 3.0 + 0.012 * (xs - w / 2) + 0.007 * (ys - h / 2) + 0.01 * torch.randn(h, w, generator=gen)
    low = u(h, w) < 0.08
    if special == 'exact':                                       # sixteenths: 0.5 itself at a third of the pixels, 0.4375 just below it
        A = torch.randint(9, 17, (h, w), generator=gen).float() / 16.0
        A = torch.where(u(h, w) < 0.33, torch.full_like(A, 0.5), A)
        A = torch.where(low, torch.full_like(A, 0.4375), A)
    else:
        A = torch.where(low, 0.5 * u(h, w), 0.5 + 0.5 * u(h, w))
    direction = torch.randn(3, h, w, generator=gen)
    Nr = direction / direction.norm(dim=0, keepdim=True) * (A * u(h, w))[None]
    D = d * A
    M = torch.cat([Nr, D[None], A[None]]).contiguous()
    if special == 'hole':
        M[:, 10:21, 20:41] = 0.0
    return M


@functools.lru_cache(maxsize=None)
def image_case(name: str) -> dict:
    size, intrinsics, min_alpha, special = IMAGE_CASES[name]
    seed = 300 + sorted(IMAGE_CASES).index(name)
    M = make_map(size, intrinsics, seed, special)
    w, h = size
    gE = (torch.randn(h, w, generator=torch.Generator().manual_seed(seed + 50)) / (h * w)).contiguous()
    assert float((M[:3].norm(dim=0) - M[4]).max()) <= 1e-6, name                         # |N_r| <= A
    return {'name': name, 'map': M, 'gE': gE, 'size': size, 'intrinsics': intrinsics, 'min_alpha': min_alpha, 'special': special}


def consistency_with_gradient(M: torch.Tensor, gE: torch.Tensor, intrinsics, min_alpha: float, dtype) -> dict:
    """E, n_d, valid and gM = d sum(gE E) / dM of the definition in `dtype`, by autograd (numpy arrays)."""
    leaf = M.detach().cpu().clone().requires_grad_(True)
    E, n_d, valid = consistency_of(leaf, intrinsics, min_alpha, dtype)
    (E * gE.detach().cpu().to(dtype)).sum().backward()
    g = leaf.grad.numpy()
    return {'E': E.detach().numpy(), 'normals': n_d.numpy(), 'valid': valid.numpy(), 'gN': g[:3], 'gD': g[3], 'gA': g[4]}


@functools.lru_cache(maxsize=None)
def image_reference(name: str) -> dict:
    """The fp64 reference of an image case: once per process, shared, read-only."""
    c = image_case(name)
    ref = consistency_with_gradient(c['map'], c['gE'], c['intrinsics'], c['min_alpha'], torch.float64)
    w, h = c['size']
    ref['share'] = float(ref['valid'][1:-1, 1:-1].mean()) if w >= 3 and h >= 3 else 0.0
    return ref


IMAGE_KEYS = ('E', 'gN', 'gD', 'gA')


def image_errors(got: dict, ref: dict) -> dict:
    return {k: helpers.rel_inf(got[k], ref[k]) for k in IMAGE_KEYS}


def run_image(be, M, gE, size, intrinsics, min_alpha, device='cpu') -> dict:
    RS = settings_for(size, intrinsics, device)
    M, gE = M.to(device), gE.to(device)
    E, normals = be.normal_consistency(M, RS, min_alpha, return_normals=True)
    gM = be.normal_consistency_backward(M, gE, RS, min_alpha).cpu().numpy()
    return {'E': E.cpu().numpy(), 'normals': normals.cpu().numpy(), 'gN': gM[:3], 'gD': gM[3], 'gA': gM[4], 'gM': gM}


def check_cases_are_well_conditioned() -> dict:
    """First of all: the share of valid interior pixels is between 30 % and 80 %, and the definitions evaluated in fp32 torch stay below 1e-5 of fp64."""
    figures = {}
    for name in IMAGE_CASES:
        c, ref = image_case(name), image_reference(name)
        assert 0.3 <= ref['share'] <= 0.8, (name, ref['share'])
        f32 = consistency_with_gradient(c['map'], c['gE'], c['intrinsics'], c['min_alpha'], torch.float32)
        assert np.array_equal(f32['valid'], ref['valid']), name
        figures[name] = image_errors(f32, ref)
        print(f'normal consistency {name}: valid share {ref["share"]:.3f}, fp32 restatement vs fp64 {figures[name]}')
        assert max(figures[name].values()) < RESTATEMENT_TOL, (name, figures[name])
    for n in GAUSSIAN_COUNTS:
        c, ref = gaussian_case(n), gaussian_reference(n)
        f32 = features_with_gradient(c, torch.float32)
        figures[n] = {k: helpers.rel_inf(f32[k], ref[k]) for k in GAUSSIAN_KEYS}
        print(f'surface features N = {n}: fp32 restatement vs fp64 {figures[n]}')
        assert max(figures[n].values()) < RESTATEMENT_TOL, (n, figures[n])
    return figures


def check_image_parity(be, name: str, device='cpu') -> dict:
    """1. E, gN_r, gD, gA at rel_inf < 1e-4 against fp64; no NaN or Inf anywhere; invalid pixels are exact zeros in E, n_d and gN_r; the valid mask (read
    off the returned normals) is the reference's at every pixel."""
    c, ref = image_case(name), image_reference(name)
    got = run_image(be, c['map'], c['gE'], c['size'], c['intrinsics'], c['min_alpha'], device)
    assert all(np.isfinite(got[k]).all() for k in ('E', 'normals', 'gM')), name
    errs = image_errors(got, ref)
    print(f'normal consistency {name} on {device}: valid share {ref["share"]:.3f}, rel_inf vs fp64 {errs}')
    valid = (got['normals'] != 0).any(axis=0)
    assert np.array_equal(valid, ref['valid']), (name, int((valid != ref['valid']).sum()))
    assert not got['E'][~valid].any() and not got['gN'][:, ~valid].any(), name
    assert helpers.rel_inf(got['normals'], ref['normals']) < TOL, name
    if c['special'] == 'hole':
        assert not got['E'][10:21, 20:41].any() and not got['normals'][:, 10:21, 20:41].any() and not got['gM'][:, 10:21, 20:41].any()
    if c['special'] == 'exact':
        at_threshold = c['map'][4].numpy() == np.float32(c['min_alpha'])
        assert at_threshold.mean() > 0.2 and (valid & at_threshold).any(), name          # pixels AT min_alpha count as covered
    assert max(errs.values()) < TOL, (name, errs)
    return errs


def check_degenerate_shapes(be, device='cpu') -> None:
    """2. No interior pixel: all zeros, forward and backward. 3 x 3: the one interior pixel against the reference. gE = 0: gM exactly 0."""
    intrinsics = (5.0, 5.0, 1.2, 1.4)
    for w, h in ((1, 1), (2, 5), (5, 2)):
        gen = torch.Generator().manual_seed(w * 10 + h)
        M = torch.cat([0.3 * torch.randn(3, h, w, generator=gen), 2.0 + torch.rand(1, h, w, generator=gen), 0.6 + 0.4 * torch.rand(1, h, w, generator=gen)]).contiguous()
        got = run_image(be, M, torch.ones(h, w), (w, h), intrinsics, 0.5, device)
        assert not got['E'].any() and not got['normals'].any() and not got['gM'].any(), (w, h)
    gen = torch.Generator().manual_seed(33)
    A = 0.6 + 0.4 * torch.rand(1, 3, 3, generator=gen)
    M = torch.cat([0.3 * torch.randn(3, 3, 3, generator=gen), (2.0 + 0.2 * torch.rand(1, 3, 3, generator=gen)) * A, A]).contiguous()
    gE = torch.randn(3, 3, generator=gen)
    ref = consistency_with_gradient(M, gE, intrinsics, 0.5, torch.float64)
    got = run_image(be, M, gE, (3, 3), intrinsics, 0.5, device)
    assert ref['valid'].sum() == 1 and ref['valid'][1, 1] and got['E'][1, 1] != 0
    edge = np.ones((3, 3), bool); edge[1, 1] = False
    assert not got['E'][edge].any()
    errs = image_errors(got, ref)
    assert max(errs.values()) < TOL, errs
    c = image_case('multi')
    quiet = run_image(be, c['map'], torch.zeros_like(c['gE']), c['size'], c['intrinsics'], c['min_alpha'], device)
    assert not quiet['gM'].any()


# ---- Gaussian cases -----------------------------------------------------------------------------------------------------------------------------------------
def off_axis_camera():
    """A camera off every axis: (w2c [4,4], position [3]), float32."""
    from harness.scenes import look_at_view
    v = look_at_view((1.1, -0.7, -4.0), (0.1, 0.05, 0.0), 64, 48, 50.0)
    return v.w2c, v.position


@functools.lru_cache(maxsize=None)
def gaussian_case(n: int) -> dict:
    gen = torch.Generator().manual_seed(500 + n)
    w2c, cam = off_axis_camera()
    means = torch.rand(n, 3, generator=gen) * 2.0 - 1.0
    scales, _ = torch.sort(-4.0 + 3.0 * torch.rand(n, 3, generator=gen), dim=1)
    scales[:, 0] = torch.where(scales[:, 1] - scales[:, 0] < 0.05, scales[:, 0] - 0.1, scales[:, 0])     # the two smallest at least 0.05 apart ...
    scales = torch.stack([scales[i, torch.randperm(3, generator=gen)] for i in range(n)]) if n else scales    # ... on any axis
    rotations = torch.randn(n, 4, generator=gen) * (0.5 + 1.5 * torch.rand(n, 1, generator=gen))
    for _ in range(100):
        a = rotation_of(rotations.double())[torch.arange(n), :, smallest_axis(scales)]
        v = means.double() - cam.double()[None]
        risky = (a * v).sum(dim=1).abs() < 1e-3 * v.norm(dim=1)
        if not risky.any():
            break
        rotations[risky] = torch.randn(int(risky.sum()), 4, generator=gen)
    gF = torch.randn(n, 5, generator=gen)
    c = {'n': n, 'means': means.contiguous(), 'scales': scales.contiguous(), 'rotations': rotations.contiguous(), 'w2c': w2c, 'cam': cam, 'gF': gF.contiguous()}
    check_gaussian_inputs(c)
    return c


def check_gaussian_inputs(c: dict) -> None:
    """The conditions of test 3 on the inputs: no Gaussian at risk of another argmin or another sign."""
    n = c['n']
    if n == 0:
        return
    two = torch.sort(c['scales'], dim=1).values
    assert float((two[:, 1] - two[:, 0]).min()) >= 0.05 - 1e-6
    a = rotation_of(c['rotations'].double())[torch.arange(n), :, smallest_axis(c['scales'])]
    v = c['means'].double() - c['cam'].double()[None]
    assert bool(((a * v).sum(dim=1).abs() >= 1e-3 * v.norm(dim=1)).all())
    assert float((c['rotations'].norm(dim=1) - 1.0).abs().max()) > 0.1 or n < 4             # unnormalised


GAUSSIAN_KEYS = ('features', 'grad_rotations', 'grad_means')


def features_with_gradient(c: dict, dtype) -> dict:
    means, rotations = c['means'].clone().requires_grad_(True), c['rotations'].clone().requires_grad_(True)
    scales = c['scales'].clone().requires_grad_(True)
    feats = surface_features_of(means, scales, rotations, c['w2c'], c['cam'], dtype)
    (feats * c['gF'].to(dtype)).sum().backward()
    assert scales.grad is None                                                              # the definition gives the scales no gradient
    return {'features': feats.detach().numpy(), 'grad_rotations': rotations.grad.numpy(), 'grad_means': means.grad.numpy()}


@functools.lru_cache(maxsize=None)
def gaussian_reference(n: int) -> dict:
    return features_with_gradient(gaussian_case(n), torch.float64)


def run_gaussians(be, c: dict, device='cpu', need_rotations: bool = True, need_means: bool = True) -> dict:
    means, scales, rotations, gF = (c[k].to(device) for k in ('means', 'scales', 'rotations', 'gF'))
    w2c, cam = c['w2c'].to(device), c['cam'].to(device)
    feats = be.surface_features(means, scales, rotations, w2c, cam)
    gq, gm = be.surface_features_backward(means, scales, rotations, w2c, cam, gF, need_rotations=need_rotations, need_means=need_means)
    return {'features': feats.cpu().numpy(), 'grad_rotations': None if gq is None else gq.cpu().numpy(), 'grad_means': None if gm is None else gm.cpu().numpy()}


def check_gaussian_parity(be, n: int, device='cpu') -> dict:
    """3. features, grad_rotations, grad_means at rel_inf < 1e-4 against fp64; grad_rotations . q = 0 within 1e-5 of its norm."""
    c, ref = gaussian_case(n), gaussian_reference(n)
    got = run_gaussians(be, c, device)
    errs = {k: helpers.rel_inf(got[k], ref[k]) for k in GAUSSIAN_KEYS}
    print(f'surface features N = {n} on {device}: rel_inf vs fp64 {errs}')
    assert got['features'].shape == (n, 5) and np.array_equal(got['features'][:, 4], np.ones(n, np.float32))
    assert max(errs.values()) < TOL, (n, errs)
    q, g = c['rotations'].numpy().astype(np.float64), got['grad_rotations'].astype(np.float64)
    assert (np.abs((q * g).sum(axis=1)) <= 1e-5 * np.linalg.norm(q, axis=1) * np.linalg.norm(g, axis=1)).all(), n
    return errs


def check_no_gaussians(be, device='cpu') -> None:
    """3. N = 0: empty tensors, no launch."""
    w2c, cam = off_axis_camera()
    e3, e4 = torch.empty(0, 3, device=device), torch.empty(0, 4, device=device)
    feats = be.surface_features(e3, e3, e4, w2c.to(device), cam.to(device))
    gq, gm = be.surface_features_backward(e3, e3, e4, w2c.to(device), cam.to(device), torch.empty(0, 5, device=device))
    assert feats.shape == (0, 5) and gq.shape == (0, 4) and gm.shape == (0, 3)


def check_gaussian_edges(be, device='cpu') -> None:
    """3. The edges of definition 1, each against what the rule says."""
    eye, cam = torch.eye(4), torch.tensor([0.0, 0.0, -4.0])
    eye[2, 3] = 4.0                                                       # the camera of make_s0: looks down +z from z = -4
    ident = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    feats_of = lambda means, scales, rotations, w2c=eye, c=cam: be.surface_features(
        means.to(device).contiguous(), scales.to(device).contiguous(), rotations.to(device).contiguous(), w2c.to(device), c.to(device)).cpu()
    # exact ties: the lowest index
    a, b = -3.0, -2.0
    ties = torch.tensor([[a, a, b], [b, a, a], [a, b, a], [a, a, a], [b, b, a]])
    assert smallest_axis(ties).tolist() == [0, 1, 0, 0, 2]
    means = torch.tensor([[0.3, -0.2, 0.5]]).repeat(5, 1)
    q = torch.tensor([[0.9, 0.1, -0.3, 0.2]]).repeat(5, 1)
    got = feats_of(means, ties, q)
    R = rotation_of(q.double())[0]
    for row, k in enumerate([0, 1, 0, 0, 2]):
        col = R[:, k]
        s = -1.0 if float(col @ (means[0].double() - cam.double())) > 0 else 1.0
        assert helpers.rel_inf(got[row, :3].numpy(), (s * col).numpy()) < 1e-6, row      # w2c's rotation is the identity
    # a . v exactly 0 does not flip: a = +x, v = (0, 0.5, 5)
    flat = feats_of(torch.tensor([[0.0, 0.5, 1.0]]), torch.tensor([[-3.0, -1.0, -1.0]]), ident)
    assert flat[0].tolist() == [1.0, 0.0, 0.0, 5.0, 1.0]
    # ... and a hair on either side does what the rule says: towards the camera (v.x > 0: a . v > 0, flipped)
    assert feats_of(torch.tensor([[0.25, 0.5, 1.0]]), torch.tensor([[-3.0, -1.0, -1.0]]), ident)[0, 0] == -1.0
    assert feats_of(torch.tensor([[-0.25, 0.5, 1.0]]), torch.tensor([[-3.0, -1.0, -1.0]]), ident)[0, 0] == 1.0
    # behind the camera: still the rule's answer, z negative
    w2c, c = off_axis_camera()
    behind = {'n': 1, 'means': torch.tensor([[1.3, -0.9, -6.0]]), 'scales': torch.tensor([[-1.0, -3.0, -2.0]]), 'rotations': torch.tensor([[0.3, -0.8, 0.1, 0.6]]),
              'w2c': w2c, 'cam': c, 'gF': torch.ones(1, 5)}
    ref = features_with_gradient(behind, torch.float64)
    got = run_gaussians(be, behind, device)
    assert ref['features'][0, 3] < 0 and all(helpers.rel_inf(got[k], ref[k]) < TOL for k in GAUSSIAN_KEYS)
    # a quaternion seven times as long: the same features
    c257 = gaussian_case(257)
    longer = dict(c257, rotations=(c257['rotations'] * 7.0).contiguous())
    assert helpers.rel_inf(run_gaussians(be, longer, device)['features'], run_gaussians(be, c257, device)['features']) < 1e-6


# ---- 4. reproducibility, requested gradients, stale memory: the C entry points with the caller's buffers ------------------------------------------------
def _raw_image(lib, c: dict, device, E, normals, gM, min_alpha=None, size=None, intrinsics=None, M='map', gE='gE') -> tuple:
    P = lambda t: None if t is None else t.data_ptr()
    (w, h), k = (c['size'] if size is None else size), (c['intrinsics'] if intrinsics is None else intrinsics)
    ma = c['min_alpha'] if min_alpha is None else min_alpha
    M = c[M] if isinstance(M, str) else M
    gE = c[gE] if isinstance(gE, str) else gE
    return (lib.fgs_normal_consistency(P(M), w, h, *k, ma, P(E), P(normals), None),
            lib.fgs_normal_consistency_backward(P(M), P(gE), w, h, *k, ma, P(gM), None))


def check_reproducible_and_complete(be, device='cpu') -> None:
    """4. Two runs of each backward pass are bit-identical; a gradient that is not requested leaves the other bit-identical (and its buffer alone);
    outputs that arrive full of NaN are overwritten in full."""
    lib = be.lib
    nan = lambda *shape: torch.full(shape, float('nan'), device=device)
    for name in ('multi', 'hole'):
        c = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in image_case(name).items()}
        w, h = c['size']
        runs = []
        for _ in range(2):
            E, normals, gM = nan(h, w), nan(3, h, w), nan(5, h, w)
            assert _raw_image(lib, c, device, E, normals, gM) == (0, 0), lib.fgs_last_error()
            assert bool(torch.isfinite(E).all()) and bool(torch.isfinite(normals).all()) and bool(torch.isfinite(gM).all()), name
            runs.append((E, normals, gM))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), name
        E2 = nan(h, w)
        assert lib.fgs_normal_consistency(c['map'].data_ptr(), w, h, *c['intrinsics'], c['min_alpha'], E2.data_ptr(), None, None) == 0
        assert torch.equal(E2, runs[0][0]), name                                         # without the normals: the same E
    for n in (65, 257):
        c = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in gaussian_case(n).items()}
        P = lambda t: t.data_ptr()
        back = lambda need_q, need_m, gq, gm: lib.fgs_surface_features_backward(P(c['means']), P(c['scales']), P(c['rotations']), n, P(c['w2c']), P(c['cam']),
                                                                                 P(c['gF']), need_q, need_m, P(gq), P(gm), None)
        feats = nan(n, 5)
        assert lib.fgs_surface_features(P(c['means']), P(c['scales']), P(c['rotations']), n, P(c['w2c']), P(c['cam']), P(feats), None) == 0
        assert bool(torch.isfinite(feats).all())
        full = [(nan(n, 4), nan(n, 3)) for _ in range(2)]
        for gq, gm in full:
            assert back(1, 1, gq, gm) == 0 and bool(torch.isfinite(gq).all()) and bool(torch.isfinite(gm).all())
        assert torch.equal(full[0][0], full[1][0]) and torch.equal(full[0][1], full[1][1])
        gq, gm = nan(n, 4), nan(n, 3)
        assert back(1, 0, gq, gm) == 0 and torch.equal(gq, full[0][0]) and bool(torch.isnan(gm).all())
        gq, gm = nan(n, 4), nan(n, 3)
        assert back(0, 1, gq, gm) == 0 and torch.equal(gm, full[0][1]) and bool(torch.isnan(gq).all())
        assert lib.fgs_surface_features_backward(P(c['means']), P(c['scales']), P(c['rotations']), n, P(c['w2c']), P(c['cam']), P(c['gF']), 0, 0, None, None, None) == 0
        only_q, none_m = be.surface_features_backward(c['means'], c['scales'], c['rotations'], c['w2c'], c['cam'], c['gF'], need_means=False)
        assert none_m is None and torch.equal(only_q, full[0][0])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(be, device='cpu') -> None:
    """5. Every refusal of the four entry points: status -1, a text, the outputs untouched; the ABI version stays 3; the backend's own checks."""
    import pytest
    lib = be.lib
    err = lambda: lib.fgs_last_error().decode()
    c = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in image_case('small').items()}
    (w, h), k = c['size'], c['intrinsics']
    E, normals, gM = (torch.full(s, 7.0, device=device) for s in ((h, w), (3, h, w), (5, h, w)))
    P = lambda t: t.data_ptr()
    fwd = lambda M=P(c['map']), w=w, h=h, k=k, ma=0.5, E_=P(E): lib.fgs_normal_consistency(M, w, h, *k, ma, E_, P(normals), None)
    bwd = lambda M=P(c['map']), g=P(c['gE']), w=w, h=h, k=k, ma=0.5, out=P(gM): lib.fgs_normal_consistency_backward(M, g, w, h, *k, ma, out, None)
    assert fwd(M=None) == -1 and 'NULL' in err() and fwd(E_=None) == -1 and 'NULL' in err()
    assert bwd(M=None) == -1 and 'NULL' in err() and bwd(g=None) == -1 and 'NULL' in err() and bwd(out=None) == -1 and 'NULL' in err()
    for call in (fwd, bwd):
        assert call(w=0) == -1 and 'image size' in err() and call(h=-2) == -1 and 'image size' in err()
        assert call(k=(0.0, k[1], k[2], k[3])) == -1 and 'focal' in err() and call(k=(k[0], -3.0, k[2], k[3])) == -1 and 'focal' in err()
        assert call(k=(float('nan'), k[1], k[2], k[3])) == -1 and 'focal' in err()
        for bad in (0.0, -0.1, 1.5, float('nan')):
            assert call(ma=bad) == -1 and 'min_alpha' in err(), bad
    assert bool((E == 7.0).all()) and bool((normals == 7.0).all()) and bool((gM == 7.0).all())      # none of the refused calls wrote anything
    assert fwd(ma=1.0) == 0 and bwd(ma=1.0) == 0 and not bool((E == 7.0).any()) and not bool((gM == 7.0).any())      # (0, 1]: 1 itself is allowed
    g = {kk: (v.to(device) if isinstance(v, torch.Tensor) else v) for kk, v in gaussian_case(65).items()}
    n = 65
    feats, gq, gm = (torch.full(s, 7.0, device=device) for s in ((n, 5), (n, 4), (n, 3)))
    sf = lambda means=P(g['means']), scales=P(g['scales']), rot=P(g['rotations']), n=n, w2c=P(g['w2c']), cam=P(g['cam']), out=P(feats): \
        lib.fgs_surface_features(means, scales, rot, n, w2c, cam, out, None)
    sb = lambda means=P(g['means']), rot=P(g['rotations']), n=n, w2c=P(g['w2c']), gF=P(g['gF']), nq=1, nm=1, oq=P(gq), om=P(gm): \
        lib.fgs_surface_features_backward(means, P(g['scales']), rot, n, w2c, P(g['cam']), gF, nq, nm, oq, om, None)
    assert sf(n=-1) == -1 and 'negative' in err() and sb(n=-5) == -1 and 'negative' in err()
    for call in (sf, sb):
        assert call(means=None) == -1 and 'NULL' in err() and call(rot=None) == -1 and 'NULL' in err() and call(w2c=None) == -1 and 'NULL' in err()
        assert call(rot=P(g['rotations']) + 4) == -1 and '16-byte' in err()
    assert sf(scales=None) == -1 and sf(cam=None) == -1 and sf(out=None) == -1 and 'NULL features' in err()
    assert sb(gF=None) == -1 and 'NULL grad_features' in err()
    assert sb(oq=None) == -1 and 'need_rotations' in err() and sb(om=None) == -1 and 'need_means' in err()
    assert bool((feats == 7.0).all()) and bool((gq == 7.0).all()) and bool((gm == 7.0).all())       # none of the refused calls wrote anything
    assert sb(oq=None, nq=0) == 0 and sb(om=None, nm=0) == 0                              # not asked for: may be NULL
    assert sf(n=0, means=None, scales=None, rot=None, out=None) == 0 and sb(n=0, means=None, rot=None, gF=None, oq=None, om=None) == 0
    assert lib.fgs_abi_version() == 3
    # the backend's checks: dtype, shape, device, contiguity
    RS = settings_for(c['size'], k, device)
    with pytest.raises(RuntimeError, match='contiguous float32'):
        be.normal_consistency(c['map'].double(), RS)
    with pytest.raises(RuntimeError, match=r'\[5, H, W\]'):
        be.normal_consistency(c['map'][:4].contiguous(), RS)
    with pytest.raises(RuntimeError, match=r'\[5, H, W\]'):
        be.normal_consistency(c['map'], settings_for((w + 1, h), k, device))
    with pytest.raises(RuntimeError, match='contiguous float32'):
        be.normal_consistency(c['map'].transpose(1, 2), settings_for((h, w), k, device))
    with pytest.raises(RuntimeError, match=r'\[H, W\]'):
        be.normal_consistency_backward(c['map'], c['gE'][:-1].contiguous(), RS)
    with pytest.raises(RuntimeError, match='min_alpha'):
        be.normal_consistency(c['map'], RS, min_alpha=0.0)
    with pytest.raises(RuntimeError, match=r'\[N,3\], \[N,3\], \[N,4\]'):
        be.surface_features(g['means'], g['scales'], g['rotations'][:, :3].contiguous(), g['w2c'], g['cam'])
    with pytest.raises(RuntimeError, match='contiguous float32'):
        be.surface_features(g['means'].double(), g['scales'], g['rotations'], g['w2c'], g['cam'])
    with pytest.raises(RuntimeError, match=r'\[N,5\]'):
        be.surface_features_backward(g['means'], g['scales'], g['rotations'], g['w2c'], g['cam'], g['gF'][:, :4].contiguous())
    with pytest.raises(RuntimeError, match='w2c must be'):
        be.surface_features(g['means'], g['scales'], g['rotations'], g['w2c'][:2], g['cam'])
    if device != 'cpu':
        with pytest.raises(RuntimeError, match='contiguous float32'):
            be.surface_features(g['means'], g['scales'].cpu(), g['rotations'], g['w2c'], g['cam'])


# ---- 6. the public operators, composed with the feature render ----------------------------------------------------------------------------------------------
def small_scene(device='cpu', n: int = 300, size=(52, 39)):
    """make_s0(n) seen by its own camera at `size` = (W, H) (focal 52: within the conditioning limit), as the bilagrid tests use it."""
    from harness import trainer as T
    from harness.scenes import View, make_s0
    params, view = make_s0(n=n)
    f = view.focal_x * size[0] / view.width
    view = View(view.w2c, view.position, size[0], size[1], f, f, size[0] / 2.0 + 1.3, size[1] / 2.0 - 0.8, view.near_plane, view.far_plane, view.background_color)
    return T, params, view.to(torch.device(device))


def check_operators(B, be, device='cpu', tol: float = OPERATOR_TOL_SIM, min_alpha: float = 0.3) -> dict:
    """6. gaussian_surface_features -> diff_rasterize_features -> normal_consistency(...).mean(): the gradients of all Gaussian parameters equal those of
    the same graph with the two new operators replaced by their fp32 torch restatements (the same diff_rasterize_features in the middle)."""
    T, params, view = small_scene(device)
    RS = T.extract_settings(view, 16, view.background_color)
    intrinsics = (view.focal_x, view.focal_y, view.center_x, view.center_y)
    none = torch.empty(0)

    def gradients(features_fn, consistency_fn):
        leaves = [params[k].to(device).clone().requires_grad_(True) for k in helpers.NAMES]
        feats = features_fn(leaves[0], leaves[1], leaves[2])
        image, surface_map = B.diff_rasterize_features(*leaves, none, RS, feats)
        E = consistency_fn(surface_map)
        grads = torch.autograd.grad(E.mean(), leaves, allow_unused=True)
        return E.detach(), surface_map.detach(), [torch.zeros_like(p) if g is None else g for p, g in zip(leaves, grads)]

    E_op, map_op, g_op = gradients(lambda m, s, q: B.gaussian_surface_features(m, s, q, view.w2c, view.position),
                                   lambda M: B.normal_consistency(M, RS, min_alpha=min_alpha))
    E_re, map_re, g_re = gradients(lambda m, s, q: surface_features_of(m, s, q, view.w2c, view.position, torch.float32),
                                   lambda M: consistency_of(M, intrinsics, min_alpha, torch.float32)[0])
    share = float((E_op != 0).float().mean())
    assert E_op.shape == (view.height, view.width) and share > 0.1, share               # the term reaches a good part of the image
    errs = {'E': helpers.rel_inf(E_op.cpu().numpy(), E_re.cpu().numpy()), 'map': helpers.rel_inf(map_op.cpu().numpy(), map_re.cpu().numpy())}
    for k, a, b in zip(helpers.GRAD_KEYS, g_op, g_re):
        errs[k] = helpers.rel_inf(a.cpu().numpy(), b.cpu().numpy())
    print(f'normal consistency operators on {device}: share of pixels with E != 0 {share:.3f}, rel_inf vs the fp32 restatement {errs}')
    assert float(g_op[0].abs().max()) > 0 and float(g_op[1].abs().max()) > 0 and float(g_op[2].abs().max()) > 0 and float(g_op[3].abs().max()) > 0
    assert not g_op[4].any() and not g_op[5].any()                                       # the image is not part of the loss: the colours get nothing
    assert max(errs.values()) < tol, errs

    # no_grad: forward only; return_normals: unit normals where E is defined, no gradient through them; an input without requires_grad gets None
    with torch.no_grad():
        quiet = B.normal_consistency(map_op, RS, min_alpha=min_alpha)
    assert not quiet.requires_grad and torch.equal(quiet, E_op)
    leaf = map_op.clone().requires_grad_(True)
    E, normals = B.normal_consistency(leaf, RS, min_alpha=min_alpha, return_normals=True)
    assert torch.equal(E.detach(), E_op) and not normals.requires_grad and normals.shape == (3, view.height, view.width)
    length = normals.norm(dim=0)
    assert bool(((length - 1).abs() < 1e-5)[E_op != 0].all()) and not normals[:, length == 0].any()           # unit where defined, zeros elsewhere
    (gm,) = torch.autograd.grad(E.sum(), [leaf])
    assert torch.equal(gm, be.normal_consistency_backward(map_op, torch.ones_like(E_op), RS, min_alpha))
    means, scales, rotations = (params[k].to(device) for k in ('means', 'scales', 'rotations'))
    calls = []
    spy = type(be).surface_features_backward
    try:                                                                                  # ... and it costs nothing: the backend is asked for one gradient
        type(be).surface_features_backward = lambda self, *a, **k: calls.append(k) or spy(self, *a, **k)
        q = rotations.clone().requires_grad_(True)
        feats = B.gaussian_surface_features(means, scales, q, view.w2c, view.position)
        torch.autograd.grad(feats.sum(), [q])
    finally:
        type(be).surface_features_backward = spy
    assert calls == [{'need_rotations': True, 'need_means': False}]
    return errs


# ---- 7. the harness -----------------------------------------------------------------------------------------------------------------------------------------
def check_training_iteration(be, device='cpu', exact: bool = True, weight: float = 0.05, min_alpha: float = 0.3) -> None:
    """7. training_iteration(normal_weight=w) equals the step composed by hand from the operators; normal_weight=0 is bit-identical to the plain step;
    the combinations that are different renders raise."""
    import pytest
    import FasterGSCudaBackend as B
    T, params, view = small_scene(device)
    dev = torch.device(device)
    with torch.no_grad():
        target = T.render_image_training(T.Gaussians(params, dev), view, False, view.background_color).clone()
    gen = torch.Generator().manual_seed(8)
    start = {k: (v + 0.01 * torch.randn(v.shape, generator=gen)) for k, v in params.items()}

    def fresh():
        g = T.Gaussians({k: v.clone() for k, v in start.items()}, dev)
        g.training_setup(training_cameras_extent=4.0)
        return g
    ga = fresh()
    loss_a = T.training_iteration(ga, view, target, 0, normal_weight=weight, normal_min_alpha=min_alpha)
    gb = fresh()
    gb.update_learning_rate(1)
    RS = T.extract_settings(view, gb.active_sh_bases, view.background_color)
    feats = B.gaussian_surface_features(gb.means, gb.scales, gb.rotations, view.w2c, view.position)
    image, surface_map = B.diff_rasterize_features(*gb.tensors(), gb.densification_info, RS, feats)
    E = B.normal_consistency(surface_map, RS, min_alpha=min_alpha)
    loss_b = T.photometric_loss(image, target) + weight * E.mean()
    loss_b.backward()
    gb.optimizer.step()
    gb.optimizer.zero_grad()
    same = torch.equal if exact else (lambda a, b: helpers.rel_inf(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < RUN_TO_RUN)
    assert float(E.detach().mean()) > 0 and same(loss_a, loss_b.detach())
    for k in T.PARAM_ORDER:
        assert same(getattr(ga, k), getattr(gb, k)), k
    assert same(ga.densification_info, gb.densification_info)
    # normal_weight = 0: the plain step, bit for bit (the same kernels in the same order; on the device K11's float atomics decide the last bits)
    gc, gd = fresh(), fresh()
    loss_c = T.training_iteration(gc, view, target, 0, normal_weight=0.0)
    loss_d = T.training_iteration(gd, view, target, 0)
    assert same(loss_c, loss_d) and all(same(getattr(gc, k), getattr(gd, k)) for k in T.PARAM_ORDER)
    assert not same(ga.rotations, gd.rotations) or not exact                              # ... and the term did move the step
    for kw in ({'distortion_weight': 0.1}, {'absgrad': True}, {'depth_target': torch.ones(view.height, view.width, device=dev), 'depth_weight': 0.5}):
        with pytest.raises(ValueError, match='normal-consistency term does not combine'):
            T.training_iteration(fresh(), view, target, 0, normal_weight=weight, **kw)


# ---- 8. it regularises --------------------------------------------------------------------------------------------------------------------------------------
REGULARISE_STEPS, REGULARISE_LR = 8, 0.03       # chosen on the simulation: the factor reached there is in FIGURES['regularises']


def disk_patch(side: int = 10, max_degrees: float = 20.0, seed: int = 5) -> dict:
    """A planar patch of side x side flat disks (log-scale ratios 0, 0, -2.3) in the plane z = 0 facing the camera of make_s0, every rotation turned by up
    to max_degrees about a random axis."""
    gen = torch.Generator().manual_seed(seed)
    n = side * side
    line = torch.linspace(-0.9, 0.9, side)
    gy, gx = torch.meshgrid(line, line, indexing='ij')
    means = torch.stack([gx.reshape(-1), gy.reshape(-1), torch.zeros(n)], dim=1)
    scales = torch.tensor([0.0, 0.0, -2.3]).repeat(n, 1) + float(np.log(0.12))
    axis = torch.randn(n, 3, generator=gen)
    axis = axis / axis.norm(dim=1, keepdim=True)
    half = 0.5 * np.deg2rad(max_degrees) * torch.rand(n, 1, generator=gen)
    rotations = torch.cat([torch.cos(half), torch.sin(half) * axis], dim=1)
    return {'means': means, 'scales': scales, 'rotations': rotations.contiguous(), 'opacities': torch.full((n, 1), 2.2),
            'sh_coefficients_0': 0.3 * torch.randn(n, 1, 3, generator=gen), 'sh_coefficients_rest': torch.zeros(n, 15, 3)}


def check_regularises(device='cpu', steps: int = REGULARISE_STEPS, lr: float = REGULARISE_LR) -> tuple:
    """8. Everything frozen but the rotations, the loss E.mean() alone: it falls below half of its start value."""
    T, _, view = small_scene(device)
    g = T.Gaussians(disk_patch(), torch.device(device))
    opt = torch.optim.Adam([g.rotations], lr=lr)
    before = {k: getattr(g, k).detach().clone() for k in T.PARAM_ORDER}
    losses = []
    for _ in range(steps + 1):
        _, E = T.render_image_training_normals(g, view, False, view.background_color)
        loss = E.mean()
        losses.append(float(loss.detach()))
        if len(losses) > steps:
            break
        for p in g.parameters():
            p.grad = None
        loss.backward()
        opt.step()
    print(f'normal consistency on {device}: E.mean() {losses[0]:.6f} -> {losses[-1]:.6f} in {steps} steps (factor {losses[-1] / losses[0]:.3f})')
    assert all(np.isfinite(losses)) and losses[0] > 0
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    assert all(torch.equal(getattr(g, k), before[k]) for k in T.PARAM_ORDER if k != 'rotations')
    return losses[0], losses[-1]
