"""TSDF fusion and mesh extraction (csrc/tsdf.hip): fp64 numpy restatements of the definitions in include/fgs_hip.h, the cases and the bars. Shared by
tests/test_tsdf.py (CPU simulation of the product library) and tests/test_gpu_tsdf.py (MI355X): every check takes a Backend and a device.

Bars and where they come from
  integration   weights equal; tsdf and colour within 1e-5 absolute of the fp64 model outside the points the model flags (a discrete decision within an
                fp32 rounding of flipping: u or v within 1e-3 px of an integer, z within 1e-5 of near, sdf within 1e-4 trunc of -trunc); the flagged share
                of the case below is asserted < 2 % (1.35 % on the model alone)
  extraction    vertex count and canonical face set equal to the restatement; positions within 1e-5 voxel_size; signed volume within 1e-4 relative
  end to end    median distance of the mesh vertices of a sphere of opaque disks from that sphere < 1 voxel. Nothing predicts this number but a run:
                END_TO_END_MEASURED, recorded below beside the bar (the median depth of a pixel is the view-space z of a disk's CENTRE, and the disks
                are about a voxel wide: that, not the fusion, is the error)
"""
from __future__ import annotations

import ctypes as C
import functools
import itertools
import math

import numpy as np
import torch

import helpers

# ------------------------------------------------------------------ integration: model -------------------------------------------------------------------
INT_DIMS = (24, 20, 16)            # nx, ny, nz: a multiple of no tile size
INT_SIZE = (37, 29)                # width, height
INT_VOXEL, INT_ORIGIN, INT_TRUNC = 0.1, (-1.15, -0.95, -0.75), 0.3
INT_SCALARS = dict(near=0.2, depth_max=6.0, min_alpha=0.5, max_weight=65536.0)
INT_EYES = ((0.3, -0.4, -3.0), (2.2, -0.5, -2.0), (-2.5, 0.6, -1.4))
INT_FOCAL = 45.0
FLAGGED_BAR = 0.02
TSDF_TOL = 1e-5
END_TO_END_BAR_VOXELS = 1.0
END_TO_END_MEASURED = 0.731        # voxels, simulation and device alike (2500 disks, six 88 x 88 views, voxel 0.08; 90th percentile 1.29)


def lattice(dims, origin, voxel):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    o32, v32 = np.asarray(origin, np.float32).astype(np.float64), float(np.float32(voxel))
    return np.stack([o32[0] + v32 * i, o32[1] + v32 * j, o32[2] + v32 * k], axis=-1)          # [nz,ny,nx,3]


def integrate_model(state, color, dims, origin, voxel, trunc, views, near, depth_max, min_alpha, max_weight):
    """fp64 restatement of fgs_tsdf_integrate. state [nz,ny,nx,2] / color [3,nz,ny,nx] or None (float64 copies are returned); views: dicts with w2c [>=3,4],
    fx, fy, cx, cy, depth [H,W], alpha [H,W] or None, color [3,H,W] or None. Returns (state, color, touched, flagged)."""
    P = lattice(dims, origin, voxel)
    s = np.array(state, np.float64)
    col = None if color is None else np.array(color, np.float64)
    touched = np.zeros(P.shape[:3], bool)
    flagged = np.zeros(P.shape[:3], bool)
    trunc, near = float(np.float32(trunc)), float(np.float32(near))
    for V in views:
        M = np.asarray(V['w2c'], np.float64)
        depth = np.asarray(V['depth'], np.float64)
        h, w = depth.shape
        c = P @ M[:3, :3].T + M[:3, 3]
        z = c[..., 2]
        flagged |= np.abs(z - near) < 1e-5
        ok = z > near
        zs = np.where(ok, z, 1.0)
        u = float(np.float32(V['fx'])) * c[..., 0] / zs + float(np.float32(V['cx']))
        v = float(np.float32(V['fy'])) * c[..., 1] / zs + float(np.float32(V['cy']))
        near_int = (np.abs(u - np.rint(u)) < 1e-3) | (np.abs(v - np.rint(v)) < 1e-3)
        px, py = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        loose = ok & (px >= -1) & (px <= w) & (py >= -1) & (py <= h)
        flagged |= loose & near_int
        ok &= (px >= 0) & (px < w) & (py >= 0) & (py < h)
        pxc, pyc = np.clip(px, 0, w - 1), np.clip(py, 0, h - 1)
        d = depth[pyc, pxc]
        ok &= (d > 0) & (d <= float(np.float32(depth_max)))
        if V.get('alpha') is not None:
            ok &= np.asarray(V['alpha'], np.float64)[pyc, pxc] >= float(np.float32(min_alpha))
        sdf = d - z
        flagged |= ok & (np.abs(sdf + trunc) < 1e-4 * trunc)
        ok &= sdf >= -trunc
        f = np.minimum(1.0, sdf / trunc)
        wgt = s[..., 1]
        w1 = wgt + 1.0
        if col is not None:
            cm = np.asarray(V['color'], np.float64)[:, pyc, pxc]
            col = np.where(ok[None], (col * wgt[None] + cm) / w1[None], col)
        s[..., 0] = np.where(ok, (s[..., 0] * wgt + f) / w1, s[..., 0])
        s[..., 1] = np.where(ok, np.minimum(w1, float(max_weight)), wgt)
        touched |= ok
    return s, col, touched, flagged


@functools.lru_cache(maxsize=None)
def integration_case():
    """Three look-at views of a sphere (radius 0.5 at the origin) in front of a plane of constant view-space depth, with holes (d = 0) and an opacity map
    that drops below min_alpha in a band of rows."""
    from harness.scenes import look_at_view
    w, h = INT_SIZE
    rng = np.random.default_rng(5)
    views = []
    for n, eye in enumerate(INT_EYES):
        view = look_at_view(eye, (0.0, 0.0, 0.0), w, h, INT_FOCAL)
        M = view.w2c.numpy().astype(np.float64)
        ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing='ij')
        ray = np.stack([(xs - view.center_x) / view.focal_x, (ys - view.center_y) / view.focal_y, np.ones_like(xs)], axis=-1)       # view space, z = 1
        centre = M[:3, 3]                                                                                                         # the world origin in view space
        a, b, c = (ray * ray).sum(-1), -2.0 * (ray @ centre), centre @ centre - 0.25
        disc = b * b - 4 * a * c
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.linalg.norm(centre) + 0.9)                        # else the plane behind it
        depth = t.astype(np.float32)
        depth[(xs.astype(int) * 7 + ys.astype(int) * 3 + n) % 11 == 0] = 0.0                                                        # holes
        alpha = np.full((h, w), 0.97, np.float32)
        alpha[10 + n:14 + n] = 0.3
        views.append(dict(view=view, w2c=view.w2c.numpy(), fx=view.focal_x, fy=view.focal_y, cx=view.center_x, cy=view.center_y, depth=depth, alpha=alpha,
                          color=rng.random((3, h, w), dtype=np.float32)))
    return views


def _settings(view, device):
    _, RS = helpers.settings_pair(view, device=device)
    return RS


def empty_volume(dims, device, color=True):
    nx, ny, nz = dims
    return (torch.zeros((nz, ny, nx, 2), dtype=torch.float32, device=device), torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=device) if color else None)


def run_integrate(be, device, tw, col, views, with_alpha=True, **over):
    sc = dict(INT_SCALARS, **over)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    be.tsdf_integrate(tw, col, INT_ORIGIN, INT_VOXEL, INT_TRUNC, [_settings(V['view'], device) for V in views], [t(V['depth']) for V in views],
                      [t(V['alpha']) for V in views] if with_alpha else None, [t(V['color']) for V in views] if col is not None else None, **sc)


@functools.lru_cache(maxsize=None)
def integration_reference():
    """The fp64 model over the three views from an empty volume, computed once: (state, color, touched, flagged)."""
    nx, ny, nz = INT_DIMS
    return integrate_model(np.zeros((nz, ny, nx, 2)), np.zeros((3, nz, ny, nx)), INT_DIMS, INT_ORIGIN, INT_VOXEL, INT_TRUNC, integration_case(), **INT_SCALARS)


def check_integration_against_model(be, device='cpu'):
    """1. weights equal, tsdf and colour within 1e-5 outside the flagged points; the flagged share < 2 %."""
    views = integration_case()
    ref_s, ref_c, touched, flagged = integration_reference()
    share = float(flagged.mean())
    print(f'flagged share {share:.4f}, touched {float(touched.mean()):.3f}')
    assert share < FLAGGED_BAR, share
    assert 0.2 < touched.mean() < 0.95                       # both kinds of point exist
    tw, col = empty_volume(INT_DIMS, device)
    run_integrate(be, device, tw, col, views)
    got_s, got_c = tw.cpu().numpy().astype(np.float64), col.cpu().numpy().astype(np.float64)
    keep = ~flagged
    err_t = float(np.abs(got_s[..., 0] - ref_s[..., 0])[keep].max())
    err_c = float(np.abs(got_c - ref_c)[:, keep].max())
    print(f'tsdf max abs err {err_t:.2e}, colour {err_c:.2e}')
    assert np.array_equal(got_s[..., 1][keep], ref_s[..., 1][keep])
    assert err_t < TSDF_TOL and err_c < TSDF_TOL, (err_t, err_c)
    # without the opacity maps the band is integrated too: more weight, same model
    ref2 = integrate_model(np.zeros_like(ref_s), None, INT_DIMS, INT_ORIGIN, INT_VOXEL, INT_TRUNC, [dict(V, alpha=None) for V in views], **INT_SCALARS)
    tw2, _ = empty_volume(INT_DIMS, device, color=False)
    run_integrate(be, device, tw2, None, views, with_alpha=False)
    got2 = tw2.cpu().numpy().astype(np.float64)
    keep2 = ~ref2[3]
    assert ref2[0][..., 1].sum() > ref_s[..., 1].sum()
    assert np.array_equal(got2[..., 1][keep2], ref2[0][..., 1][keep2]) and np.abs(got2[..., 0] - ref2[0][..., 0])[keep2].max() < TSDF_TOL


def check_batched_equals_single(be, device='cpu'):
    """2. V = 3 in one call, V = 8 (views repeated) in one call, and the same views one call each: bit-identical volumes."""
    views = integration_case()
    for batch in (list(views), [views[k % 3] for k in range(8)]):
        a_tw, a_c = empty_volume(INT_DIMS, device)
        run_integrate(be, device, a_tw, a_c, batch)
        b_tw, b_c = empty_volume(INT_DIMS, device)
        for V in batch:
            run_integrate(be, device, b_tw, b_c, [V])
        assert torch.equal(a_tw.view(torch.int32), b_tw.view(torch.int32)) and torch.equal(a_c.view(torch.int32), b_c.view(torch.int32)), len(batch)
        assert float(a_tw[..., 1].max()) == len(batch)


def check_untouched_and_cap(be, device='cpu'):
    """3. untouched points keep their bytes (zeros, and a sentinel pattern); max_weight = 2 holds after four integrations; integrating twice doubles the
    weight and leaves tsdf within 1e-6."""
    views = integration_case()
    _, _, touched, flagged = integration_reference()
    still = torch.from_numpy(~touched & ~flagged).to(device)
    assert int(still.sum()) > 100
    tw, col = empty_volume(INT_DIMS, device)
    run_integrate(be, device, tw, col, views)
    assert int(tw.view(torch.int32)[still].abs().max()) == 0 and int(col.view(torch.int32)[:, still].abs().max()) == 0
    once = tw.clone()
    # a sentinel where no view reaches: NaN payloads and denormals, which only an untouched load/store-free path preserves
    s_tw, s_col = empty_volume(INT_DIMS, device)
    pattern = torch.arange(s_tw.numel(), dtype=torch.int32, device=device).view(s_tw.shape) * 2654435 + 0x7fc00001
    s_tw.view(torch.int32)[still] = pattern[still]
    s_col.view(torch.int32)[:, still] = pattern[..., 0][still]
    before_tw, before_col = s_tw.view(torch.int32).clone(), s_col.view(torch.int32).clone()
    run_integrate(be, device, s_tw, s_col, views)
    assert torch.equal(s_tw.view(torch.int32)[still], before_tw[still]) and torch.equal(s_col.view(torch.int32)[:, still], before_col[:, still])
    hit = torch.from_numpy(touched & ~flagged).to(device)
    assert torch.equal(s_tw.view(torch.int32)[hit], once.view(torch.int32)[hit])
    # twice
    run_integrate(be, device, tw, col, views)
    assert torch.equal(tw[..., 1], 2 * once[..., 1])
    assert float((tw[..., 0] - once[..., 0]).abs().max()) < 1e-6
    # the cap
    c_tw, _ = empty_volume(INT_DIMS, device, color=False)
    for _ in range(4):
        run_integrate(be, device, c_tw, None, [views[0]], max_weight=2.0)
    w = c_tw[..., 1]
    assert float(w.max()) == 2.0 and set(w.unique().tolist()) == {0.0, 2.0}


def check_pixel_convention(be, device='cpu'):
    """4. the pixel of a lattice point is the pixel in which the rasterizer draws a Gaussian centred there."""
    from harness.scenes import look_at_view
    nx, ny, nz = INT_DIMS
    view = look_at_view((0.37, -0.21, -3.0), (0.05, 0.02, 0.0), 37, 29, 57.0)
    M = view.w2c.numpy().astype(np.float64)
    P = lattice(INT_DIMS, INT_ORIGIN, INT_VOXEL)
    for idx in itertools.product(range(6, 10), range(8, 12), range(9, 13)):        # k, j, i: the first lattice point that projects well inside a pixel
        mean = P[idx]
        c = M[:3, :3] @ mean + M[:3, 3]
        u, v = view.focal_x * c[0] / c[2] + view.center_x, view.focal_y * c[1] / c[2] + view.center_y
        if min(u % 1, 1 - u % 1, v % 1, 1 - v % 1) > 0.25:
            break
    assert min(u % 1, 1 - u % 1, v % 1, 1 - v % 1) > 0.25, (u, v)                 # the maximum of alpha is unambiguous
    params = {'means': torch.tensor(mean[None], dtype=torch.float32), 'scales': torch.full((1, 3), math.log(0.004)), 'rotations': torch.tensor([[1.0, 0, 0, 0]]),
              'opacities': torch.full((1, 1), 6.0), 'sh_coefficients_0': torch.ones(1, 1, 3), 'sh_coefficients_rest': torch.zeros(1, 15, 3)}
    RS = _settings(view, device)
    out = be.inference_aux(*[params[k].to(device) for k in helpers.NAMES], RS, True, True, True, False, False)
    alpha = out['alpha'].cpu().numpy()
    py, px = np.unravel_index(int(alpha.argmax()), alpha.shape)
    assert alpha[py, px] > 0.5 and (px, py) == (math.floor(u), math.floor(v)), (px, py, u, v)
    for dx, dy, expect in ((0, 0, 1.0), (1, 0, 0.0), (-1, 0, 0.0), (0, 1, 0.0), (0, -1, 0.0)):
        depth = torch.zeros((29, 37), dtype=torch.float32)
        depth[py + dy, px + dx] = float(c[2])
        tw, _ = empty_volume(INT_DIMS, device, color=False)
        be.tsdf_integrate(tw, None, INT_ORIGIN, INT_VOXEL, INT_TRUNC, [RS], [depth.to(device)], None, None, **INT_SCALARS)
        assert float(tw[idx][1]) == expect, (dx, dy)
        if expect:
            assert abs(float(tw[idx][0])) < 1e-5


# ------------------------------------------------------------------ extraction: model --------------------------------------------------------------------
def _tets():
    out = []
    for perm in itertools.permutations(range(3)):            # lexicographic
        v1 = 1 << perm[0]
        out.append((0, v1, v1 | (1 << perm[1]), 7))
    return out


TETS = _tets()
_CORNER = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)], np.float64)


def mesh_model(state, dims, origin, voxel, iso=0.0, min_weight=1.0, color=None):
    """fp64 restatement of the marching-tetrahedra definition. state [nz,ny,nx,2]. Orientation is decided here on the GEOMETRY (the normal of the triangle
    through the edge midpoints against the direction from the inside corners to the outside corners), not by the kernel's determinant rule.
    Returns dict(vertices [Nv,3], faces [Nf,3], owner [Nv] linear lattice index, type [Nv] 1..7, colors or None)."""
    nx, ny, nz = dims
    f = np.asarray(state, np.float64)[..., 0].reshape(-1)
    valid = (np.asarray(state, np.float64)[..., 1] >= float(np.float32(min_weight))).reshape(-1)
    iso = float(np.float32(iso))
    inside = f < iso
    n = nx * ny * nz
    lin = np.arange(n)
    x, y, z = lin % nx, (lin // nx) % ny, lin // (nx * ny)
    step = lambda d: (d & 1) + ((d >> 1) & 1) * nx + (d >> 2) * nx * ny
    there = lambda d: ((x + (d & 1)) < nx) & ((y + ((d >> 1) & 1)) < ny) & ((z + (d >> 2)) < nz)
    mask = np.zeros(n, np.int64)
    for d in range(1, 8):
        ok = there(d)
        b = np.where(ok, lin + step(d), 0)
        mask |= (ok & valid & valid[b] & (inside != inside[b])).astype(np.int64) << (d - 1)
    count = np.array([bin(m).count('1') for m in range(128)])[mask]
    vbase = np.cumsum(count) - count
    owners = np.nonzero(mask)[0]
    o32, v32 = np.asarray(origin, np.float32).astype(np.float64), float(np.float32(voxel))
    col = None if color is None else np.asarray(color, np.float64).reshape(3, -1)
    verts, vown, vtyp, vcol = [], [], [], []
    for a in owners:
        for d in range(1, 8):
            if (mask[a] >> (d - 1)) & 1:
                b = a + step(d)
                t = (iso - f[a]) / (f[b] - f[a])
                verts.append(o32 + v32 * np.array([x[a], y[a], z[a]]) + _CORNER[d] * v32 * t)
                vown.append(a); vtyp.append(d)
                if col is not None:
                    vcol.append(col[:, a] + (col[:, b] - col[:, a]) * t)
    vid = lambda a, d: int(vbase[a] + bin(int(mask[a]) & ((1 << (d - 1)) - 1)).count('1'))

    cube_ok = there(7).copy()
    mixed_lo, mixed_hi = np.ones(n, bool), np.zeros(n, bool)
    for c in range(8):
        b = np.where(there(7), lin + step(c), 0)
        cube_ok &= valid[b]
        mixed_lo &= inside[b]; mixed_hi |= inside[b]
    faces = []
    for a in np.nonzero(cube_ok & mixed_hi & ~mixed_lo)[0]:
        ins_of = [bool(inside[a + step(c)]) for c in range(8)]
        for tet in TETS:
            ins = [c for c in tet if ins_of[c]]
            outs = [c for c in tet if not ins_of[c]]
            if not ins or not outs:
                continue
            edge = lambda c0, c1: (min(c0, c1), max(c0, c1))
            if len(ins) == 2:
                (p, q), (r, s) = ins, outs
                quads = [[edge(p, r), edge(p, s), edge(q, s)], [edge(p, r), edge(q, s), edge(q, r)]]
            elif len(ins) == 1:
                quads = [[edge(ins[0], o) for o in outs]]
            else:
                quads = [[edge(outs[0], i) for i in ins]]
            away = _CORNER[outs].mean(0) - _CORNER[ins].mean(0)
            for tri in quads:
                mid = [(_CORNER[c0] + _CORNER[c1]) / 2 for c0, c1 in tri]
                normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                ids = [vid(a + step(c0), c0 ^ c1) for c0, c1 in tri]
                assert abs(normal @ away) > 1e-9
                faces.append(ids if normal @ away > 0 else [ids[0], ids[2], ids[1]])
    return dict(vertices=np.array(verts, np.float64).reshape(-1, 3), faces=np.array(faces, np.int64).reshape(-1, 3), owner=np.array(vown, np.int64),
                type=np.array(vtyp, np.int64), colors=None if col is None else np.array(vcol, np.float64).reshape(-1, 3))


def canonical(faces):
    """every triple rotated to its smallest index first, rows sorted"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(f):
        return f
    k = f.argmin(1)
    rot = np.stack([f[np.arange(len(f)), (k + s) % 3] for s in range(3)], axis=1)
    return rot[np.lexsort(rot.T[::-1])]


def edge_report(faces):
    """(closed: every directed edge once and its reverse once, number of undirected edges, boundary edges [[a,b]...] used exactly once in all)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    if not len(d):
        return True, 0, d
    key = lambda e: e[:, 0] * (int(f.max()) + 1) + e[:, 1]
    fw, counts = np.unique(key(d), return_counts=True)
    und, ucounts = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    closed = bool((counts == 1).all() and np.isin(key(d[:, ::-1]), fw).all() and (ucounts == 2).all())
    return closed, len(und), und[ucounts == 1]


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def degenerate_count(vertices, faces):
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return int((np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) == 0).sum())


MESH_VOXEL, MESH_ORIGIN = 0.03, (-0.41, -0.37, -0.45)


def _index_grid(dims):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    return np.stack([i, j, k], -1).astype(np.float64)


def field_volume(dims, f, weight=None):
    nx, ny, nz = dims
    s = np.zeros((nz, ny, nx, 2), np.float32)
    s[..., 0] = f
    s[..., 1] = 1.0 if weight is None else weight
    return s


def sphere_field(dims, centre, radius, trunc=3.0):
    return np.clip((np.linalg.norm(_index_grid(dims) - np.asarray(centre), axis=-1) - radius) / trunc, -1, 1)


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """(dims, state float32 [nz,ny,nx,2], colour float32 [3,nz,ny,nx] or None)"""
    if name == 'sphere':
        dims = (32, 28, 30)
        nx, ny, nz = dims
        col = np.random.default_rng(3).random((3, nz, ny, nx), dtype=np.float32)
        return dims, field_volume(dims, sphere_field(dims, (15.3, 13.6, 14.45), 9.3)), col
    if name == 'torus':
        dims = (34, 34, 18)
        g = _index_grid(dims) - np.array([16.4, 16.7, 8.3])
        f = np.sqrt((np.hypot(g[..., 0], g[..., 1]) - 10.2) ** 2 + g[..., 2] ** 2) - 4.1
        return dims, field_volume(dims, np.clip(f / 3.0, -1, 1)), None
    if name == 'two_spheres':
        dims = (36, 16, 16)
        return dims, field_volume(dims, np.minimum(sphere_field(dims, (8.3, 7.6, 7.4), 5.2), sphere_field(dims, (26.4, 8.2, 8.3), 5.7))), None
    if name == 'lattice_valued':
        dims = (18, 17, 16)
        g = _index_grid(dims)
        f = np.abs(g[..., 0] - 8) + np.abs(g[..., 1] - 8) + np.abs(g[..., 2] - 7) - 5.0          # integers: exact zeros on corners
        return dims, field_volume(dims, f / 16.0), None
    if name == 'half_valid':
        dims = (32, 28, 30)
        w = np.ones((30, 28, 32), np.float32)
        w[:, :, 16:] = 0.0
        return dims, field_volume(dims, sphere_field(dims, (15.3, 13.6, 14.45), 9.3), w), None
    if name == 'all_positive':
        dims = (9, 7, 5)
        return dims, field_volume(dims, np.full((5, 7, 9), 0.5)), None
    if name == 'extent_2':
        dims = (2, 2, 2)
        f = np.full((2, 2, 2), 0.4)
        f[0, 0, 0], f[1, 0, 1] = -0.7, -0.2
        return dims, field_volume(dims, f), None
    if name in ('nx_65', 'nx_129'):
        dims = (int(name[3:]), 5, 4)
        g = _index_grid(dims)
        wave = 0.9 * np.sin(0.37 * g[..., 0] + 0.5) * (g[..., 0] < dims[0] - 1)          # the last plane x = nx - 1 crosses zero in y and z: it owns vertices
        f = wave + 0.21 * (g[..., 1] - 2.2) - 0.17 * (g[..., 2] - 1.4)
        return dims, field_volume(dims, np.clip(f, -1, 1)), None
    raise KeyError(name)


def mesh_origin(name):
    """The long rows are centred on zero: the position bar, 1e-5 voxel_size = 3e-7, is three fp32 roundings of a coordinate below 2, not of one at 3.4."""
    return (-0.5 * MESH_VOXEL * mesh_case(name)[0][0] + 0.004,) + MESH_ORIGIN[1:] if name.startswith('nx_') else MESH_ORIGIN


@functools.lru_cache(maxsize=None)
def mesh_reference(name, iso=0.0):
    dims, state, col = mesh_case(name)
    return mesh_model(state, dims, mesh_origin(name), MESH_VOXEL, iso=iso, color=col)


def run_extract(be, device, name, iso=0.0):
    dims, state, col = mesh_case(name)
    tw = torch.from_numpy(state).to(device)
    c = None if col is None else torch.from_numpy(col).to(device)
    v, f, vc = be.tsdf_extract_mesh(tw, c, mesh_origin(name), MESH_VOXEL, iso=iso, min_weight=1.0)
    return v.cpu().numpy(), f.cpu().numpy(), None if vc is None else vc.cpu().numpy()


def check_against_model(be, device, name, iso=0.0):
    """vertex count and canonical face set equal; positions within 1e-5 voxel_size (colours 1e-5); returns (vertices, faces, reference)."""
    ref = mesh_reference(name, iso)
    v, f, vc = run_extract(be, device, name, iso)
    assert v.shape == ref['vertices'].shape and f.shape == ref['faces'].shape, (v.shape, f.shape, ref['vertices'].shape, ref['faces'].shape)
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert np.array_equal(canonical(f), canonical(ref['faces']))
    if len(v):
        err = float(np.abs(v - ref['vertices']).max())
        print(f'{name}: {len(v)} vertices, {len(f)} faces, position err {err / MESH_VOXEL:.2e} voxels')
        assert err < 1e-5 * MESH_VOXEL, err
        if vc is not None:
            assert float(np.abs(vc - ref['colors']).max()) < 1e-5
    return v, f, ref


def check_sphere(be, device='cpu'):
    """5."""
    v, f, ref = check_against_model(be, device, 'sphere')
    closed, n_edges, boundary = edge_report(f)
    assert closed and len(boundary) == 0
    assert len(v) - n_edges + len(f) == 2
    assert len(np.unique(f)) == len(v)                      # every vertex is used
    vol, vol_ref = signed_volume(v, f), signed_volume(ref['vertices'], ref['faces'])
    assert vol > 0 and abs(vol - vol_ref) < 1e-4 * vol_ref
    assert abs(vol / (4 / 3 * math.pi * (9.3 * MESH_VOXEL) ** 3) - 1) < 0.02          # and it IS the sphere
    # a second level set of the same field: iso is honoured
    v2, f2, _ = check_against_model(be, device, 'sphere', iso=0.25)
    assert signed_volume(v2, f2) > vol


def check_genus(be, device='cpu'):
    """6. torus: V - E + F = 0; two disjoint spheres: 4."""
    for name, chi in (('torus', 0), ('two_spheres', 4)):
        v, f, _ = check_against_model(be, device, name)
        closed, n_edges, _ = edge_report(f)
        assert closed and len(v) - n_edges + len(f) == chi, (name, len(v) - n_edges + len(f))
        assert signed_volume(v, f) > 0


def check_lattice_valued(be, device='cpu'):
    """7. exact zeros on corners: index topology still closed, the degenerate triangles present and counted by the model."""
    v, f, ref = check_against_model(be, device, 'lattice_valued')
    closed, n_edges, _ = edge_report(f)
    assert closed and len(v) - n_edges + len(f) == 2
    # a vertex whose edge has an end exactly at iso sits ON that lattice corner; a triangle with two vertices on one corner has no area
    (nx, ny, nz), state, _ = mesh_case('lattice_valued')
    fld = state[..., 0].reshape(-1)
    step = lambda d: (d & 1) + ((d >> 1) & 1) * nx + (d >> 2) * nx * ny
    ends = ref['owner'] + np.array([step(int(d)) for d in ref['type']])
    corner = np.where(fld[ref['owner']] == 0, ref['owner'], np.where(fld[ends] == 0, ends, -1 - np.arange(len(ends))))
    collapsed = lambda faces: int((np.sort(corner[np.asarray(faces, np.int64)], axis=1)[:, [0, 1]] == np.sort(corner[np.asarray(faces, np.int64)], axis=1)[:, [1, 2]]).any(1).sum())
    n_deg = collapsed(f)
    assert n_deg > 0 and n_deg == collapsed(ref['faces']) == degenerate_count(ref['vertices'], ref['faces'])
    tri = v.astype(np.float64)[f]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) / 2
    assert int((area < 1e-5 * MESH_VOXEL ** 2).sum()) == n_deg                 # in fp32 positions too: these and no others
    print(f'lattice_valued: {n_deg} zero-area triangles of {len(f)}')


def check_half_valid(be, device='cpu'):
    """8. weight 0 for i >= nx / 2: no face uses an edge with an invalid end; every boundary edge lies in the last valid plane (its cubes are invalid)."""
    v, f, ref = check_against_model(be, device, 'half_valid')
    (nx, ny, nz), state, _ = mesh_case('half_valid')
    valid = (state[..., 1] >= 1.0).reshape(-1)
    step = lambda d: (d & 1) + ((d >> 1) & 1) * nx + (d >> 2) * nx * ny
    used = np.unique(f)
    ends = ref['owner'][used] + np.array([step(int(d)) for d in ref['type'][used]])
    assert valid[ref['owner'][used]].all() and valid[ends].all()
    closed, _, boundary = edge_report(f)
    assert not closed and len(boundary) > 0
    bv = np.unique(boundary)
    assert (ref['owner'][bv] % nx == nx // 2 - 1).all() and (ref['type'][bv] & 1 == 0).all()
    # away from that plane the surface is closed: every other edge is shared by two triangles of opposite direction
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und, counts = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    assert set(counts.tolist()) == {1, 2}


def check_edge_cases(be, device='cpu'):
    """9. empty result, extents of 2, nx across a wave and a workgroup, two runs byte-identical."""
    v, f, vc = run_extract(be, device, 'all_positive')
    assert v.shape == (0, 3) and f.shape == (0, 3) and vc is None
    for name in ('extent_2', 'nx_65', 'nx_129'):
        v, f, ref = check_against_model(be, device, name)
        assert len(f) > 0
        if name != 'extent_2':
            assert (ref['owner'] % mesh_case(name)[0][0]).max() == mesh_case(name)[0][0] - 1      # vertices owned beyond the first wave / workgroup of a row
    a, b = run_extract(be, device, 'sphere'), run_extract(be, device, 'sphere')
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


def refusal_cases(lib):
    """9, last item: each refusal comes back as fgs_status -1 with a text, before anything touches a device (every pointer is NULL or bogus)."""
    _lib, _ = helpers.backend_modules()
    view = (_lib.TsdfView * 9)()
    for k in range(9):
        view[k] = _lib.TsdfView(64, 1.0, 1.0, 0.0, 0.0, 64, None, None)
    integrate = lambda dims=(4, 4, 4), voxel=0.1, trunc=0.3, n_views=1, tw=64: lib.fgs_tsdf_integrate(tw, None, *dims, 0.0, 0.0, 0.0, voxel, trunc, view, n_views, 8, 8,
                                                                                                      0.1, 10.0, 0.5, 100.0, None)
    over = (2, 3, 44739243)                                   # 2^28 + 2 points: the smallest excess three extents >= 2 can make (2^28 + 1 = 17 x a prime)
    assert over[0] * over[1] * over[2] == 2 ** 28 + 2
    out = []
    for what, kw in (('extent 1', dict(dims=(1, 4, 4))), ('2^28 + 2 points', dict(dims=over)), ('V = 0', dict(n_views=0)), ('V = 9', dict(n_views=9)),
                     ('voxel_size 0', dict(voxel=0.0)), ('trunc 0', dict(trunc=0.0)), ('trunc nan', dict(trunc=float('nan'))), ('NULL volume', dict(tw=None))):
        out.append((what, integrate(**kw), lib.fgs_last_error().decode()))
    counts = (C.c_int64 * 2)()
    out.append(('count extent 1', lib.fgs_tsdf_mesh_count(64, 4, 1, 4, 0.0, 1.0, 64, counts, None), lib.fgs_last_error().decode()))
    out.append(('count too large', lib.fgs_tsdf_mesh_count(64, *over, 0.0, 1.0, 64, counts, None), lib.fgs_last_error().decode()))
    out.append(('count NULL scratch', lib.fgs_tsdf_mesh_count(64, 4, 4, 4, 0.0, 1.0, None, counts, None), lib.fgs_last_error().decode()))
    emit = lambda nv, nf, v, f, dims=(4, 4, 4): lib.fgs_tsdf_mesh_emit(64, None, *dims, 0.0, 0.0, 0.0, 0.1, 0.0, 1.0, 64, nv, nf, v, None, f, None)
    out.append(('emit NULL vertices', emit(3, 1, None, 64), lib.fgs_last_error().decode()))
    out.append(('emit NULL faces', emit(3, 1, 64, None), lib.fgs_last_error().decode()))
    out.append(('emit extent 1', emit(0, 0, None, None, dims=(4, 4, 1)), lib.fgs_last_error().decode()))
    for what, status, text in out:
        assert status == -1 and text, (what, status, text)
    assert emit(0, 0, None, None) == 0                        # an empty mesh is a normal result: nothing is launched
    assert lib.fgs_tsdf_mesh_scratch_bytes(1, 4, 4) == 0 and lib.fgs_tsdf_mesh_scratch_bytes(*over) == 0
    assert lib.fgs_tsdf_mesh_scratch_bytes(1024, 512, 512) >= 4 * 2 ** 28           # exactly 2^28 points is accepted
    return out


# ------------------------------------------------------------------ surface: harness, files, end to end ---------------------------------------------------
def check_harness_round_trip(be, tmp_path, device='cpu'):
    """10. harness.mesh.extract_mesh == render_image_aux -> tsdf_integrate -> tsdf_extract_mesh composed by hand, bit for bit; the PLY round trip."""
    import FasterGSCudaBackend as B
    from harness import mesh as HM
    from harness.scenes import make_s0, orbit_views
    from harness.trainer import Gaussians, extract_settings, render_image_aux
    params, _ = make_s0(n=1000)
    g = Gaussians(params, device)
    views = [v.to(device) for v in orbit_views(n_views=4, radius=4.0, cam_height=1.0, width=96, height=64, focal=80.0)]
    origin, voxel, dims, trunc = (-1.2, -1.2, -1.2), 0.1, (25, 24, 26), 0.35
    v1, f1, c1 = HM.extract_mesh(g, views, origin, voxel, dims, trunc=trunc, batch=3)
    tw, col = empty_volume(dims, device)
    outs = [render_image_aux(g, v, to_chw=True, alpha=True, depth='median') for v in views]
    B.tsdf_integrate(tw, col, origin, voxel, trunc, [extract_settings(v, g.active_sh_bases, v.background_color) for v in views],
                     [o['depth_median'] for o in outs], [o['alpha'] for o in outs], [o['rgb'] for o in outs], near=views[0].near_plane)
    v2, f2, c2 = B.tsdf_extract_mesh(tw, col, origin, voxel)
    assert len(f1) > 0 and torch.equal(v1, v2) and torch.equal(f1, f2) and torch.equal(c1, c2)
    assert int(f1.max()) < len(v1) and int(f1.min()) >= 0
    # expected depth goes through the same path
    v3, f3, _ = HM.extract_mesh(g, views, origin, voxel, dims, trunc=trunc, depth='expected', color=False)
    assert len(f3) > 0
    path = tmp_path / 'mesh.ply'
    HM.save_mesh_ply(path, v1, f1, c1)
    lv, lf, lc = HM.load_mesh_ply(path)
    assert torch.equal(lv, v1.cpu()) and torch.equal(lf, f1.cpu()) and lc.dtype == torch.uint8
    assert torch.equal(lc, (c1.cpu().clamp(0, 1) * 255).round().to(torch.uint8))
    HM.save_mesh_ply(tmp_path / 'again.ply', lv, lf, lc.float() / 255)
    assert (tmp_path / 'again.ply').read_bytes() == path.read_bytes()
    head = path.read_bytes().split(b'end_header\n')[0].decode().splitlines()
    assert head[:2] == ['ply', 'format binary_little_endian 1.0'] and 'property list uchar int vertex_indices' in head and 'property uchar red' in head
    HM.save_mesh_ply(tmp_path / 'plain.ply', v1, f1)
    pv, pf, pc = HM.load_mesh_ply(tmp_path / 'plain.ply')
    assert torch.equal(pv, v1.cpu()) and torch.equal(pf, f1.cpu()) and pc is None


def sphere_disk_scene(n=2500, radius=1.0, seed=7):
    """Opaque thin disks in the tangent planes of a sphere (the way harness.scenes.make_surface_scene lays its ellipsoids out)."""
    from harness.scenes import _logit, rgb_to_sh0
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    spacing = math.sqrt(4 * math.pi * radius ** 2 / n)
    s_t = torch.full((n, 2), 1.1 * spacing)
    q = torch.nn.functional.normalize(torch.stack([1 + d[:, 2], -d[:, 1], d[:, 0], torch.zeros(n)], dim=1), dim=1)      # local z onto the normal
    rgb = 0.5 + 0.5 * d
    return {'means': radius * d, 'scales': torch.log(torch.cat([s_t, 0.1 * s_t[:, :1]], dim=1)), 'rotations': q, 'opacities': _logit(torch.full((n, 1), 0.995)),
            'sh_coefficients_0': rgb_to_sh0(rgb).reshape(n, 1, 3), 'sh_coefficients_rest': torch.zeros(n, 15, 3)}


def check_end_to_end(device='cpu', n=2500, size=(88, 88)):
    """11. disks on a sphere, six views, median depth: a non-empty mesh whose vertices lie within a voxel of the sphere (median)."""
    from harness import mesh as HM
    from harness.scenes import look_at_view
    from harness.trainer import Gaussians
    g = Gaussians(sphere_disk_scene(n), device)
    eyes = ((3.2, 0.2, 0.1), (-3.2, -0.1, 0.3), (0.2, 3.2, -0.1), (0.1, -3.2, 0.2), (0.3, 0.1, 3.2), (-0.2, 0.2, -3.2))
    views = [look_at_view(e, (0.0, 0.0, 0.0), size[0], size[1], 0.75 * size[0]) for e in eyes]
    voxel, dims = 0.08, (34, 33, 35)
    v, f, c = HM.extract_mesh(g, views, (-1.32, -1.3, -1.36), voxel, dims, trunc=4 * voxel)
    assert len(f) > 500 and c is not None
    dist = (v.double().norm(dim=1) - 1.0).abs() / voxel
    median = float(dist.median())
    print(f'end to end: {len(v)} vertices, {len(f)} faces, median |r - 1| = {median:.3f} voxels, 90th percentile {float(dist.quantile(0.9)):.3f}')
    assert median < END_TO_END_BAR_VOXELS, median
    return median
