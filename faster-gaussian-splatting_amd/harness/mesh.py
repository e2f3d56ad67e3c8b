"""From a trained model to a triangle mesh: render depth from the training views, fuse the maps into a TSDF volume, extract the zero level set -- the last
stage of the 2DGS / GOF / PGSR / RaDe-GS pipelines, which the reference projects hand to Open3D's CUDA integrator. Here it stays on the device
(`FasterGSCudaBackend.tsdf_integrate` / `tsdf_extract_mesh`, csrc/tsdf.hip). `save_mesh_ply` / `load_mesh_ply` write and read the result."""
from __future__ import annotations

import math
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from FasterGSCudaBackend import tsdf_extract_mesh, tsdf_integrate

from .scenes import View
from .trainer import Gaussians, extract_settings, render_image_aux


class TSDFVolume:
    """A dense volume of dims = (nx, ny, nz) lattice points, point (i, j, k) at origin + voxel_size * (i, j, k); trunc in world units."""

    def __init__(self, origin: Sequence[float], voxel_size: float, dims: Sequence[int], trunc: float, color: bool = True, device='cuda') -> None:
        nx, ny, nz = (int(d) for d in dims)
        self.origin, self.voxel_size, self.dims, self.trunc = tuple(float(o) for o in origin), float(voxel_size), (nx, ny, nz), float(trunc)
        self.tsdf_weight = torch.zeros((nz, ny, nx, 2), dtype=torch.float32, device=device)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=device) if color else None

    @torch.no_grad()
    def integrate(self, gaussians: Gaussians, views: Sequence[View], depth: str = 'median', min_alpha: float = 0.5, batch: int = 8,
                  depth_max: float = math.inf, max_weight: float = 65536.0) -> None:
        """Renders every view through `render_image_aux` and folds the maps in, `batch` views per launch. depth: 'median' (the depth at which transmittance
        crosses one half) or 'expected' (the blended depth divided by the accumulated opacity)."""
        if depth not in ('median', 'expected'):
            raise ValueError(f"depth must be 'median' or 'expected', not {depth!r}")
        device = self.tsdf_weight.device
        for first in range(0, len(views), max(int(batch), 1)):
            settings, depths, alphas, colors = [], [], [], []
            for view in views[first:first + max(int(batch), 1)]:
                view = view.to(device)
                out = render_image_aux(gaussians, view, to_chw=True, alpha=True, depth=depth, normalize_depth=depth == 'expected')
                settings.append(extract_settings(view, gaussians.active_sh_bases, view.background_color))
                depths.append(out['depth_median' if depth == 'median' else 'depth'].contiguous())
                alphas.append(out['alpha'].contiguous())
                colors.append(out['rgb'].contiguous())
            tsdf_integrate(self.tsdf_weight, self.color, self.origin, self.voxel_size, self.trunc, settings, depths, alphas,
                           colors if self.color is not None else None, near=views[0].near_plane, depth_max=depth_max, min_alpha=min_alpha, max_weight=max_weight)

    def extract(self, iso: float = 0.0, min_weight: float = 1.0) -> tuple:
        """(vertices [Nv,3], faces [Nf,3] int32, colors [Nv,3] or None) on the volume's device."""
        return tsdf_extract_mesh(self.tsdf_weight, self.color, self.origin, self.voxel_size, iso=iso, min_weight=min_weight)


def extract_mesh(gaussians: Gaussians, views: Sequence[View], origin: Sequence[float], voxel_size: float, dims: Sequence[int], trunc: Optional[float] = None,
                 color: bool = True, depth: str = 'median', min_alpha: float = 0.5, batch: int = 8, iso: float = 0.0, min_weight: float = 1.0,
                 depth_max: float = math.inf) -> tuple:
    """Render, fuse and extract in one call; trunc defaults to four voxels. Returns (vertices, faces, colors)."""
    volume = TSDFVolume(origin, voxel_size, dims, 4.0 * voxel_size if trunc is None else trunc, color=color, device=gaussians.means.device)
    volume.integrate(gaussians, views, depth=depth, min_alpha=min_alpha, batch=batch, depth_max=depth_max)
    return volume.extract(iso=iso, min_weight=min_weight)


def save_mesh_ply(path, vertices: torch.Tensor, faces: torch.Tensor, colors: Optional[torch.Tensor] = None) -> None:
    """Binary little-endian PLY: `vertex` x y z (float) and, with colours in [0, 1], uchar red green blue; `face` as `list uchar int vertex_indices`."""
    v = np.ascontiguousarray(vertices.detach().cpu().numpy(), dtype='<f4').reshape(-1, 3)
    f = np.ascontiguousarray(faces.detach().cpu().numpy(), dtype='<i4').reshape(-1, 3)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    if colors is not None:
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    vert = np.empty(v.shape[0], dtype=fields)
    vert['x'], vert['y'], vert['z'] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c = np.rint(np.clip(colors.detach().cpu().numpy().reshape(-1, 3), 0.0, 1.0) * 255.0).astype('u1')
        vert['red'], vert['green'], vert['blue'] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(f.shape[0], dtype=[('n', 'u1'), ('idx', '<i4', (3,))])
    face['n'], face['idx'] = 3, f
    header = ['ply', 'format binary_little_endian 1.0', 'comment Generated with faster-gaussian-splatting_amd', f'element vertex {v.shape[0]}']
    header += [f'property {"uchar" if t == "u1" else "float"} {n}' for n, t in fields]
    header += [f'element face {f.shape[0]}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as out:
        out.write(('\n'.join(header) + '\n').encode('ascii'))
        out.write(vert.tobytes())
        out.write(face.tobytes())


def load_mesh_ply(path, device='cpu') -> tuple:
    """(vertices [Nv,3] float32, faces [Nf,3] int32, colors [Nv,3] uint8 or None) of a file written by `save_mesh_ply`."""
    raw = Path(path).read_bytes()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    lines = raw[:end].decode('ascii').splitlines()
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    nv = int(next(l for l in lines if l.startswith('element vertex')).split()[-1])
    nf = int(next(l for l in lines if l.startswith('element face')).split()[-1])
    props = [l.split()[1:] for l in lines if l.startswith('property') and not l.startswith('property list')]
    vert = np.frombuffer(raw, dtype=[(n, 'u1' if t == 'uchar' else '<f4') for t, n in props], count=nv, offset=end)
    face = np.frombuffer(raw, dtype=[('n', 'u1'), ('idx', '<i4', (3,))], count=nf, offset=end + vert.nbytes)
    assert nf == 0 or bool((face['n'] == 3).all())
    vertices = torch.from_numpy(np.stack([vert['x'], vert['y'], vert['z']], axis=1).astype(np.float32)).reshape(nv, 3)
    faces = torch.from_numpy(face['idx'].astype(np.int32)).reshape(nf, 3)
    colors = torch.from_numpy(np.stack([vert['red'], vert['green'], vert['blue']], axis=1)).reshape(nv, 3) if 'red' in vert.dtype.names else None
    return vertices.to(device), faces.to(device), None if colors is None else colors.to(device)
