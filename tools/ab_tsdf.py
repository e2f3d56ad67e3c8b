"""What do the TSDF fusion and the mesh extraction cost on the device, and how close to their traffic do they run? In ONE process, every timed block is `--reps`
calls between two HIP events on the stream after a warm-up; the variants of a comparison take turns inside every round. Reported: medians (min / max).

(a) integration at 256^3 and 512^3 lattice points (--sizes) with 1920x1080 maps (analytic depth of a sphere seen from orbit views, opacity 1), for V = 1 and
    V = 8 views per call, state only (no colour volume): Backend.tsdf_integrate against the SAME update written with torch elementwise operators on the
    same device (project every lattice point, gather the nearest pixel, running mean under torch.where) -- nothing in the parent commit does this work,
    so that is the baseline. Both results are compared first: the shares of points whose weight differs or whose tsdf differs by more than 1e-5
    (points whose pixel or truncation test a rounding flips; the kernel multiplies by reciprocals where torch divides).
    Algorithmic bytes of the kernel: 8 read + 8 written per lattice point that is updated + 4 per depth sample actually read (one per point and view
    that reaches the pixel test; they are cache hits: the maps are 8 MB each), next to bench.HBM_PEAK_GBS.
(b) extraction of a sphere of radius 0.35 * n voxels at both sizes: fgs_tsdf_mesh_count (classify + scan + the read-back of the sizes) and
    fgs_tsdf_mesh_emit alone. Algorithmic bytes: count 8 read + 4 written per point; emit 4 read per point + 12 per vertex + 12 per triangle written.
(c) --bench-steps K > 0: `bench.py --gpus 1 --steps K --warmup 3 --no-extras --no-cpu-baseline --no-pmc` as child processes, of this tree and, with
    --parent-tree (a built checkout of the parent commit: its Python binds only the symbols its own library has), of the parent, alternating,
    --bench-runs times each: the headline lines, to show the plain path within the parent's own spread.
Writes profiles/tsdf_ab.json (or --out). Nothing is gated."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / 'faster-gaussian-splatting_amd')]


def timed_rounds(variants: dict, rounds: int, reps: int, warmup: int) -> dict:
    order = list(variants)
    for k in order:
        for _ in range(warmup):
            variants[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in order}
    for rnd in range(rounds):
        shift = rnd % len(order)
        for k in order[shift:] + order[:shift]:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                variants[k]()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / reps)
    return times


def summary(v: list) -> dict:
    return {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v), 'ms_rounds': [round(x, 4) for x in v]}


def sphere_depth(view, radius, dev):
    """[H,W] view-space z of the first hit of the pixel-centre rays with a sphere at the world origin; a plane 1.5 radii behind its centre elsewhere."""
    M = view.w2c.double()
    ys, xs = torch.meshgrid(torch.arange(view.height, dtype=torch.float64) + 0.5, torch.arange(view.width, dtype=torch.float64) + 0.5, indexing='ij')
    ray = torch.stack([(xs - view.center_x) / view.focal_x, (ys - view.center_y) / view.focal_y, torch.ones_like(xs)], dim=-1)
    c = M[:3, 3]
    a, b, cc = (ray * ray).sum(-1), -2.0 * (ray @ c), c @ c - radius * radius
    disc = b * b - 4 * a * cc
    t = torch.where(disc > 0, (-b - disc.clamp_min(0).sqrt()) / (2 * a), c.norm() + 1.5 * radius)
    return t.float().contiguous().to(dev)


def torch_integrate(tw, P, views, depths, trunc, near, depth_max, max_weight):
    """The definition with framework operators, in place on tw [nz,ny,nx,2]; P [nz,ny,nx,3] lattice positions (made once, outside the timed region)."""
    t, w = tw[..., 0], tw[..., 1]
    for V, depth in zip(views, depths):
        M = V.w2c
        h, wd = depth.shape
        z = P[..., 0] * M[2, 0] + P[..., 1] * M[2, 1] + P[..., 2] * M[2, 2] + M[2, 3]
        x = P[..., 0] * M[0, 0] + P[..., 1] * M[0, 1] + P[..., 2] * M[0, 2] + M[0, 3]
        y = P[..., 0] * M[1, 0] + P[..., 1] * M[1, 1] + P[..., 2] * M[1, 2] + M[1, 3]
        ok = z > near
        u, v = torch.floor(V.focal_x * x / z + V.center_x), torch.floor(V.focal_y * y / z + V.center_y)
        ok &= (u >= 0) & (u < wd) & (v >= 0) & (v < h)
        pix = (v.clamp(0, h - 1) * wd + u.clamp(0, wd - 1)).long()
        d = depth.reshape(-1)[pix]
        sdf = d - z
        ok &= (d > 0) & (d <= depth_max) & (sdf >= -trunc)
        f = (sdf / trunc).clamp_max(1.0)
        w1 = w + 1.0
        t.copy_(torch.where(ok, (t * w + f) / w1, t))
        w.copy_(torch.where(ok, w1.clamp_max(max_weight), w))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--bench-steps', type=int, default=0, help='(c): steps of each bench.py child run; 0 = skip')
    ap.add_argument('--bench-runs', type=int, default=3)
    ap.add_argument('--parent-tree', default='', help='a built checkout of the parent commit for (c)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'tsdf_ab.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ab_tsdf.py measures on the GPU; none is visible')

    import bench
    from FasterGSCudaBackend import _backend
    from harness.scenes import orbit_views
    from harness.trainer import extract_settings
    dev = torch.device('cuda:0')
    be = _backend.default_backend()
    result = {'what': 'TSDF fusion and mesh extraction; medians over alternating rounds of HIP-event-timed blocks', 'device': torch.cuda.get_device_name(dev),
              'box': os.uname().nodename, 'library': be.lib.fgs_build_info().decode(), 'rounds': args.rounds, 'reps': args.reps, 'hbm_rate_gbs': bench.HBM_PEAK_GBS,
              'integration': {}, 'extraction': {}}
    views = [v.to(dev) for v in orbit_views(n_views=8, radius=3.0, cam_height=1.0)]
    settings = [extract_settings(v, 1, v.background_color) for v in views]
    radius, near, depth_max, max_weight = 0.7, 0.2, 100.0, 65536.0
    depths = [sphere_depth(v.to('cpu'), radius, dev) for v in views]

    for n in args.sizes:
        voxel = 2.0 / n
        origin, trunc = (-1.0, -1.0, -1.0), 4 * voxel
        idx = torch.arange(n, device=dev, dtype=torch.float32)
        k, j, i = torch.meshgrid(idx, idx, idx, indexing='ij')
        P = torch.stack([origin[0] + voxel * i, origin[1] + voxel * j, origin[2] + voxel * k], dim=-1)
        del k, j, i
        entry = {}
        for nv in (1, 8):
            tw_a = torch.zeros((n, n, n, 2), device=dev)
            tw_b = torch.zeros_like(tw_a)
            fused = lambda tw=tw_a: be.tsdf_integrate(tw, None, origin, voxel, trunc, settings[:nv], depths[:nv], None, None, near, depth_max, 0.5, max_weight)
            framework = lambda tw=tw_b: torch_integrate(tw, P, views[:nv], depths[:nv], trunc, near, depth_max, max_weight)
            fused(); framework()
            # a point whose pixel or truncation test sits within a rounding of flipping takes another sample in the two formulations: shares, not maxima
            agree = {'weights_differ_share': float((tw_a[..., 1] != tw_b[..., 1]).float().mean()),
                     'tsdf_differs_by_more_than_1e-5_share': float(((tw_a[..., 0] - tw_b[..., 0]).abs() > 1e-5).float().mean())}
            touched = int((tw_a[..., 1] > 0).sum())
            samples = int(tw_a[..., 1].sum())                                     # one per (point, view) update; the skipped ones read a sample too, not counted
            times = timed_rounds({'fused': fused, 'torch': framework}, args.rounds, args.reps, args.warmup)
            ms = statistics.median(times['fused'])
            nbytes = 8 * n ** 3 + 8 * touched + 4 * samples
            entry[f'V{nv}'] = {'fused': summary(times['fused']), 'torch': summary(times['torch']), 'torch_over_fused': statistics.median(times['torch']) / ms,
                               'agreement': agree, 'points': n ** 3, 'points_updated_per_call': touched, 'algorithmic_bytes': nbytes,
                               'achieved_gbs': nbytes / ms / 1e6, 'fraction_of_hbm_rate': nbytes / ms / 1e6 / bench.HBM_PEAK_GBS, 'ms_per_view': ms / nv}
            print(f'(a) {n}^3 V={nv}: fused {ms:.4f} ms ({ms / nv:.4f} per view), torch {statistics.median(times["torch"]):.3f} ms '
                  f'({entry[f"V{nv}"]["torch_over_fused"]:.1f}x); {nbytes / 1e6:.0f} MB -> {nbytes / ms / 1e6:.0f} GB/s; agreement {agree}', flush=True)
            del tw_a, tw_b
        result['integration'][str(n)] = entry
        del P

        # ---- (b) a sphere written straight into the volume ----
        c = idx - (n / 2 - 0.37)
        r = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2).sqrt()
        tw = torch.stack([((r - 0.35 * n) / 4.0).clamp(-1, 1), torch.ones_like(r)], dim=-1).contiguous()
        del r
        v, f, _ = be.tsdf_extract_mesh(tw, None, origin, voxel)
        nvx, nf = len(v), len(f)
        import ctypes as C
        scratch = torch.empty(be.lib.fgs_tsdf_mesh_scratch_bytes(n, n, n), dtype=torch.uint8, device=dev)
        counts = (C.c_int64 * 2)()
        stream = torch.cuda.current_stream(dev).cuda_stream
        count = lambda: be.lib.fgs_tsdf_mesh_count(tw.data_ptr(), n, n, n, 0.0, 1.0, scratch.data_ptr(), counts, stream)
        emit = lambda: be.lib.fgs_tsdf_mesh_emit(tw.data_ptr(), None, n, n, n, *origin, voxel, 0.0, 1.0, scratch.data_ptr(), nvx, nf, v.data_ptr(), None, f.data_ptr(), stream)
        assert count() == 0 and (counts[0], counts[1]) == (nvx, nf) and emit() == 0
        times = timed_rounds({'count': count, 'emit': emit}, args.rounds, args.reps, args.warmup)
        ex = {'vertices': nvx, 'triangles': nf}
        for name, nbytes in (('count', 12 * n ** 3), ('emit', 4 * n ** 3 + 12 * nvx + 12 * nf)):
            ms = statistics.median(times[name])
            ex[name] = dict(summary(times[name]), algorithmic_bytes=nbytes, achieved_gbs=nbytes / ms / 1e6, fraction_of_hbm_rate=nbytes / ms / 1e6 / bench.HBM_PEAK_GBS)
            print(f'(b) {n}^3 {name}: {ms:.4f} ms; {nbytes / 1e6:.0f} MB -> {nbytes / ms / 1e6:.0f} GB/s ({nvx} vertices, {nf} triangles)', flush=True)
        result['extraction'][str(n)] = ex
        del tw, scratch, v, f
        torch.cuda.empty_cache()

    # ---- (c) the plain path: bench.py headline lines, this tree and the parent's library, fresh child processes ----
    if args.bench_steps > 0:
        flags = ['--gpus', '1', '--steps', str(args.bench_steps), '--warmup', '3', '--no-extras', '--no-cpu-baseline', '--no-pmc']
        trees = {'this_tree': ROOT}
        if args.parent_tree:
            trees['parent_tree'] = Path(args.parent_tree).resolve()
        lines = {k: [] for k in trees}
        for _ in range(args.bench_runs):
            for name, tree in trees.items():
                out = subprocess.run([sys.executable, str(tree / 'bench.py'), *flags], capture_output=True, text=True, timeout=600, cwd=str(tree))
                if out.returncode != 0 or not out.stdout.strip():
                    sys.exit(f'bench.py of {name} failed ({out.returncode}): {out.stderr[-2000:]}')
                line = json.loads(out.stdout.strip().splitlines()[-1])
                lines[name].append({k: line.get(k) for k in ('metric', 'value', 'unit', 'ms_per_step')})
                print(f'(c) {name}: {lines[name][-1]}', flush=True)
        cmd = ['python', 'bench.py', *flags]
        result['bench_headline'] = {'command': ' '.join(cmd), 'runs': lines,
                                    'median_value': {k: statistics.median(x['value'] for x in v) for k, v in lines.items()},
                                    'spread_value': {k: max(x['value'] for x in v) - min(x['value'] for x in v) for k, v in lines.items()}}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
