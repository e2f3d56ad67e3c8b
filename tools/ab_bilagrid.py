"""What does the per-view bilateral-grid colour correction cost, and what does fusing it buy? At 1920x1080 with a 16x16x8 grid per view, in ONE process,
alternating: every timed block is `--reps` calls between two HIP events on the stream, after a warm-up; the variants take turns inside every round,
so drift of the box hits all alike. Reported: the median over the rounds (min / max), and differences next to the spread of the rounds.

(a) operator against torch: forward + backward (gradients for image and grid) of FasterGSCudaBackend.bilagrid_slice against the same function
    written with F.grid_sample + einsum (fp32, same device, same inputs: a rendered S2 view and a perturbed identity grid; the pixel coordinates of the
    torch form are made once, outside the timed region). Their outputs and gradients are compared first.
(b) per kernel: Backend.bilagrid_slice (one launch) and Backend.bilagrid_slice_backward (scratch clear, the kernel, the transpose) alone, next to their
    traffic floors -- 25 MB read + 25 MB written and 75 MB -- at the HBM rate bench.py uses for its rooflines (HBM_PEAK_GBS), and the achieved fraction.
(c) training step: harness.trainer.training_iteration over the S2 orbit views without and with a BilateralGrids module (TV term and grid optimizer
    included). Two plain variants run (A/A: what the rounds' spread is); with --parent-library (a libfgs_hip.so built from the parent commit) a third
    plain variant runs through that library: the plain iteration of this tree must equal it within the spread.
Writes profiles/bilagrid_ab.json (or --out). The differences are recorded, not gated."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / 'faster-gaussian-splatting_amd')]
LUMA = (0.299, 0.587, 0.114)


def torch_slice(image, grid, xy):
    """The definition with framework operators: grid_sample of the 12 channels at (x, y, luma), then the 3 x 4 matrix product."""
    guide = (LUMA[0] * image[0] + LUMA[1] * image[1] + LUMA[2] * image[2]).clamp(0.0, 1.0)
    coords = torch.cat([xy, guide[..., None] * 2.0 - 1.0], dim=-1)
    M = F.grid_sample(grid[None], coords[None, None], mode='bilinear', align_corners=True, padding_mode='border')[0, :, 0]
    M = M.reshape(3, 4, *image.shape[1:])
    return torch.einsum('ijhw,jhw->ihw', M[:, :3], image) + M[:, 3]


def timed_rounds(variants: dict, rounds: int, reps: int, warmup: int) -> dict:
    """variants: name -> callable. ms per call of every variant in every round, the variants taking turns."""
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


def summary(times: dict) -> dict:
    return {k: {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v), 'ms_rounds': [round(x, 4) for x in v]} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=20, help='operator / kernel calls per timed block')
    ap.add_argument('--step-reps', type=int, default=2, help='passes over the views per timed block of training iterations')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--grid', type=int, nargs=3, default=[16, 16, 8], metavar=('WG', 'HG', 'L'))
    ap.add_argument('--parent-library', default='', help='libfgs_hip.so of the parent commit: the plain training iteration through it joins the rounds of (c)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'bilagrid_ab.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ab_bilagrid.py measures on the GPU; none is visible')

    import bench
    import FasterGSCudaBackend as B
    from FasterGSCudaBackend import _backend, _lib
    from harness import trainer as T
    from harness.bilagrid import BilateralGrids
    argv, sys.argv = sys.argv, ['bench.py'] + (['--n-gaussians', str(args.n_gaussians)] if args.n_gaussians else [])
    params, views, what = bench.build_scene(bench.parse())
    sys.argv = argv
    dev = torch.device('cuda:0')
    be = _backend.default_backend()
    views = [v.to(dev) for v in views]
    gw, gh, gl = args.grid
    truth = T.Gaussians(params, dev)
    with torch.no_grad():
        targets = [T.render_image_training(truth, v, False, v.background_color).clamp(0.0, 1.0) for v in views]
    del truth
    image = targets[0].contiguous()
    _, h, w = image.shape
    gen = torch.Generator().manual_seed(1)
    grid = torch.zeros(12, gl, gh, gw)
    grid[[0, 5, 10]] = 1.0
    grid = (grid + 0.1 * torch.randn(grid.shape, generator=gen)).to(dev)
    gO = (torch.randn(3, h, w, generator=gen) / (3 * h * w)).to(dev)
    result = {'what': f'bilateral-grid colour correction, {w}x{h}, grid {gw}x{gh}x{gl}; medians over alternating rounds of HIP-event-timed blocks',
              'scene': what, 'device': torch.cuda.get_device_name(dev), 'box': os.uname().nodename, 'library': be.lib.fgs_build_info().decode(),
              'rounds': args.rounds, 'lds_staged': be.bilagrid_staged(grid.shape, w, h)}

    # ---- (a) the operator against the torch formulation ----
    ys, xs = torch.meshgrid((torch.arange(h, device=dev, dtype=torch.float32) + 0.5) / h, (torch.arange(w, device=dev, dtype=torch.float32) + 0.5) / w, indexing='ij')
    xy = (torch.stack([xs, ys], dim=-1) * 2.0 - 1.0).contiguous()
    leaves = lambda: (image.clone().requires_grad_(True), grid.clone().requires_grad_(True))

    def fused():
        i, g = leaves()
        B.bilagrid_slice(i, g).backward(gO)
        return i.grad, g.grad

    def framework():
        i, g = leaves()
        torch_slice(i, g, xy).backward(gO)
        return i.grad, g.grad

    def only_leaves():           # what both pay for making their leaves: subtracted from neither, reported
        leaves()
    rel = lambda a, r: float((a - r).abs().max() / r.abs().max().clamp_min(1e-30))
    with torch.no_grad():
        agree = {'out': rel(B.bilagrid_slice(image, grid), torch_slice(image, grid, xy))}
    (fi, fg), (ti, tg) = fused(), framework()
    agree.update(grad_image=rel(fi, ti), grad_grid=rel(fg, tg))
    op = timed_rounds({'fused': fused, 'torch': framework, 'leaves_only': only_leaves}, args.rounds, args.reps, args.warmup)
    med = {k: statistics.median(v) for k, v in op.items()}
    result['operator'] = {'forward_plus_backward': summary(op), 'fused_vs_torch_rel_inf': agree, 'torch_over_fused': med['torch'] / med['fused'],
                          'torch_minus_fused_ms': med['torch'] - med['fused'],
                          'spread_ms': max(max(op[k]) - min(op[k]) for k in ('fused', 'torch'))}
    print(f'(a) forward + backward: fused {med["fused"]:.4f} ms, torch {med["torch"]:.4f} ms ({med["torch"] / med["fused"]:.1f}x), difference '
          f'{med["torch"] - med["fused"]:+.4f} ms, spread of the rounds {result["operator"]["spread_ms"]:.4f} ms; agreement {agree}', flush=True)

    # ---- (b) the kernels alone next to their traffic floors ----
    plane = 3 * w * h * 4
    floors = {'slice': 2 * plane, 'slice_backward': 3 * plane}
    kernels = timed_rounds({'slice': lambda: be.bilagrid_slice(image, grid),
                            'slice_backward': lambda: be.bilagrid_slice_backward(image, grid, gO),
                            'slice_backward_image_only': lambda: be.bilagrid_slice_backward(image, grid, gO, need_grid=False),
                            'tv': lambda: be.bilagrid_tv(grid)}, args.rounds, args.reps, args.warmup)
    result['kernels'] = summary(kernels)
    for k, nbytes in floors.items():
        ms = statistics.median(kernels[k])
        e = result['kernels'][k]
        e.update(traffic_floor_bytes=nbytes, hbm_rate_gbs=bench.HBM_PEAK_GBS, floor_ms=nbytes / bench.HBM_PEAK_GBS / 1e6,
                 achieved_gbs=nbytes / ms / 1e6, fraction_of_hbm_rate=nbytes / ms / 1e6 / bench.HBM_PEAK_GBS)
        print(f'(b) {k:15s} {ms:.4f} ms; floor {e["floor_ms"]:.4f} ms ({nbytes / 1e6:.0f} MB at {bench.HBM_PEAK_GBS:.0f} GB/s): {e["achieved_gbs"]:.0f} GB/s = '
              f'{e["fraction_of_hbm_rate"]:.3f} of the rate', flush=True)
    print('(b) image gradient only', round(statistics.median(kernels['slice_backward_image_only']), 4), 'ms; tv', round(statistics.median(kernels['tv']), 4), 'ms', flush=True)

    # ---- (c) the training iteration without and with the grids ----
    def trainer_of(backend, with_grids):
        g = T.Gaussians({k: v.clone() for k, v in params.items()}, dev)
        g.training_setup(training_cameras_extent=5.0)
        m = None
        if with_grids:
            m = BilateralGrids(len(views), shape=(gw, gh, gl), device=dev)
            m.training_setup()
        state = {'it': 0}

        def step():
            saved, _backend._DEFAULT = _backend._DEFAULT, backend          # every operator of the iteration asks default_backend()
            try:
                for i, v in enumerate(views):
                    T.training_iteration(g, v, targets[i], state['it'], bilagrid=m, view_index=i if m is not None else None)
                    state['it'] += 1
            finally:
                _backend._DEFAULT = saved
        return step
    variants = {'plain': trainer_of(be, False), 'plain_again': trainer_of(be, False), 'with_grids': trainer_of(be, True)}
    if args.parent_library:
        variants['plain_parent_library'] = trainer_of(_backend.Backend(_bind_parent(_lib, args.parent_library)), False)
    steps = timed_rounds(variants, args.rounds, args.step_reps, args.warmup)
    per_iter = {k: [x / len(views) for x in v] for k, v in steps.items()}
    med = {k: statistics.median(v) for k, v in per_iter.items()}
    entry = {'ms_per_iteration': summary(per_iter), 'iterations_per_block': args.step_reps * len(views),
             'grids_minus_plain_ms': med['with_grids'] - med['plain'], 'plain_again_minus_plain_ms': med['plain_again'] - med['plain'],
             'plain_spread_ms': max(per_iter['plain']) - min(per_iter['plain'])}
    if args.parent_library:
        entry['plain_minus_parent_library_ms'] = med['plain'] - med['plain_parent_library']
    result['training_iteration'] = entry
    for k in per_iter:
        e = entry['ms_per_iteration'][k]
        print(f'(c) {k:22s} {e["ms_median"]:.4f} ms per iteration (min {e["ms_min"]:.4f}, max {e["ms_max"]:.4f})', flush=True)
    print(f'(c) with_grids - plain {entry["grids_minus_plain_ms"]:+.4f} ms; plain_again - plain {entry["plain_again_minus_plain_ms"]:+.4f} ms; spread of the plain rounds '
          f'{entry["plain_spread_ms"]:.4f} ms' + (f'; plain - plain_parent_library {entry["plain_minus_parent_library_ms"]:+.4f} ms' if args.parent_library else ''), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


def _bind_parent(_lib, path):
    """The parent commit's library exports everything this tree's does but the entry points the tree adds: bind what it has."""
    import ctypes as C
    lib = C.CDLL(str(path))
    for name, (restype, argtypes) in _lib._SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


if __name__ == '__main__':
    main()
