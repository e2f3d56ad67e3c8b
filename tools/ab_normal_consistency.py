"""What does the normal-consistency regulariser cost, and did adding it move the plain pass? On S2 and on layered S2 (every opacity logit lowered by 3)
at 1920x1080, in ONE process, alternating: every timed block is `--reps` passes over the orbit views between two HIP events on the stream, after a
warm-up; the variants take turns inside every round, so drift of the box hits all alike. Reported: the median over the rounds of ms per view
(min / max), and differences next to the spread of the rounds.

(a) the per-Gaussian kernel pair alone (`Backend.surface_features`, `surface_features_backward`) next to its traffic floor at bench.HBM_PEAK_GBS.
(b) the image-space pair alone (`Backend.normal_consistency`, `normal_consistency_backward`) on a blended map of the scene, next to its traffic floor.
(c) one composed call, forward + backward: gaussian_surface_features -> diff_rasterize_features -> normal_consistency(...).mean() plus a loss on the
    image; the same with the two operators written in torch (the definitions restated below, the same diff_rasterize_features in the middle); the
    feature render with five constant channels (what the rasterizer's part costs); and plain diff_rasterize.
(d) the S2 training iteration (harness.trainer.training_iteration over the views) without the term, without it a second time (A/A: the spread), and
    with normal_weight > 0.
(e) with --parent-library (a libfgs_hip.so built from the parent commit): diff_rasterize forward + backward, and the plain training iteration, through
    this tree's library, through the parent's, and through the parent's a second time. The margin is what the parent shows against itself, the largest
    per-round |parent_again - parent|; this tree's median per-round difference to the parent must lie within it (recorded, `within_margin`).
Writes profiles/normal_consistency_ab.json (or --out). No cost is fixed in advance; (e) is the one condition."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / 'faster-gaussian-splatting_amd')]


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


def bind_partial(_lib, path):
    """A library that lacks the entry points this tree adds (the parent commit's): bind what it has."""
    import ctypes as C
    lib = C.CDLL(str(path))
    for name, (restype, argtypes) in _lib._SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


# ---- the two definitions in fp32 torch (INTEGRATION.md 'Normal consistency'), as a user without the kernels would write them ----
def torch_surface_features(means, scales, rotations, w2c, cam_position):
    r, x, y, z = (rotations / rotations.norm(dim=1, keepdim=True)).unbind(dim=1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    k = torch.argmin(scales.detach(), dim=1)
    a = R[torch.arange(means.shape[0], device=means.device), :, k]
    along = (a * (means - cam_position[None, :])).sum(dim=1).detach()
    n_cam = (torch.where(along > 0, -1.0, 1.0)[:, None] * a) @ w2c[:3, :3].T
    zc = means @ w2c[2, :3] + w2c[2, 3]
    return torch.cat([n_cam, zc[:, None], torch.ones_like(zc)[:, None]], dim=1)


def torch_normal_consistency(M, fx, fy, cx, cy, min_alpha=0.5):
    Nr, D, A = M[:3], M[3], M[4]
    H, W = D.shape
    ok = A.detach() >= min_alpha
    d = torch.where(ok, D / torch.where(ok, A, torch.ones_like(A)), torch.zeros_like(D))
    xs = ((torch.arange(W, dtype=M.dtype, device=M.device) + 0.5 - cx) / fx)[None, :]
    ys = ((torch.arange(H, dtype=M.dtype, device=M.device) + 0.5 - cy) / fy)[:, None]
    P = torch.stack([xs * d, ys * d, d])
    gx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    gy = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = torch.cross(gy, gx, dim=0)
    len_sq = (c * c).sum(dim=0)
    valid = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1] & (len_sq.detach() > 1e-30)
    n_d = c / torch.sqrt(torch.where(valid, len_sq, torch.ones_like(len_sq)))[None]
    E = torch.where(valid, A[1:-1, 1:-1] - (Nr[:, 1:-1, 1:-1] * n_d).sum(dim=0), torch.zeros_like(len_sq))
    return torch.nn.functional.pad(E, (1, 1, 1, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=2, help='passes over the views per timed block')
    ap.add_argument('--warmup', type=int, default=1, help='untimed passes over the views per variant')
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--weight', type=float, default=0.05, help='normal_weight of the training iteration of (d)')
    ap.add_argument('--parent-library', default='', help='libfgs_hip.so of the parent commit: (e)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'normal_consistency_ab.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ab_normal_consistency.py measures on the GPU; none is visible')

    import bench
    import FasterGSCudaBackend as B
    from FasterGSCudaBackend import _backend, _lib
    from harness import trainer as T
    dev = torch.device('cuda:0')
    be = _backend.default_backend()
    parent = [_backend.Backend(bind_partial(_lib, args.parent_library)) for _ in range(2)] if args.parent_library else None
    none = torch.empty(0)
    result = {'what': 'normal-consistency regulariser, 1920x1080, min_alpha 0.5; ms per view (per call in kernel_pairs), medians over alternating rounds of '
                      'HIP-event-timed blocks', 'device': torch.cuda.get_device_name(dev), 'box': os.uname().nodename,
              'library': be.lib.fgs_build_info().decode(), 'rounds': args.rounds, 'scenes': {}}

    def through(backend, fn):
        def run(*a):
            saved, _backend._DEFAULT = _backend._DEFAULT, backend          # the operators ask default_backend()
            try:
                fn(*a)
            finally:
                _backend._DEFAULT = saved
        return run

    def against_parent(make) -> dict:
        """make(backend) -> callable: parent, this tree, parent again, taking turns."""
        t = per_view(timed_rounds({'parent': make(parent[0]), 'new': make(be), 'parent_again': make(parent[1])}, args.rounds, args.reps, args.warmup))
        margin = max(abs(a - b) for a, b in zip(t['parent_again'], t['parent']))
        diff = statistics.median(a - b for a, b in zip(t['new'], t['parent']))
        return dict(summary(t), parent_self_spread_ms=margin, new_minus_parent_ms=diff, within_margin=abs(diff) <= margin)

    for label, shift in (('S2', 0.0), ('layered_S2', -3.0)):
        argv, sys.argv = sys.argv, ['bench.py'] + (['--n-gaussians', str(args.n_gaussians)] if args.n_gaussians else []) + (['--opacity-shift', str(shift)] if shift else [])
        params, views, what = bench.build_scene(bench.parse())
        sys.argv = argv
        views = [v.to(dev) for v in views]
        g = T.Gaussians(params, dev)
        p = [t.detach() for t in g.tensors()]
        leaves = [t.detach().clone().requires_grad_(True) for t in g.tensors()]
        n = p[0].shape[0]
        gen = torch.Generator().manual_seed(1)
        passes = []
        for v in views:
            RS = T.extract_settings(v, g.active_sh_bases, v.background_color)
            gC = torch.randn((3, v.height, v.width), generator=gen).to(dev) / (3 * v.height * v.width)
            passes.append((v, RS, gC))
        over_views = lambda fn: (lambda: [fn(*q) for q in passes] and None)
        per_view = lambda times: {k: [x / len(passes) for x in v] for k, v in times.items()}
        entry = {'scene': what + (f', opacity logits {shift:+.1f}' if shift else ''), 'views': len(passes), 'gaussians': n}

        # ---- (a), (b) the kernel pairs alone, per call ----
        v0, RS0, _ = passes[0]
        with torch.no_grad():
            feats0 = be.surface_features(p[0], p[1], p[2], v0.w2c, v0.position)
            _, map0 = B.diff_rasterize_features(*p, none, RS0, feats0)
            E0 = be.normal_consistency(map0, RS0)[0]
        entry['valid_share_view0'], entry['consistency_mean_view0'] = float((E0 != 0).float().mean()), float(E0.mean())
        gF = torch.randn((n, 5), generator=gen).to(dev)
        gE = torch.randn(E0.shape, generator=gen).to(dev) / E0.numel()
        pixels = E0.numel()
        t = timed_rounds({'surface_features': lambda: be.surface_features(p[0], p[1], p[2], v0.w2c, v0.position),
                          'surface_features_backward': lambda: be.surface_features_backward(p[0], p[1], p[2], v0.w2c, v0.position, gF),
                          'normal_consistency': lambda: be.normal_consistency(map0, RS0),
                          'normal_consistency_backward': lambda: be.normal_consistency_backward(map0, gE, RS0)}, args.rounds, max(args.reps, 8), args.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        floor = lambda nbytes: nbytes / (bench.HBM_PEAK_GBS * 1e9) * 1e3                  # ms at the HBM peak
        floors = {'surface_features': floor(4 * n * (10 + 5)), 'surface_features_backward': floor(4 * n * (10 + 5 + 7)),
                  'normal_consistency': floor(4 * pixels * (5 + 1)), 'normal_consistency_backward': floor(4 * pixels * (5 + 1 + 5))}
        entry['kernel_pairs'] = dict(summary(t), traffic_floor_ms=floors, fraction_of_hbm_peak={k: floors[k] / med[k] for k in floors})
        print(f'{label} (a) surface features {med["surface_features"]:.4f} ms, backward {med["surface_features_backward"]:.4f} ms (N = {n}); '
              f'(b) normal consistency {med["normal_consistency"]:.4f} ms, backward {med["normal_consistency_backward"]:.4f} ms; '
              f'fractions of the HBM peak {({k: round(floors[k] / med[k], 3) for k in floors})}', flush=True)
        del feats0, map0, E0, gF, gE

        # ---- (c) one composed call, forward + backward ----
        def clear():
            for x in leaves:
                x.grad = None

        def op_plain(v, RS, gC):
            (B.diff_rasterize(*leaves, none, RS) * gC).sum().backward()
            clear()

        def op_features_only(v, RS, gC):
            image, fmap = B.diff_rasterize_features(*leaves, none, RS, torch.ones((n, 5), device=dev))
            ((image * gC).sum() + fmap.mean()).backward()
            clear()

        def op_fused(v, RS, gC):
            feats = B.gaussian_surface_features(leaves[0], leaves[1], leaves[2], v.w2c, v.position)
            image, surface_map = B.diff_rasterize_features(*leaves, none, RS, feats)
            ((image * gC).sum() + B.normal_consistency(surface_map, RS).mean()).backward()
            clear()

        def op_torch(v, RS, gC):
            feats = torch_surface_features(leaves[0], leaves[1], leaves[2], v.w2c, v.position)
            image, surface_map = B.diff_rasterize_features(*leaves, none, RS, feats)
            ((image * gC).sum() + torch_normal_consistency(surface_map, v.focal_x, v.focal_y, v.center_x, v.center_y).mean()).backward()
            clear()
        t = per_view(timed_rounds({'diff_rasterize': over_views(op_plain), 'feature_render_5_channels': over_views(op_features_only),
                                   'fused_operators': over_views(op_fused), 'torch_restatements': over_views(op_torch)}, args.rounds, args.reps, args.warmup))
        med = {k: statistics.median(v) for k, v in t.items()}
        entry['operator'] = dict(summary(t), fused_minus_feature_render_ms=med['fused_operators'] - med['feature_render_5_channels'],
                                 torch_minus_feature_render_ms=med['torch_restatements'] - med['feature_render_5_channels'],
                                 fused_minus_plain_ms=med['fused_operators'] - med['diff_rasterize'], torch_over_fused=med['torch_restatements'] / med['fused_operators'])
        print(f'{label} (c) diff_rasterize {med["diff_rasterize"]:.4f} ms, feature render alone {med["feature_render_5_channels"]:.4f} ms, with the fused operators '
              f'{med["fused_operators"]:.4f} ms, with the torch restatements {med["torch_restatements"]:.4f} ms: the two ends cost '
              f'{entry["operator"]["fused_minus_feature_render_ms"]:+.4f} ms fused, {entry["operator"]["torch_minus_feature_render_ms"]:+.4f} ms in torch', flush=True)

        # ---- (e) the plain pass of this tree against the parent commit's library ----
        if parent is not None:
            entry['plain_pass_vs_parent'] = against_parent(lambda backend: over_views(through(backend, op_plain)))
            e = entry['plain_pass_vs_parent']
            print(f'{label} (e) diff_rasterize forward + backward: new - parent {e["new_minus_parent_ms"]:+.5f} ms, parent against itself '
                  f'{e["parent_self_spread_ms"]:.5f} ms, within: {e["within_margin"]}', flush=True)

        # ---- (d) the training iteration ----
        if label == 'S2':
            with torch.no_grad():
                targets = [T.render_image_training(g, v, False, v.background_color).clamp(0.0, 1.0) for v in views]

            def trainer_of(weight):
                m = T.Gaussians({k: v.clone() for k, v in params.items()}, dev)
                m.training_setup(training_cameras_extent=5.0)
                state = {'it': 0}

                def step():
                    for i, v in enumerate(views):
                        T.training_iteration(m, v, targets[i], state['it'], normal_weight=weight)
                        state['it'] += 1
                return step
            t = per_view(timed_rounds({'plain': trainer_of(0.0), 'plain_again': trainer_of(0.0), 'with_normals': trainer_of(args.weight)},
                                      args.rounds, args.reps, args.warmup))
            med = {k: statistics.median(v) for k, v in t.items()}
            entry['training_iteration'] = dict(summary(t), normal_weight=args.weight, normals_minus_plain_ms=med['with_normals'] - med['plain'],
                                               plain_again_minus_plain_ms=med['plain_again'] - med['plain'], plain_spread_ms=max(t['plain']) - min(t['plain']))
            print(f'{label} (d) training iteration {med["plain"]:.4f} ms, with the term {med["with_normals"]:.4f} ms '
                  f'({entry["training_iteration"]["normals_minus_plain_ms"]:+.4f}); plain_again - plain {entry["training_iteration"]["plain_again_minus_plain_ms"]:+.4f} ms, '
                  f'spread of the plain rounds {entry["training_iteration"]["plain_spread_ms"]:.4f} ms', flush=True)
            if parent is not None:
                entry['training_iteration_vs_parent'] = against_parent(lambda backend: through(backend, trainer_of(0.0)))
                e = entry['training_iteration_vs_parent']
                print(f'{label} (e) plain training iteration: new - parent {e["new_minus_parent_ms"]:+.5f} ms, parent against itself '
                      f'{e["parent_self_spread_ms"]:.5f} ms, within: {e["within_margin"]}', flush=True)
            del targets
        result['scenes'][label] = entry
        del passes, g, p, leaves
        torch.cuda.empty_cache()

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
