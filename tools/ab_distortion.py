"""What does the depth-distortion regulariser cost, and did adding it move the plain pass? On S2 and on layered S2 (every opacity logit lowered by 3:
deep semi-transparent lists) at 1920x1080, in ONE process, alternating: every timed block is `--reps` passes over the orbit views between two HIP
events on the stream, after a warm-up; the variants take turns inside every round, so drift of the box hits all alike. Reported: the median over the
rounds of ms per view (min / max), and differences next to the spread of the rounds.

(a) the passes through the backend: `forward` alone and `forward` + `blend_distortion` (the difference is the forward kernel); `backward` and
    `backward_distortion` over the same buffers (the difference is the backward kernel, the clear of dL/dz and the depth term of the means).
(b) one operator call, forward + backward: diff_rasterize_distortion with a loss on the image and the map against diff_rasterize.
(c) the S2 training iteration (harness.trainer.training_iteration over the views) without the term, without it a second time (A/A: the spread), and
    with distortion_weight > 0.
(d) with --parent-library (a libfgs_hip.so built from the parent commit): diff_rasterize forward + backward through this tree's library, through the
    parent's, and through the parent's a second time. The margin is what the parent shows against itself, the largest per-round
    |parent_again - parent|; this tree's median per-round difference to the parent must lie within it (recorded, `within_margin`).
Writes profiles/distortion_ab.json (or --out). No cost is fixed in advance; (d) is the one condition."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=2, help='passes over the views per timed block')
    ap.add_argument('--warmup', type=int, default=1, help='untimed passes over the views per variant')
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--weight', type=float, default=100.0, help='distortion_weight of the training iteration of (c)')
    ap.add_argument('--parent-library', default='', help='libfgs_hip.so of the parent commit: (d)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'distortion_ab.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ab_distortion.py measures on the GPU; none is visible')

    import bench
    import FasterGSCudaBackend as B
    from FasterGSCudaBackend import _backend, _lib
    from harness import trainer as T
    dev = torch.device('cuda:0')
    be = _backend.default_backend()
    parent = [_backend.Backend(bind_partial(_lib, args.parent_library)) for _ in range(2)] if args.parent_library else None
    none = torch.empty(0)
    result = {'what': 'depth-distortion regulariser, 1920x1080, normalized mode; ms per view, medians over alternating rounds of HIP-event-timed blocks',
              'device': torch.cuda.get_device_name(dev), 'box': os.uname().nodename, 'library': be.lib.fgs_build_info().decode(),
              'rounds': args.rounds, 'scenes': {}}

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
            gX = torch.randn((v.height, v.width), generator=gen).to(dev) / (v.height * v.width)
            res = be.forward(*p, RS)
            passes.append((RS, gC, gX, res, be.blend_distortion(p[0], res, n, RS)))
        over_views = lambda fn: (lambda: [fn(*q) for q in passes] and None)
        per_view = lambda times: {k: [x / len(passes) for x in v] for k, v in times.items()}
        entry = {'scene': what + (f', opacity logits {shift:+.1f}' if shift else ''), 'views': len(passes), 'instances_view0': passes[0][3].state[1]}
        with torch.no_grad():
            entry['distortion_mean_view0'] = float(passes[0][4][0].mean())

        # ---- (a) the passes through the backend ----
        def fwd_plain(RS, gC, gX, res, st):
            be.forward(*p, RS)

        def fwd_dist(RS, gC, gX, res, st):
            be.blend_distortion(p[0], be.forward(*p, RS), n, RS)

        def bwd_plain(RS, gC, gX, res, st):
            be.backward(None, gC, res.image, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)

        def bwd_dist(RS, gC, gX, res, st):
            be.backward_distortion(None, gC, gX, res.image, st, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
        t = per_view(timed_rounds({'forward': over_views(fwd_plain), 'forward_with_distortion': over_views(fwd_dist), 'backward': over_views(bwd_plain),
                                   'backward_with_distortion': over_views(bwd_dist)}, args.rounds, args.reps, args.warmup))
        med = {k: statistics.median(v) for k, v in t.items()}
        entry['passes'] = dict(summary(t), forward_blend_ms=med['forward_with_distortion'] - med['forward'],
                               backward_blend_ms=med['backward_with_distortion'] - med['backward'])
        print(f'{label} (a) forward {med["forward"]:.4f} ms, with the distortion blend {med["forward_with_distortion"]:.4f} ms '
              f'({entry["passes"]["forward_blend_ms"]:+.4f}); backward {med["backward"]:.4f} ms, with the distortion term {med["backward_with_distortion"]:.4f} ms '
              f'({entry["passes"]["backward_blend_ms"]:+.4f})', flush=True)

        # ---- (b) one operator call ----
        def clear():
            for x in leaves:
                x.grad = None

        def op_plain(RS, gC, gX, res, st):
            (B.diff_rasterize(*leaves, none, RS) * gC).sum().backward()
            clear()

        def op_dist(RS, gC, gX, res, st):
            image, dmap = B.diff_rasterize_distortion(*leaves, none, RS)
            ((image * gC).sum() + (dmap * gX).sum()).backward()
            clear()
        t = per_view(timed_rounds({'diff_rasterize': over_views(op_plain), 'diff_rasterize_distortion': over_views(op_dist)}, args.rounds, args.reps, args.warmup))
        med = {k: statistics.median(v) for k, v in t.items()}
        entry['operator'] = dict(summary(t), distortion_minus_plain_ms=med['diff_rasterize_distortion'] - med['diff_rasterize'],
                                 distortion_over_plain=med['diff_rasterize_distortion'] / med['diff_rasterize'])
        print(f'{label} (b) diff_rasterize {med["diff_rasterize"]:.4f} ms, diff_rasterize_distortion {med["diff_rasterize_distortion"]:.4f} ms '
              f'({entry["operator"]["distortion_minus_plain_ms"]:+.4f}, x{entry["operator"]["distortion_over_plain"]:.3f})', flush=True)

        # ---- (d) the plain pass of this tree against the parent commit's library ----
        if parent is not None:
            def through(backend):
                def run(RS, gC, gX, res, st):
                    saved, _backend._DEFAULT = _backend._DEFAULT, backend          # the operator asks default_backend()
                    try:
                        op_plain(RS, gC, gX, res, st)
                    finally:
                        _backend._DEFAULT = saved
                return over_views(run)
            t = per_view(timed_rounds({'parent': through(parent[0]), 'new': through(be), 'parent_again': through(parent[1])}, args.rounds, args.reps, args.warmup))
            margin = max(abs(a - b) for a, b in zip(t['parent_again'], t['parent']))
            diff = statistics.median(a - b for a, b in zip(t['new'], t['parent']))
            entry['plain_pass_vs_parent'] = dict(summary(t), parent_self_spread_ms=margin, new_minus_parent_ms=diff, within_margin=abs(diff) <= margin)
            print(f'{label} (d) diff_rasterize forward + backward: new - parent {diff:+.5f} ms, parent against itself {margin:.5f} ms, within: {abs(diff) <= margin}', flush=True)

        # ---- (c) the training iteration ----
        if label == 'S2':
            with torch.no_grad():
                targets = [T.render_image_training(g, v, False, v.background_color).clamp(0.0, 1.0) for v in views]

            def trainer_of(weight):
                m = T.Gaussians({k: v.clone() for k, v in params.items()}, dev)
                m.training_setup(training_cameras_extent=5.0)
                state = {'it': 0}

                def step():
                    for i, v in enumerate(views):
                        T.training_iteration(m, v, targets[i], state['it'], distortion_weight=weight)
                        state['it'] += 1
                return step
            t = per_view(timed_rounds({'plain': trainer_of(0.0), 'plain_again': trainer_of(0.0), 'with_distortion': trainer_of(args.weight)},
                                      args.rounds, args.reps, args.warmup))
            med = {k: statistics.median(v) for k, v in t.items()}
            entry['training_iteration'] = dict(summary(t), distortion_weight=args.weight, distortion_minus_plain_ms=med['with_distortion'] - med['plain'],
                                               plain_again_minus_plain_ms=med['plain_again'] - med['plain'], plain_spread_ms=max(t['plain']) - min(t['plain']))
            print(f'{label} (c) training iteration {med["plain"]:.4f} ms, with the term {med["with_distortion"]:.4f} ms '
                  f'({entry["training_iteration"]["distortion_minus_plain_ms"]:+.4f}); plain_again - plain {entry["training_iteration"]["plain_again_minus_plain_ms"]:+.4f} ms, '
                  f'spread of the plain rounds {entry["training_iteration"]["plain_spread_ms"]:.4f} ms', flush=True)
            del targets
        result['scenes'][label] = entry
        del passes, g, p, leaves
        torch.cuda.empty_cache()

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
