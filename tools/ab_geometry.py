"""What does the one render of the geometry terms (diff_rasterize_geometry: distortion + surface map in one walk) cost against the two renders it
replaces, and did adding it move the plain pass? On S2 and on layered S2 (every opacity logit lowered by 3: deep semi-transparent lists) at 1920x1080,
in ONE process, alternating: every timed block is `--reps` passes over the orbit views between two HIP events on the stream, after a warm-up; the
variants take turns inside every round, so drift of the box hits all alike. Reported: the median over the rounds of ms per view (min / max), and
differences next to the spread of the rounds. The method is tools/ab_distortion.py's.

(a) the passes through the backend over one forward pass's buffers: blend_geometry against blend_distortion + blend_features (F = 5), and
    backward_geometry against backward_distortion + backward_features (the two K11 / K12 passes a caller of both operators pays today).
(b) one operator call, forward + backward, with a loss on the image, the distortion map and the surface map: diff_rasterize_geometry against
    diff_rasterize_distortion + diff_rasterize_features (two full renders), and diff_rasterize for scale.
(c) the S2 training iteration (harness.trainer.training_iteration over the views): plain, plain again (A/A: the spread), geometry_render=True with the
    distortion and the normal term, and each term by its own render as it was (distortion_weight alone, normal_weight alone).
(d) with --parent-library (a libfgs_hip.so built from the parent commit): diff_rasterize forward + backward through this tree's library, through the
    parent's, and through the parent's a second time. The margin is what the parent shows against itself, the largest per-round
    |parent_again - parent|; this tree's median per-round difference to the parent must lie within it (recorded, `within_margin`).
Writes profiles/geometry_ab.json (or --out). No cost is fixed in advance; (d) is the one condition."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / 'faster-gaussian-splatting_amd'), str(ROOT / 'tools')]

from ab_distortion import bind_partial, summary, timed_rounds  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=2, help='passes over the views per timed block')
    ap.add_argument('--warmup', type=int, default=1, help='untimed passes over the views per variant')
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--distortion-weight', type=float, default=100.0)
    ap.add_argument('--normal-weight', type=float, default=0.05)
    ap.add_argument('--parent-library', default='', help='libfgs_hip.so of the parent commit: (d)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'geometry_ab.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ab_geometry.py measures on the GPU; none is visible')

    import bench
    import FasterGSCudaBackend as B
    from FasterGSCudaBackend import _backend, _lib
    from harness import trainer as T
    dev = torch.device('cuda:0')
    be = _backend.default_backend()
    parent = [_backend.Backend(bind_partial(_lib, args.parent_library)) for _ in range(2)] if args.parent_library else None
    none = torch.empty(0)
    result = {'what': 'one render for distortion + surface map, 1920x1080, normalized mode; ms per view, medians over alternating rounds of HIP-event-timed blocks',
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
            gM = torch.randn((5, v.height, v.width), generator=gen).to(dev) / (5 * v.height * v.width)
            fe = be.surface_features(p[0], p[1], p[2], v.w2c, v.position)
            res = be.forward(*p, RS)
            passes.append({'RS': RS, 'gC': gC, 'gX': gX, 'gM': gM, 'fe': fe, 'res': res, 'gstate': be.blend_geometry(p[0], fe, res, n, RS),
                           'dstate': be.blend_distortion(p[0], res, n, RS), 'fmap': be.blend_features(fe, res, n, RS)})
        over_views = lambda fn: (lambda: [fn(q) for q in passes] and None)
        per_view = lambda times: {k: [x / len(passes) for x in v] for k, v in times.items()}
        entry = {'scene': what + (f', opacity logits {shift:+.1f}' if shift else ''), 'views': len(passes), 'instances_view0': passes[0]['res'].state[1]}

        # ---- (a) the passes through the backend ----
        def fwd_one(q):
            be.blend_geometry(p[0], q['fe'], q['res'], n, q['RS'])

        def fwd_two(q):
            be.blend_distortion(p[0], q['res'], n, q['RS'])
            be.blend_features(q['fe'], q['res'], n, q['RS'])

        def bwd_one(q):
            r = q['res']
            be.backward_geometry(None, q['gC'], q['gX'], q['gM'], r.image, q['gstate'], q['fe'], p[0], p[1], p[2], p[3], p[5], r.buffers, q['RS'], r.state)

        def bwd_two(q):
            r = q['res']
            be.backward_distortion(None, q['gC'], q['gX'], r.image, q['dstate'], p[0], p[1], p[2], p[3], p[5], r.buffers, q['RS'], r.state)
            be.backward_features(None, q['gC'], q['gM'], r.image, q['fmap'], q['fe'], p[0], p[1], p[2], p[3], p[5], r.buffers, q['RS'], r.state)

        def bwd_plain(q):
            r = q['res']
            be.backward(None, q['gC'], r.image, p[0], p[1], p[2], p[3], p[5], r.buffers, q['RS'], r.state)
        t = per_view(timed_rounds({'blend_geometry': over_views(fwd_one), 'blend_distortion_plus_blend_features': over_views(fwd_two),
                                   'backward': over_views(bwd_plain), 'backward_geometry': over_views(bwd_one),
                                   'backward_distortion_plus_backward_features': over_views(bwd_two)}, args.rounds, args.reps, args.warmup))
        med = {k: statistics.median(v) for k, v in t.items()}
        entry['passes'] = dict(summary(t), forward_one_minus_two_ms=med['blend_geometry'] - med['blend_distortion_plus_blend_features'],
                               backward_one_minus_two_ms=med['backward_geometry'] - med['backward_distortion_plus_backward_features'],
                               backward_walk_ms=med['backward_geometry'] - med['backward'])
        print(f'{label} (a) blend_geometry {med["blend_geometry"]:.4f} ms against the two blends {med["blend_distortion_plus_blend_features"]:.4f} ms; '
              f'backward_geometry {med["backward_geometry"]:.4f} ms (plain backward {med["backward"]:.4f} ms) against the two backward passes '
              f'{med["backward_distortion_plus_backward_features"]:.4f} ms', flush=True)

        # ---- (b) one operator call ----
        def clear():
            for x in leaves:
                x.grad = None

        def op_plain(q):
            (B.diff_rasterize(*leaves, none, q['RS']) * q['gC']).sum().backward()
            clear()

        def op_one(q):
            image, dmap, smap = B.diff_rasterize_geometry(*leaves, none, q['RS'], q['fe'])
            ((image * q['gC']).sum() + (dmap * q['gX']).sum() + (smap * q['gM']).sum()).backward()
            clear()

        def op_two(q):
            image, dmap = B.diff_rasterize_distortion(*leaves, none, q['RS'])
            _, smap = B.diff_rasterize_features(*leaves, none, q['RS'], q['fe'])
            ((image * q['gC']).sum() + (dmap * q['gX']).sum() + (smap * q['gM']).sum()).backward()
            clear()
        t = per_view(timed_rounds({'diff_rasterize': over_views(op_plain), 'diff_rasterize_geometry': over_views(op_one),
                                   'diff_rasterize_distortion_plus_features': over_views(op_two)}, args.rounds, args.reps, args.warmup))
        med = {k: statistics.median(v) for k, v in t.items()}
        entry['operator'] = dict(summary(t), one_minus_two_ms=med['diff_rasterize_geometry'] - med['diff_rasterize_distortion_plus_features'],
                                 one_over_two=med['diff_rasterize_geometry'] / med['diff_rasterize_distortion_plus_features'],
                                 one_over_plain=med['diff_rasterize_geometry'] / med['diff_rasterize'])
        print(f'{label} (b) diff_rasterize {med["diff_rasterize"]:.4f} ms, diff_rasterize_geometry {med["diff_rasterize_geometry"]:.4f} ms, the two operators it '
              f'replaces {med["diff_rasterize_distortion_plus_features"]:.4f} ms (x{entry["operator"]["one_over_two"]:.3f})', flush=True)

        # ---- (d) the plain pass of this tree against the parent commit's library ----
        if parent is not None:
            def through(backend):
                def run(q):
                    saved, _backend._DEFAULT = _backend._DEFAULT, backend          # the operator asks default_backend()
                    try:
                        op_plain(q)
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

            def trainer_of(**kw):
                m = T.Gaussians({k: v.clone() for k, v in params.items()}, dev)
                m.training_setup(training_cameras_extent=5.0)
                state = {'it': 0}

                def step():
                    for i, v in enumerate(views):
                        T.training_iteration(m, v, targets[i], state['it'], **kw)
                        state['it'] += 1
                return step
            dw, nw = args.distortion_weight, args.normal_weight
            t = per_view(timed_rounds({'plain': trainer_of(), 'plain_again': trainer_of(),
                                       'geometry_render_both_terms': trainer_of(geometry_render=True, distortion_weight=dw, normal_weight=nw),
                                       'distortion_alone': trainer_of(distortion_weight=dw), 'normals_alone': trainer_of(normal_weight=nw)},
                                      args.rounds, args.reps, args.warmup))
            med = {k: statistics.median(v) for k, v in t.items()}
            entry['training_iteration'] = dict(summary(t), distortion_weight=dw, normal_weight=nw, both_minus_plain_ms=med['geometry_render_both_terms'] - med['plain'],
                                               distortion_minus_plain_ms=med['distortion_alone'] - med['plain'], normals_minus_plain_ms=med['normals_alone'] - med['plain'],
                                               plain_again_minus_plain_ms=med['plain_again'] - med['plain'], plain_spread_ms=max(t['plain']) - min(t['plain']))
            print(f'{label} (c) training iteration {med["plain"]:.4f} ms, with both terms in one render {med["geometry_render_both_terms"]:.4f} ms, distortion alone '
                  f'{med["distortion_alone"]:.4f} ms, normals alone {med["normals_alone"]:.4f} ms; plain_again - plain '
                  f'{entry["training_iteration"]["plain_again_minus_plain_ms"]:+.4f} ms', flush=True)
            del targets
        result['scenes'][label] = entry
        del passes, g, p, leaves
        torch.cuda.empty_cache()

    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
