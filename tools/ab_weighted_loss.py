"""What does the per-pixel weight of the fused L1 + DSSIM loss cost, and did adding it move the unweighted kernels? At 1920x1080, in ONE process,
alternating: every timed block is `--reps` calls between two HIP events on the stream, after a warm-up; the variants take turns inside every round,
so drift of the box hits all alike. Reported: the median over the rounds (min / max).

(a) unweighted forward (l1_dssim_forward), backward (l1_dssim_backward) and one call (l1_dssim) through --parent-library (a libfgs_hip.so built from the
    parent commit), through the SAME parent library a second time, and through this tree's library. The margin is what the parent shows against itself:
    the largest per-round |parent_again - parent|. This tree's median per-round difference to the parent must lie within it (recorded, `within_margin`).
(b) the weighted calls of this tree for all-ones weights, a half-image binary mask and random weights, in the same rounds as (a).
(c) the two designs for S in the weighted one call: every backward workgroup re-sums the tiles' weight sums (FGS_LOSS_WEIGHTED_RESUM=1, the product) against
    a separate ssim_reduce_kernel launch (--separate-reduce-library: `bash tools/build_variant.sh wsep loss.hip -DFGS_LOSS_WEIGHTED_RESUM=0`).
(d) harness.trainer.training_iteration over the S2 orbit views without and with loss_weight (the half-image mask), two plain variants for the spread.
Writes profiles/weighted_loss_ab.json (or --out). Differences are recorded, not gated."""
import argparse
import ctypes as C
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
    return {k: {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v), 'ms_rounds': [round(x, 5) for x in v]} for k, v in times.items()}


def bind_partial(_lib, path):
    """A library that lacks the entry points this tree adds (the parent commit's): bind what it has."""
    lib = C.CDLL(str(path))
    for name, (restype, argtypes) in _lib._SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--reps', type=int, default=50, help='loss calls per timed block')
    ap.add_argument('--step-reps', type=int, default=2, help='passes over the views per timed block of training iterations')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--size', type=int, nargs=2, default=[1920, 1080], metavar=('W', 'H'))
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--parent-library', default='', help='libfgs_hip.so of the parent commit: (a)')
    ap.add_argument('--separate-reduce-library', default='', help='this tree built with -DFGS_LOSS_WEIGHTED_RESUM=0: (c)')
    ap.add_argument('--skip-training', action='store_true', help='leave (d) out')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'weighted_loss_ab.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ab_weighted_loss.py measures on the GPU; none is visible')

    from FasterGSCudaBackend import _backend, _lib
    dev = torch.device('cuda:0')
    be = _backend.default_backend()
    w, h = args.size
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(3, h, w, generator=gen).to(dev)
    y = (x.cpu() + 0.1 * torch.randn(3, h, w, generator=gen)).clamp(0, 1).to(dev)
    half = torch.ones(h, w)
    half[:, w // 2:] = 0.0
    weights = {'ones': torch.ones(h, w, device=dev), 'half_mask': half.to(dev), 'random': (2.0 * torch.rand(h, w, generator=gen)).to(dev)}
    result = {'what': f'fused L1 + DSSIM loss with and without per-pixel weights, {w}x{h}; medians over alternating rounds of HIP-event-timed blocks',
              'device': torch.cuda.get_device_name(dev), 'box': os.uname().nodename, 'library': be.lib.fgs_build_info().decode(),
              'rounds': args.rounds, 'reps': args.reps}

    def calls(backend, weight=None):
        kw = {} if weight is None else {'weight': weight}
        _, _, scratch = backend.l1_dssim_forward(x, y, **kw)
        return {'forward': lambda: backend.l1_dssim_forward(x, y, **kw), 'backward': lambda: backend.l1_dssim_backward(x, y, scratch, **kw),
                'one_call': lambda: backend.l1_dssim(x, y, **kw)}

    # ---- (a) + (b): one set of rounds ----
    sets = {'new_unweighted': calls(be)}
    sets.update({'new_weighted_' + k: calls(be, v) for k, v in weights.items()})
    if args.parent_library:
        sets['parent'] = calls(_backend.Backend(bind_partial(_lib, args.parent_library)))
        sets['parent_again'] = calls(_backend.Backend(bind_partial(_lib, args.parent_library)))
    result['loss_calls'] = {}
    for form in ('forward', 'backward', 'one_call'):
        t = timed_rounds({k: v[form] for k, v in sets.items()}, args.rounds, args.reps, args.warmup)
        entry = {'ms': summary(t)}
        med = {k: statistics.median(v) for k, v in t.items()}
        for k in weights:
            entry[f'weighted_{k}_minus_unweighted_ms'] = med['new_weighted_' + k] - med['new_unweighted']
        if args.parent_library:
            margin = max(abs(a - b) for a, b in zip(t['parent_again'], t['parent']))
            diff = statistics.median(a - b for a, b in zip(t['new_unweighted'], t['parent']))
            entry.update(parent_self_spread_ms=margin, new_minus_parent_ms=diff, within_margin=abs(diff) <= margin)
        result['loss_calls'][form] = entry
        print(f'(a,b) {form:9s} ' + ', '.join(f'{k} {m:.4f}' for k, m in med.items()) +
              (f'; new - parent {entry["new_minus_parent_ms"]:+.5f} ms, parent against itself {entry["parent_self_spread_ms"]:.5f} ms' if args.parent_library else ''), flush=True)

    # ---- (c) the two designs for S ----
    if args.separate_reduce_library:
        sep = _backend.Backend(_lib.bind(args.separate_reduce_library))
        a, b = be.l1_dssim(x, y, weight=weights['random']), sep.l1_dssim(x, y, weight=weights['random'])
        same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        t = timed_rounds({'resum_in_backward': calls(be, weights['random'])['one_call'], 'separate_reduce_launch': calls(sep, weights['random'])['one_call']},
                         args.rounds, args.reps, args.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        result['total_weight_designs'] = {'ms': summary(t), 'separate_minus_resum_ms': med['separate_reduce_launch'] - med['resum_in_backward'], 'same_bits': same}
        print(f'(c) weighted one call: re-sum in every backward workgroup {med["resum_in_backward"]:.4f} ms, separate reduce launch '
              f'{med["separate_reduce_launch"]:.4f} ms; same bits: {same}', flush=True)

    # ---- (d) the training iteration without and with loss_weight ----
    if not args.skip_training:
        import bench
        from harness import trainer as T
        argv, sys.argv = sys.argv, ['bench.py'] + (['--n-gaussians', str(args.n_gaussians)] if args.n_gaussians else [])
        params, views, what = bench.build_scene(bench.parse())
        sys.argv = argv
        views = [v.to(dev) for v in views]
        truth = T.Gaussians(params, dev)
        with torch.no_grad():
            targets = [T.render_image_training(truth, v, False, v.background_color).clamp(0.0, 1.0) for v in views]
        del truth
        mask = torch.ones(views[0].height, views[0].width, device=dev)
        mask[:, views[0].width // 2:] = 0.0

        def trainer_of(weight):
            g = T.Gaussians({k: v.clone() for k, v in params.items()}, dev)
            g.training_setup(training_cameras_extent=5.0)
            state = {'it': 0}

            def step():
                for i, v in enumerate(views):
                    T.training_iteration(g, v, targets[i], state['it'], loss_weight=weight)
                    state['it'] += 1
            return step
        t = timed_rounds({'plain': trainer_of(None), 'plain_again': trainer_of(None), 'with_loss_weight': trainer_of(mask)}, min(args.rounds, 9), args.step_reps, args.warmup)
        per_iter = {k: [v / len(views) for v in vs] for k, vs in t.items()}
        med = {k: statistics.median(v) for k, v in per_iter.items()}
        result['training_iteration'] = {'scene': what, 'ms_per_iteration': summary(per_iter), 'weighted_minus_plain_ms': med['with_loss_weight'] - med['plain'],
                                        'plain_again_minus_plain_ms': med['plain_again'] - med['plain'],
                                        'plain_spread_ms': max(per_iter['plain']) - min(per_iter['plain'])}
        print('(d) ' + ', '.join(f'{k} {m:.4f} ms' for k, m in med.items()), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
