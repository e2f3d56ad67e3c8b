"""What does the absolute-gradient densification statistic cost a backward pass? On S2 and on the layered S2 (opacity logits - 3: deep lists, the
blend-bound regime), over the forward buffers of every orbit view, `Backend.backward` with a densification_info tensor (fgs_backward_recycled: the
plain pass) against `Backend.backward_absgrad` with an abs_densification_info tensor instead (fgs_backward_absgrad: K11 with the two extra sums, the
fold and the statistic kernel), in ONE process, alternating: every timed block is `--reps` passes over the views between two HIP events on the
stream, after a warm-up; the variants take turns inside every round, so drift of the box hits all alike. With --parent-library (a libfgs_hip.so built
from the parent commit) a third variant runs that library's plain pass over forward buffers of its own in the same rounds: the plain pass of this tree
must equal it within the spread of the rounds. Reported per scene: the median over the rounds of ms per backward pass (min / max), the differences,
then K11's own time for every variant (the library's per-stage events on `blend_backward`: K11 and its folds) and the staging pass's.
Writes profiles/absgrad_ab.json (or --out). The differences are recorded, not gated."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / 'faster-gaussian-splatting_amd')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=3, help='passes over the views per timed block')
    ap.add_argument('--warmup', type=int, default=2, help='untimed passes over the views per variant')
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--parent-library', default='', help='libfgs_hip.so of the parent commit: its plain backward pass joins the rounds')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'absgrad_ab.json'))
    args = ap.parse_args()

    import bench
    from FasterGSCudaBackend import _backend, _lib
    from harness import trainer as T
    argv, sys.argv = sys.argv, ['bench.py'] + (['--n-gaussians', str(args.n_gaussians)] if args.n_gaussians else [])
    params, views, what = bench.build_scene(bench.parse())
    sys.argv = argv
    dev = torch.device('cuda:0')
    backends = {'this': _backend.default_backend()}
    if args.parent_library:
        backends['parent'] = _backend.Backend(_bind_parent(_lib, args.parent_library))
    layered = dict(params)
    layered['opacities'] = params['opacities'] - 3.0
    result = {'what': 'ms per backward pass (staging, K11 + folds, K12 [+ the statistic kernel]; 1920x1080), median over alternating rounds of HIP-event-timed blocks',
              'scene': what, 'device': torch.cuda.get_device_name(dev), 'box': os.uname().nodename, 'library': backends['this'].lib.fgs_build_info().decode(),
              'rounds': args.rounds, 'scenes': {}}
    for scene_name, sp in (('S2', params), ('layered S2', layered)):
        g = T.Gaussians(sp, dev)
        p = [t.detach() for t in g.tensors()]
        n = p[0].shape[0]
        passes = {}
        for which, be in backends.items():      # one forward pass per view and library; the variants differentiate the same buffers, again and again
            passes[which] = []
            for v in views:
                v = v.to(dev)
                RS = T.extract_settings(v, g.active_sh_bases, v.background_color)
                res = be.forward(*p, RS)
                passes[which].append((RS, res, ((res.image - 0.5) / res.image.numel()).contiguous()))
        out = tuple(torch.empty(sh, dtype=torch.float32, device=dev) for sh in ((n, 3), (n, 3), (n, 4), (n, 1), (n, 1, 3), (n, p[5].shape[1], 3)))
        flags = torch.empty((n + 63) // 64, dtype=torch.uint8, device=dev)
        dens, info = torch.zeros(2, n, device=dev), torch.zeros(2, n, device=dev)

        def run(k, i):
            RS, res, gi = passes['parent' if k == 'parent_backward' else 'this'][i]
            tail = (res.image, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
            if k == 'backward_absgrad':
                return backends['this'].backward_absgrad(None, info, gi, None, None, tail[0], None, *tail[1:], out=out, reached_blocks=flags)
            return backends['parent' if k == 'parent_backward' else 'this'].backward(dens, gi, *tail, out=out, reached_blocks=flags)

        order = ['backward', 'backward_absgrad'] + (['parent_backward'] if 'parent' in backends else [])
        for k in order:
            for _ in range(args.warmup):
                for i in range(len(views)):
                    run(k, i)
        torch.cuda.synchronize()
        times = {k: [] for k in order}
        for rnd in range(args.rounds):
            shift = rnd % len(order)
            for k in order[shift:] + order[:shift]:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.reps):
                    for i in range(len(views)):
                        run(k, i)
                t1.record()
                t1.synchronize()
                times[k].append(t0.elapsed_time(t1) / (args.reps * len(views)))
        med = {k: statistics.median(v) for k, v in times.items()}
        entry = {'n_gaussians': n, 'passes_per_block': args.reps * len(views),
                 'backward': {k: {'ms_median': med[k], 'ms_min': min(v), 'ms_max': max(v), 'ms_rounds': [round(x, 4) for x in v]} for k, v in times.items()},
                 'absgrad_minus_plain_ms': med['backward_absgrad'] - med['backward'],
                 'plain_spread_ms': max(times['backward']) - min(times['backward'])}
        if 'parent' in backends:
            entry['plain_minus_parent_ms'] = med['backward'] - med['parent_backward']
        for k, e in entry['backward'].items():
            print(f'{scene_name:10s} {k:18s} {e["ms_median"]:.4f} ms (min {e["ms_min"]:.4f}, max {e["ms_max"]:.4f})', flush=True)
        print(f'{scene_name:10s} backward_absgrad - backward: {entry["absgrad_minus_plain_ms"]:+.4f} ms; spread of the plain rounds {entry["plain_spread_ms"]:.4f} ms'
              + (f'; backward - parent_backward: {entry["plain_minus_parent_ms"]:+.4f} ms' if 'parent' in backends else ''), flush=True)
        stage = {k: {'blend_backward': [], 'stage_pixels': []} for k in order}
        for rnd in range(5):             # K11 (with its folds) and the staging pass alone: two events per launch of that one stage
            for name in ('blend_backward', 'stage_pixels'):
                for k in order[rnd % len(order):] + order[:rnd % len(order)]:
                    be = backends['parent' if k == 'parent_backward' else 'this']
                    be.profile_enable(True, only=name)
                    be.profile_read()
                    for i in range(len(views)):
                        run(k, i)
                    torch.cuda.synchronize()
                    ms, calls = be.profile_read()[name]
                    be.profile_enable(False)
                    stage[k][name].append(ms / max(calls, 1))
        entry['stages'] = {k: {name: {'ms_median': statistics.median(v), 'ms_rounds': [round(x, 4) for x in v]} for name, v in d.items()} for k, d in stage.items()}
        entry['k11_absgrad_minus_plain_ms'] = entry['stages']['backward_absgrad']['blend_backward']['ms_median'] - entry['stages']['backward']['blend_backward']['ms_median']
        print(f'{scene_name:10s} K11 stage', {k: round(d['blend_backward']['ms_median'], 4) for k, d in entry['stages'].items()},
              f'difference {entry["k11_absgrad_minus_plain_ms"]:+.4f} ms; staging', {k: round(d['stage_pixels']['ms_median'], 4) for k, d in entry['stages'].items()}, flush=True)
        result['scenes'][scene_name] = entry
        del g, p, passes, out, dens, info
        torch.cuda.empty_cache()
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
