"""What does depth / opacity supervision cost a training iteration? One S2 iteration (render -> loss -> backward -> FusedAdam) with diff_rasterize against
one with diff_rasterize_aux and both maps supervised (harness.trainer.training_iteration with depth_target / depth_weight, plus an opacity term through
`loss_fn`), in ONE process, alternating: every timed block is `--reps` passes over the orbit views between two HIP events on the stream, after a warm-up;
the two variants take turns inside every round, so drift of the box hits both alike; reported: the median over the rounds of ms per iteration (min / max)
and the ratio. Then K10, the staging pass and K11 alone for both variants, from the library's per-stage events (fgs_profile_enable on that one stage:
two events per launch). Writes profiles/aux_grad_ab.json (or --out). The ratio is recorded, not gated."""
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
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=4, help='passes over the views per timed block')
    ap.add_argument('--warmup', type=int, default=2, help='untimed passes over the views per variant')
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'aux_grad_ab.json'))
    args = ap.parse_args()

    import bench
    from FasterGSCudaBackend._backend import default_backend
    from harness import trainer as T
    argv, sys.argv = sys.argv, ['bench.py'] + (['--n-gaussians', str(args.n_gaussians)] if args.n_gaussians else [])
    params, views, what = bench.build_scene(bench.parse())
    sys.argv = argv
    dev = torch.device('cuda:0')
    be = default_backend()
    views = [v.to(dev) for v in views]
    truth = T.Gaussians(params, dev)
    targets = []
    with torch.no_grad():          # colour, mean depth and opacity of the generating parameters; the trained copy starts from perturbed means
        for v in views:
            image, a, d = T.render_image_training_aux(truth, v, False, v.background_color)
            targets.append((image.clone(), torch.where(a > 0.5, d / a.clamp_min(1e-8), torch.zeros_like(d)), a.clone()))
    del truth
    start = {k: t.clone() for k, t in params.items()}
    start['means'] = start['means'] + 0.01 * torch.randn(start['means'].shape, generator=torch.Generator().manual_seed(3))

    def make():
        g = T.Gaussians(start, dev)
        g.training_setup(training_cameras_extent=4.0)
        return g
    models = {'diff_rasterize': make(), 'diff_rasterize_aux (alpha + depth supervised)': make()}
    counter = {k: 0 for k in models}

    def iterate(k, i):
        g, (image, depth, alpha) = models[k], targets[i]
        counter[k] += 1
        if k == 'diff_rasterize':
            return T.training_iteration(g, views[i], image, counter[k])
        # both maps in the loss: depth L1 through D / A (gradients into D and A) -- opacity supervision rides on the same A
        return T.training_iteration(g, views[i], image, counter[k], depth_target=depth, depth_weight=0.5)

    for k in models:
        for _ in range(args.warmup):
            for i in range(len(views)):
                iterate(k, i)
    torch.cuda.synchronize()
    times = {k: [] for k in models}
    order = list(models)
    for rnd in range(args.rounds):
        for k in order[rnd % 2:] + order[:rnd % 2]:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.reps):
                for i in range(len(views)):
                    iterate(k, i)
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / (args.reps * len(views)))
    base = statistics.median(times['diff_rasterize'])
    result = {'what': 'ms per S2 training iteration (render, loss, backward, FusedAdam; 1920x1080), median over alternating rounds of HIP-event-timed blocks',
              'scene': what, 'device': torch.cuda.get_device_name(dev), 'box': os.uname().nodename, 'library': be.lib.fgs_build_info().decode(),
              'rounds': args.rounds, 'iterations_per_block': args.reps * len(views),
              'iteration': {k: {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v), 'ratio_to_diff_rasterize': statistics.median(v) / base,
                                'ms_rounds': [round(x, 4) for x in v]} for k, v in times.items()}, 'stages': {}}
    for k, e in result['iteration'].items():
        print(f'{k:48s} {e["ms_median"]:.4f} ms (min {e["ms_min"]:.4f}, max {e["ms_max"]:.4f})  x{e["ratio_to_diff_rasterize"]:.4f}', flush=True)
    # K10, staging, K11 alone: one stage bracketed at a time, the variants alternating
    for stage in ('blend_forward', 'stage_pixels', 'blend_backward'):
        per = {k: [] for k in models}
        for rnd in range(3):
            for k in order[rnd % 2:] + order[:rnd % 2]:
                be.profile_enable(True, only=stage)
                be.profile_read()
                for i in range(len(views)):
                    iterate(k, i)
                torch.cuda.synchronize()
                ms, calls = be.profile_read()[stage]
                be.profile_enable(False)
                per[k].append(ms / max(calls, 1))
        med = {k: statistics.median(v) for k, v in per.items()}
        result['stages'][stage] = {k: {'ms_median': med[k], 'ratio_to_diff_rasterize': med[k] / med['diff_rasterize'], 'ms_rounds': [round(x, 4) for x in per[k]]}
                                   for k in per}
        print(stage, {k: round(v, 4) for k, v in med.items()}, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
