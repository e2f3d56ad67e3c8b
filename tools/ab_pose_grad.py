"""What do the camera-pose gradients cost a backward pass? On S2, over the forward buffers of every orbit view, `Backend.backward` with a
reached_blocks array (fgs_backward_reached) against `Backend.backward_pose` (fgs_backward_pose: K12 with the POSE flag + the two reduction kernels), in
ONE process, alternating: every timed block is `--reps` passes over the views between two HIP events on the stream, after a warm-up; the two take
turns inside every round, so drift of the box hits both alike. Reported: the median over the rounds of ms per backward pass (min / max) and the
difference; then the K12 stage alone for both (the library's per-stage events on `preprocess_backward`, which bracket the reduction kernels too).
Writes profiles/pose_grad_ab.json (or --out). The difference is recorded, not gated."""
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
    ap.add_argument('--reps', type=int, default=4, help='passes over the views per timed block')
    ap.add_argument('--warmup', type=int, default=2, help='untimed passes over the views per variant')
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'pose_grad_ab.json'))
    args = ap.parse_args()

    import bench
    from FasterGSCudaBackend._backend import default_backend
    from harness import trainer as T
    argv, sys.argv = sys.argv, ['bench.py'] + (['--n-gaussians', str(args.n_gaussians)] if args.n_gaussians else [])
    params, views, what = bench.build_scene(bench.parse())
    sys.argv = argv
    dev = torch.device('cuda:0')
    be = default_backend()
    g = T.Gaussians(params, dev)
    p = [t.detach() for t in g.tensors()]
    n = p[0].shape[0]
    passes = []
    for v in views:                  # one forward pass per view; both variants differentiate the same buffers, again and again
        v = v.to(dev)
        RS = T.extract_settings(v, g.active_sh_bases, v.background_color)
        res = be.forward(*p, RS)
        gi = ((res.image - 0.5) / res.image.numel()).contiguous()
        passes.append((RS, res, gi))
    out = tuple(torch.empty(sh, dtype=torch.float32, device=dev) for sh in ((n, 3), (n, 3), (n, 4), (n, 1), (n, 1, 3), (n, p[5].shape[1], 3)))
    flags = torch.empty((n + 63) // 64, dtype=torch.uint8, device=dev)

    def run(k, i):
        RS, res, gi = passes[i]
        tail = (res.image, p[0], p[1], p[2], p[3], p[5], res.buffers, RS, res.state)
        if k == 'backward_reached':
            return be.backward(None, gi, *tail, out=out, reached_blocks=flags)
        return be.backward_pose(None, gi, None, None, tail[0], None, *tail[1:], out=out, reached_blocks=flags)

    order = ['backward_reached', 'backward_pose']
    for k in order:
        for _ in range(args.warmup):
            for i in range(len(passes)):
                run(k, i)
    torch.cuda.synchronize()
    times = {k: [] for k in order}
    for rnd in range(args.rounds):
        for k in order[rnd % 2:] + order[:rnd % 2]:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.reps):
                for i in range(len(passes)):
                    run(k, i)
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / (args.reps * len(passes)))
    med = {k: statistics.median(v) for k, v in times.items()}
    result = {'what': 'ms per S2 backward pass (staging, K11, K12 [+ pose reduction]; 1920x1080), median over alternating rounds of HIP-event-timed blocks',
              'scene': what, 'device': torch.cuda.get_device_name(dev), 'box': os.uname().nodename, 'library': be.lib.fgs_build_info().decode(),
              'rounds': args.rounds, 'passes_per_block': args.reps * len(passes),
              'backward': {k: {'ms_median': med[k], 'ms_min': min(v), 'ms_max': max(v), 'ms_rounds': [round(x, 4) for x in v]} for k, v in times.items()},
              'pose_minus_reached_ms': med['backward_pose'] - med['backward_reached']}
    for k, e in result['backward'].items():
        print(f'{k:18s} {e["ms_median"]:.4f} ms (min {e["ms_min"]:.4f}, max {e["ms_max"]:.4f})', flush=True)
    print(f'backward_pose - backward_reached: {result["pose_minus_reached_ms"]:+.4f} ms', flush=True)
    per = {k: [] for k in order}
    for rnd in range(5):             # K12 alone (with the reduction kernels, for backward_pose): two events per launch of that one stage
        for k in order[rnd % 2:] + order[:rnd % 2]:
            be.profile_enable(True, only='preprocess_backward')
            be.profile_read()
            for i in range(len(passes)):
                run(k, i)
            torch.cuda.synchronize()
            ms, calls = be.profile_read()['preprocess_backward']
            be.profile_enable(False)
            per[k].append(ms / max(calls, 1))
    k12 = {k: statistics.median(v) for k, v in per.items()}
    result['k12_stage'] = {k: {'ms_median': k12[k], 'ms_rounds': [round(x, 4) for x in per[k]]} for k in order}
    result['k12_pose_minus_reached_ms'] = k12['backward_pose'] - k12['backward_reached']
    print('K12 stage', {k: round(v, 4) for k, v in k12.items()}, f'difference {result["k12_pose_minus_reached_ms"]:+.4f} ms', flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
