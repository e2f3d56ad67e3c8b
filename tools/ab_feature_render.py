"""What does a 16-channel feature render cost, against the formulation it replaces? On S2, forward + backward through the public operators over every
orbit view, three arms in ONE process, alternating:
  features_one_call : diff_rasterize_features with F = 16 (one forward pass, one feature blend, one backward pass), loss on the image and the map;
  six_passes        : the workaround on the same commit -- 6 diff_rasterize passes with active_sh_bases = 1 and three non-negative channels each
                      pushed through the colour path as sh0 = (f - 0.5) / C0, the geometry gradients summed by autograd;
  plain_one_pass    : one diff_rasterize pass, for scale.
Every timed block is `--reps` passes over the views between two HIP events on the stream, after a warm-up; the arms take turns inside every round, so
drift of the box hits all alike. Reported: the median over the rounds of ms per forward + backward (min / max) and the ratios; then, from the
library's per-stage events, what the two feature blends add to the blend_forward and blend_backward stages of a plain pass.
Writes profiles/feature_render_ab.json (or --out). The only bar: the one call takes less time than the six passes."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / 'faster-gaussian-splatting_amd')]

SH_C0 = 0.28209479177387814
CHANNELS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=2, help='passes over the views per timed block')
    ap.add_argument('--warmup', type=int, default=1, help='untimed passes over the views per arm')
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'feature_render_ab.json'))
    args = ap.parse_args()

    import bench
    import FasterGSCudaBackend as B
    from FasterGSCudaBackend._backend import default_backend
    from harness import trainer as T
    argv, sys.argv = sys.argv, ['bench.py'] + (['--n-gaussians', str(args.n_gaussians)] if args.n_gaussians else [])
    params, views, what = bench.build_scene(bench.parse())
    sys.argv = argv
    dev = torch.device('cuda:0')
    g = T.Gaussians(params, dev)
    leaves = [t.detach().clone().requires_grad_(True) for t in g.tensors()]
    n = leaves[0].shape[0]
    gen = torch.Generator().manual_seed(1)
    feats = torch.rand((n, CHANNELS), generator=gen).to(dev).requires_grad_(True)             # non-negative: the workaround clamps the rest away
    groups = (CHANNELS + 2) // 3
    padded = torch.cat([feats.detach(), feats.new_zeros((n, 3 * groups - CHANNELS))], dim=1)
    sh0_groups = [((padded[:, 3 * k:3 * k + 3] - 0.5) / SH_C0).reshape(n, 1, 3).contiguous().requires_grad_(True) for k in range(groups)]
    none = torch.empty(0)
    passes = []
    for v in views:
        v = v.to(dev)
        RS = T.extract_settings(v, g.active_sh_bases, v.background_color)
        RS1 = RS._replace(active_sh_bases=1, bg_color=torch.zeros(3, device=dev))
        gC = torch.randn((3, v.height, v.width), generator=gen).to(dev) / (3 * v.height * v.width)
        gF = torch.randn((3 * groups, v.height, v.width), generator=gen).to(dev) / (CHANNELS * v.height * v.width)
        passes.append((RS, RS1, gC, gF))

    def run(k, i):
        RS, RS1, gC, gF = passes[i]
        if k == 'features_one_call':
            image, fmap = B.diff_rasterize_features(*leaves, none, RS, feats)
            ((image * gC).sum() + (fmap * gF[:CHANNELS]).sum()).backward()
        elif k == 'six_passes':
            for j, sh0 in enumerate(sh0_groups):
                image = B.diff_rasterize(*leaves[:4], sh0, leaves[5], none, RS1)
                (image * gF[3 * j:3 * j + 3]).sum().backward()
        else:
            (B.diff_rasterize(*leaves, none, RS) * gC).sum().backward()
        for t in leaves + [feats] + sh0_groups:
            t.grad = None

    order = ['features_one_call', 'six_passes', 'plain_one_pass']
    for k in order:
        for _ in range(args.warmup):
            for i in range(len(passes)):
                run(k, i)
    torch.cuda.synchronize()
    times = {k: [] for k in order}
    for rnd in range(args.rounds):
        for k in order[rnd % 3:] + order[:rnd % 3]:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.reps):
                for i in range(len(passes)):
                    run(k, i)
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / (args.reps * len(passes)))
    med = {k: statistics.median(v) for k, v in times.items()}
    be = default_backend()
    result = {'what': f'ms per S2 forward + backward through the public operators (1920x1080, F = {CHANNELS}), median over alternating rounds of '
                      f'HIP-event-timed blocks',
              'scene': what, 'device': torch.cuda.get_device_name(dev), 'box': os.uname().nodename, 'library': be.lib.fgs_build_info().decode(),
              'rounds': args.rounds, 'passes_per_block': args.reps * len(passes), 'channels': CHANNELS, 'workaround_passes': groups,
              'forward_backward': {k: {'ms_median': med[k], 'ms_min': min(v), 'ms_max': max(v), 'ms_rounds': [round(x, 4) for x in v]}
                                   for k, v in times.items()},
              'one_call_over_six_passes': med['features_one_call'] / med['six_passes'],
              'one_call_over_plain_pass': med['features_one_call'] / med['plain_one_pass'],
              'one_call_is_faster_than_six_passes': med['features_one_call'] < med['six_passes']}
    for k, e in result['forward_backward'].items():
        print(f'{k:18s} {e["ms_median"]:.4f} ms (min {e["ms_min"]:.4f}, max {e["ms_max"]:.4f})', flush=True)
    print(f'one call / six passes: {result["one_call_over_six_passes"]:.3f}   one call / plain pass: {result["one_call_over_plain_pass"]:.3f}', flush=True)
    stages = {}
    for k in ('plain_one_pass', 'features_one_call'):       # where the difference sits: the library's per-stage events (the feature blends are timed with K10 / K11)
        be.profile_enable(True)
        be.profile_read()
        for i in range(len(passes)):
            run(k, i)
        torch.cuda.synchronize()
        stages[k] = {name: round(ms / len(passes), 4) for name, (ms, calls) in be.profile_read().items() if calls}
        be.profile_enable(False)
    result['stage_ms_per_pass'] = stages
    result['feature_forward_blend_ms'] = stages['features_one_call']['blend_forward'] - stages['plain_one_pass']['blend_forward']
    result['feature_backward_blend_ms'] = stages['features_one_call']['blend_backward'] - stages['plain_one_pass']['blend_backward']
    print(f'feature forward blend {result["feature_forward_blend_ms"]:.3f} ms, feature backward blend {result["feature_backward_blend_ms"]:.3f} ms '
          f'(blend_forward / blend_backward stage, one call minus plain pass)', flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
