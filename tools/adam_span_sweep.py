"""K13's span length C (chunks of 1024 floats per workgroup, fgs_debug_set_option(15, C)) swept inside ONE process of the dev library. (MI355X.)
bench.py's own sequence on its scene through harness.trainer.training_iteration: one setup iteration per orbit view and the warm-up at the library's
default, then rounds of 8 iterations (one per view) at every C in turn, HIP events around the optimizer stage alone. Every C meets every view in every
round; the rounds come one after the other, so the slow growth of the non-quiet share over the run is spread over all C alike.
--spans 0 leaves the library as it was built (a library without the option, such as the parent's, is measured the same way). The option is put back to
the library's default before the process ends.
usage: python tools/adam_span_sweep.py [--scene S2] [--opacity-shift -3] [--warmup 3] [--rounds 3] [--spans 1 2 4 8 16 32]"""
import argparse
import os
import re
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / 'faster-gaussian-splatting_amd')]
os.environ.setdefault('FGS_HIP_LIBRARY', str(REPO / 'faster-gaussian-splatting_amd' / 'libfgs_hip_dev.so'))     # the dev library, or a variant of it

import torch  # noqa: E402

SPAN_OPTION = 15          # fgs_debug_set_option: chunks of 1024 floats per workgroup of K13
N_VIEWS = 8               # bench.py's orbit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scene', default='S2', choices=['S1', 'S2', 'S3'])
    ap.add_argument('--opacity-shift', type=float, default=0.0, help='-3 = the layered regime of bench.py --full')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--spans', type=int, nargs='+', default=[1, 2, 4, 8, 16, 32], help='0 = the library as built, no option set')
    args = ap.parse_args()
    from FasterGSCudaBackend._backend import default_backend
    from harness import trainer as T
    from harness.scenes import SCENE_SIZES, make_garden_like, orbit_views
    dev = torch.device('cuda:0')
    params = make_garden_like(SCENE_SIZES[args.scene])
    params['opacities'] = params['opacities'] + args.opacity_shift
    be = default_backend()
    g = T.Gaussians(params, dev)
    g.training_setup(training_cameras_extent=5.0)
    views = [v.to(dev) for v in orbit_views(N_VIEWS)]
    with torch.no_grad():                                           # bench.py's targets: renders of a perturbed copy of the scene
        gen = torch.Generator(device='cpu').manual_seed(99)
        pert = [t.detach().clone() for t in g.tensors()]
        pert[4] = pert[4] + 0.15 * torch.randn(pert[4].shape, generator=gen).to(dev)
        pert[0] = pert[0] + 0.002 * torch.randn(pert[0].shape, generator=gen).to(dev)
        targets = [be.inference(*pert, T.extract_settings(v, g.active_sh_bases, v.background_color), True, True) for v in views]
        del pert
    it = 0
    for _ in range(len(views) + args.warmup):
        T.training_iteration(g, views[it % N_VIEWS], targets[it % N_VIEWS], it)
        it += 1
    tag = f'{args.scene} shift {args.opacity_shift:+g}'
    times = {c: [] for c in args.spans}
    default = int(re.search(r'FGS_SWITCH\(g_adam_span,\s*(\d+)\)', (REPO / 'faster-gaussian-splatting_amd' / 'csrc' / 'fgs_kernels.h').read_text()).group(1))
    be.profile_enable(True, only='adam')
    try:
        for rnd in range(args.rounds):
            for c in args.spans:
                if c != 0:                                 # 0: the library as built, which may not have the option at all
                    assert be.lib.fgs_debug_set_option(SPAN_OPTION, c) == 0
                for _ in range(N_VIEWS):
                    torch.cuda.synchronize()
                    be.profile_read()
                    T.training_iteration(g, views[it % N_VIEWS], targets[it % N_VIEWS], it)
                    torch.cuda.synchronize()
                    total, calls = be.profile_read()['adam']
                    assert calls == 1
                    times[c].append(total)
                    it += 1
                quiet = g.optimizer.quiet_blocks()
                q = float('nan') if quiet is None else 1.0 - float(quiet.sum()) / quiet.numel()
                last = times[c][-N_VIEWS:]
                print(f'{tag} round {rnd} C {c:2d}: adam ms per launch over the views  mean {statistics.mean(last):.4f}  min {min(last):.4f}  max {max(last):.4f}  '
                      f'not quiet q = {q:.4f}', flush=True)
    finally:
        be.profile_enable(False)
        if any(args.spans):
            be.lib.fgs_debug_set_option(SPAN_OPTION, default)
    for c in args.spans:
        per_round = [statistics.mean(times[c][N_VIEWS * r:N_VIEWS * r + N_VIEWS]) for r in range(args.rounds)]
        print(f'{tag} C {c:2d}: mean of the rounds {statistics.mean(per_round):.4f} ms  rounds {" ".join(f"{x:.4f}" for x in per_round)}  '
              f'spread of the rounds {max(per_round) - min(per_round):.4f}', flush=True)


if __name__ == '__main__':
    main()
