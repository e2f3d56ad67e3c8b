"""Which share of the blocks of 64 Gaussians still has zero Adam moments? (MI355X.) bench.py's own sequence on its scene -- one setup iteration per orbit view,
the warm-up, the timed steps -- through harness.trainer.training_iteration; after every iteration the optimizer's quiet-block flags (FusedAdam.quiet_blocks:
1 = both moments of the block are zero in every group) are read from the device. q = the share of blocks that are NOT quiet is what the optimizer kernel's
byte model charges 1416 bytes per Gaussian for; the flags are held against a scan of the moments at the end.
usage: python tools/quiet_share.py [--scene S2] [--opacity-shift -3] [--warmup 3] [--steps 20]"""
import argparse
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / 'faster-gaussian-splatting_amd')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scene', default='S2', choices=['S1', 'S2', 'S3'])
    ap.add_argument('--opacity-shift', type=float, default=0.0, help='-3 = the layered regime of bench.py --full')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
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
    views = [v.to(dev) for v in orbit_views(8)]
    with torch.no_grad():                                           # bench.py's targets: renders of a perturbed copy of the scene
        gen = torch.Generator(device='cpu').manual_seed(99)
        pert = [t.detach().clone() for t in g.tensors()]
        pert[4] = pert[4] + 0.15 * torch.randn(pert[4].shape, generator=gen).to(dev)
        pert[0] = pert[0] + 0.002 * torch.randn(pert[0].shape, generator=gen).to(dev)
        targets = [be.inference(*pert, T.extract_settings(v, g.active_sh_bases, v.background_color), True, True) for v in views]
        del pert
    tag = f'{args.scene} shift {args.opacity_shift:+g}'
    sequence = [('setup', i) for i in range(len(views))] + [('warm-up', i) for i in range(args.warmup)] + [('timed', args.warmup + 4 + i) for i in range(args.steps)]
    for k, (phase, i) in enumerate(sequence):
        T.training_iteration(g, views[i % len(views)], targets[i % len(views)], i)
        quiet = g.optimizer.quiet_blocks()
        if quiet is None:
            print(f'{tag} iteration {k} ({phase}, view {i % len(views)}): the step used no quiet flags')
            continue
        nb, nq = quiet.numel(), int(quiet.sum())
        print(f'{tag} iteration {k} ({phase}, view {i % len(views)}): blocks {nb}  quiet {nq} = {nq / nb:.4f}  not quiet q = {1 - nq / nb:.4f}')
    names = T.PARAM_ORDER
    state = [g.optimizer.state[getattr(g, k)] for k in names]
    scan = be.adam_quiet_scan([s['exp_avg'] for s in state], [s['exp_avg_sq'] for s in state])
    quiet = g.optimizer.quiet_blocks()
    stale, missed = int((quiet > scan).sum()), int((quiet < scan).sum())
    print(f'{tag} end: flags against a scan of the moments: flagged quiet with a non-zero moment {stale} (must be 0), zero moments without the flag {missed}')
    assert stale == 0


if __name__ == '__main__':
    main()
