"""How many VISIBLE Gaussians did the backward blend kernel never reach? (MI355X.) One forward + backward pass per view of bench.py's scene; afterwards the
nine-float accumulator records are read from the primitive blob: a visible Gaussian (n_touched != 0) whose record is still all +-0 is "unreached" -- the
backward gradients kernel skips it (csrc/preprocess_backward.hip: gaussian_backward). Also counted: blocks of 64 Gaussians that are visible without a
reached lane (their SH-rest gradient block is written as zeros without touching LDS), and, for the costed follow-up in DESIGN.md, the same blocks as a
share of all blocks (what a second flag array would let the optimizer skip).
usage: python tools/reached_share.py [--scene S2] [--opacity-shift -3] [--views 0 2 5]"""
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
    ap.add_argument('--views', type=int, nargs='*', default=[0, 2, 5])
    args = ap.parse_args()
    from FasterGSCudaBackend._backend import RasterizerSettings, default_backend
    from harness.scenes import SCENE_SIZES, make_garden_like, orbit_views
    dev = torch.device('cuda:0')
    n = SCENE_SIZES[args.scene]
    params = make_garden_like(n)
    params['opacities'] = params['opacities'] + args.opacity_shift
    names = ('means', 'scales', 'rotations', 'opacities', 'sh_coefficients_0', 'sh_coefficients_rest')
    p = {k: params[k].to(dev).contiguous() for k in names}
    be = default_backend()
    views = orbit_views(8)
    for vi in args.views:
        v = views[vi].to(dev)
        RS = RasterizerSettings(v.w2c, v.position, v.background_color, 16, v.width, v.height, v.focal_x, v.focal_y, v.center_x, v.center_y,
                                v.near_plane, v.far_plane, False)
        res = be.forward(*[p[k] for k in names], RS)
        gi = torch.where(res.image >= 0, 1.0, -1.0) / res.image.numel()     # dense like the gradient of the L1 + DSSIM loss: no pixel without one
        be.backward(None, gi, res.image, p['means'], p['scales'], p['rotations'], p['opacities'], p['sh_coefficients_rest'], res.buffers, RS, res.state)
        torch.cuda.synchronize()
        layout = be.blob_layout(0, n, v.width, v.height, res.state[1], res.state[2])
        acc = be.view(res.buffers[0], layout, 'acc', torch.float32)[:9 * n].reshape(n, 9)
        visible = be.view(res.buffers[0], layout, 'n_touched', torch.int32)[:n] != 0
        reached = visible & (acc.view(torch.int32) & 0x7fffffff != 0).any(dim=1)
        pad = (-n) % 64
        blocks = lambda m: torch.cat([m, m.new_zeros(pad)]).reshape(-1, 64).any(dim=1)
        vb, rb = blocks(visible), blocks(reached)
        V, Rn = int(visible.sum()), int(reached.sum())
        print(f'{args.scene} shift {args.opacity_shift:+g} view {vi}: N {n}  visible {V} ({V / n:.3f})  reached {Rn} = {Rn / max(V, 1):.3f} of the visible  '
              f'unreached {V - Rn} = {(V - Rn) / max(V, 1):.3f} of the visible | blocks of 64: {vb.numel()}  visible {int(vb.sum())}  '
              f'visible without a reached lane {int((vb & ~rb).sum())} = {int((vb & ~rb).sum()) / max(int(vb.sum()), 1):.3f} of the visible blocks, '
              f'{int((vb & ~rb).sum()) / vb.numel():.3f} of all blocks  | instances {res.state[1]}')
        del res


if __name__ == '__main__':
    main()
