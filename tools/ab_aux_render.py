"""What do the auxiliary maps of the forward-only render cost? fgs_inference against fgs_inference_aux (all three maps; expected depth alone) in ONE
process, alternating, on S2 and on the layered S2 (opacity logits - 3: deep lists, the blend-bound regime). Every timed block is `--reps` renders over the
orbit views between two HIP events on the stream, after a warm-up; the variants take turns inside every round, so drift of the box hits all of them alike;
reported: the median over the rounds of ms per render (and min / max). `--parent-library <libfgs_hip.so of the parent commit>` adds that library's fgs_inference
to the rotation: the yardstick for 'plain inference did not move' is measured in the same session on the same box (README: +-2 % between boxes).
Writes profiles/aux_render_ab.json (or --out). The overhead of the aux variant is recorded, not gated."""
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
    ap.add_argument('--reps', type=int, default=12, help='passes over the views per timed block')
    ap.add_argument('--warmup', type=int, default=2, help='untimed passes over the views per variant')
    ap.add_argument('--n-gaussians', type=int, default=0, help='override the S2 size (debug)')
    ap.add_argument('--parent-library', default='', help="the parent commit's libfgs_hip.so: its fgs_inference joins the rotation")
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'aux_render_ab.json'))
    args = ap.parse_args()

    import bench
    from FasterGSCudaBackend import _lib
    from FasterGSCudaBackend._backend import Backend, default_backend
    from harness import trainer as T
    argv, sys.argv = sys.argv, ['bench.py'] + (['--n-gaussians', str(args.n_gaussians)] if args.n_gaussians else [])
    params, views, what = bench.build_scene(bench.parse())
    sys.argv = argv
    dev = torch.device('cuda:0')
    be = default_backend()
    parent = None
    if args.parent_library:          # bound by hand: it does not export the new entry point, so _lib.bind would refuse it
        import ctypes
        plib = ctypes.CDLL(args.parent_library)
        for fname in ('fgs_inference', 'fgs_last_error', 'fgs_build_info'):
            getattr(plib, fname).restype, getattr(plib, fname).argtypes = _lib._SIGNATURES[fname]
        parent = Backend(plib)
    layered = dict(params)
    layered['opacities'] = params['opacities'] - 3.0
    result = {'what': 'ms per forward-only render (all stages, 1920x1080), median over alternating rounds of HIP-event-timed blocks',
              'scene': what, 'device': torch.cuda.get_device_name(dev), 'box': os.uname().nodename, 'library': be.lib.fgs_build_info().decode(),
              'rounds': args.rounds, 'renders_per_block': args.reps * len(views), 'scenes': {}}
    for name, p in (('S2', params), ('layered S2', layered)):
        g = T.Gaussians(p, dev)
        P = g.tensors()
        S = [T.extract_settings(v.to(dev), g.active_sh_bases, v.to(dev).background_color) for v in views]
        variants = {'fgs_inference': lambda s: be.inference(*P, s, True, True),
                    'fgs_inference_aux (alpha + expected + median)': lambda s: be.inference_aux(*P, s, True, True, True, True, True),
                    'fgs_inference_aux (expected depth alone)': lambda s: be.inference_aux(*P, s, True, True, False, True, False)}
        if parent is not None:
            variants['fgs_inference of the parent library'] = lambda s: parent.inference(*P, s, True, True)
        # The new entry point must not change a pixel (and the parent library renders the same image) -- up to what two passes of the SAME entry point
        # differ by: Gaussians with equal depth keys keep the run-to-run varying order of K1's atomic compaction (tools/forward_repeatability.py: some
        # twenty pixels by 6e-8 on the layered scene, none on S2). Recorded beside the times.
        first = be.inference(*P, S[0], True, True)
        differ = lambda img: {'pixels': int((img != first).any(dim=0).sum()), 'max_abs': float((img - first).abs().max())}
        same = {'fgs_inference repeated': differ(be.inference(*P, S[0], True, True)), 'fgs_inference_aux': differ(be.inference_aux(*P, S[0], True, True)['rgb'])}
        if parent is not None:
            same['fgs_inference of the parent library'] = differ(parent.inference(*P, S[0], True, True))
        print(f'{name:11s} image against a first fgs_inference pass: {same}', flush=True)
        assert all(d['max_abs'] <= 1e-6 for d in same.values()), same
        assert same['fgs_inference repeated']['pixels'] > 0 or all(d['pixels'] == 0 for d in same.values()), same      # repeatable scene: bit-identical
        for fn in variants.values():
            for _ in range(args.warmup):
                for s in S:
                    fn(s)
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        order = list(variants)
        for rnd in range(args.rounds):
            for k in order[rnd % len(order):] + order[:rnd % len(order)]:          # the turn order rotates as well
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.reps):
                    for s in S:
                        variants[k](s)
                stop.record()
                stop.synchronize()
                times[k].append(start.elapsed_time(stop) / (args.reps * len(S)))
        base = statistics.median(times['fgs_inference'])
        entry = {k: {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v), 'ratio_to_fgs_inference': statistics.median(v) / base,
                     'ms_rounds': [round(x, 4) for x in v]} for k, v in times.items()}
        result['scenes'][name] = entry
        result.setdefault('image_against_a_first_fgs_inference_pass', {})[name] = same
        for k, e in entry.items():
            print(f'{name:11s} {k:48s} {e["ms_median"]:.4f} ms (min {e["ms_min"]:.4f}, max {e["ms_max"]:.4f})  x{e["ratio_to_fgs_inference"]:.4f}', flush=True)
        del g, P, S, variants
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
