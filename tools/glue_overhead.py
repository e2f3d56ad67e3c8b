"""Host time of the torch glue for one training iteration, without a GPU and without the library.

`Backend` gets a stand-in handle whose every entry returns 0 at once (the `*_bytes` entries therefore size every scratch to nothing), so what is
timed is the Python between the caller and the C ABI: parameter checks, Settings, the resize callback, pointer arrays, ForwardState. One iteration is
forward, l1_dssim, backward with both flag arrays and adam_step_multi over six groups with both flag arrays, on CPU tensors at N = 65.

    python tools/glue_overhead.py [path/to/_backend.py] [--runs 7] [--iterations 2000]

The module file is an argument so that another revision's file (git show <rev>:faster-gaussian-splatting_amd/FasterGSCudaBackend/_backend.py > file)
is timed by the same script; run the two alternately in one shell call on an otherwise idle machine and compare medians against the min .. max spread.
"""
import argparse
import importlib.util
import statistics
import sys
import time
import types
from pathlib import Path

import torch

PKG = Path(__file__).resolve().parent.parent / 'faster-gaussian-splatting_amd'
sys.path.insert(0, str(PKG))


class NullLibrary:
    """Every entry of the C ABI: returns 0 (success, zero bytes) and touches nothing."""

    def __getattr__(self, name):
        return lambda *args: 0


def load_glue(path: Path):
    """The module in `path` as a member of a bare FasterGSCudaBackend package (its `from . import _lib` resolves; nothing is dlopened)."""
    if 'FasterGSCudaBackend' not in sys.modules:
        package = types.ModuleType('FasterGSCudaBackend')
        package.__path__ = [str(PKG / 'FasterGSCudaBackend')]
        sys.modules['FasterGSCudaBackend'] = package
    spec = importlib.util.spec_from_file_location('FasterGSCudaBackend._glue_under_test', path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    return module


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('module', nargs='?', default=str(PKG / 'FasterGSCudaBackend' / '_backend.py'))
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--iterations', type=int, default=2000)
    args = ap.parse_args()
    glue = load_glue(Path(args.module))
    be = glue.Backend(NullLibrary())

    n, blocks = 65, 2
    gen = torch.Generator().manual_seed(0)
    rows = {'means': (3,), 'scales': (3,), 'rotations': (4,), 'opacities': (1,), 'sh0': (1, 3), 'sh_rest': (15, 3)}
    p = {k: torch.randn((n,) + r, generator=gen) for k, r in rows.items()}
    w2c = torch.eye(4)
    settings = glue.RasterizerSettings(w2c, torch.zeros(3), torch.zeros(3), 16, 48, 36, 40.0, 40.0, 24.0, 18.0, 0.2, 1e4, False)
    target, grad_image = torch.rand(3, 36, 48, generator=gen), torch.rand(3, 36, 48, generator=gen)
    dens = torch.zeros(2, n)
    live, reached, quiet = (torch.zeros(blocks, dtype=torch.uint8) for _ in range(3))
    order = ('means', 'sh0', 'sh_rest', 'opacities', 'scales', 'rotations')
    params = [p[k] for k in order]
    moments, second = [torch.zeros_like(t) for t in params], [torch.zeros_like(t) for t in params]
    steps, lrs = [1] * 6, [1e-3] * 6

    def iteration():
        res = be.forward(p['means'], p['scales'], p['rotations'], p['opacities'], p['sh0'], p['sh_rest'], settings)
        be.l1_dssim(res.image, target)
        grads = be.backward(dens, grad_image, res.image, p['means'], p['scales'], p['rotations'], p['opacities'], p['sh_rest'], res.buffers, settings,
                            res.state, live_blocks=live, reached_blocks=reached)
        by_name = dict(zip(('means', 'scales', 'rotations', 'opacities', 'sh0', 'sh_rest'), grads))
        be.adam_step_multi([by_name[k] for k in order], params, moments, second, steps, lrs, 0.9, 0.999, 1e-15, live_blocks=reached, quiet_blocks=quiet)

    for _ in range(200):
        iteration()
    runs = []
    for _ in range(args.runs):
        start = time.perf_counter()
        for _ in range(args.iterations):
            iteration()
        runs.append((time.perf_counter() - start) / args.iterations * 1e6)
    print(f'{args.module}: us per iteration, {args.runs} runs of {args.iterations}: ' + ' '.join(f'{r:.1f}' for r in runs)
          + f' | median {statistics.median(runs):.1f} min {min(runs):.1f} max {max(runs):.1f}')


if __name__ == '__main__':
    main()
