"""Recipe: the reference's rasterizer, built for the CPU.  TEST INFRASTRUCTURE ONLY.

Takes the reference tree from $FGS_REFERENCE_TREE (default /root/reference), copies its torch-free CUDA host files into oracle/_ref/src/ with one
mechanical change -- `kernel<<<grid, block>>>(args)` becomes `cuda_on_cpu::launch(grid, block).run(kernel, args)` -- and compiles them with g++
against the stand-in headers of oracle/cuda_on_cpu/ (layered on the fiber emulator of tests/sim) and the reference's own include directories, by
path, together with the C-ABI driver oracle/ref_driver.cpp, into oracle/_ref/libfgs_ref_cpu.so. Everything under oracle/_ref/ is ignored by git:
the rewritten sources are reference text and live only there. Without a tree the recipe says so in one line and succeeds.

Arithmetic is "as written": -O2 -ffp-contract=off and the same libm as oracle/fgs_oracle.c -- not nvcc's FMA contraction, not NVIDIA's __expf.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
OUT = HERE / '_ref'
LIB = OUT / 'libfgs_ref_cpu.so'

HOST_FILES = ('rasterization/src/forward.cu', 'rasterization/src/backward.cu', 'rasterization/src/inference.cu',
              'rasterization/src/pruning_scores.cu', 'densification/src/mcmc.cu')
INCLUDE_DIRS = ('rasterization/include', 'densification/include', 'utils')
LAUNCH = re.compile(r'([A-Za-z_][\w:]*(?:<[\w:, ]+>)?)<<<(.+?)>>>\(')


def reference_tree() -> Path | None:
    root = Path(os.environ.get('FGS_REFERENCE_TREE', '/root/reference'))
    pkg = root / 'FasterGSCudaBackend' / 'FasterGSCudaBackend'
    return pkg if all((pkg / f).is_file() for f in HOST_FILES) else None


def rewrite_launches(text: str) -> tuple[str, int]:
    return LAUNCH.subn(lambda m: f'cuda_on_cpu::launch({m.group(2)}).run({m.group(1)}, ', text)


def _inputs(pkg: Path) -> list[Path]:
    own = [HERE / 'ref_driver.cpp', Path(__file__), REPO / 'tests' / 'sim' / 'include' / 'hip' / 'hip_runtime.h', *sorted((HERE / 'cuda_on_cpu').rglob('*.*'))]
    return own + [pkg / f for f in HOST_FILES] + [p for d in INCLUDE_DIRS for p in sorted((pkg / d).iterdir())]


def _flags(pkg: Path) -> list[str]:
    # -D__CUDACC__: helper_math.h then leaves fminf / fmaxf / min / max / rsqrtf to the headers it is compiled against, as under nvcc
    return ['-std=c++17', '-O2', '-ffp-contract=off', '-fPIC', '-w', '-D__CUDACC__', f'-I{HERE / "cuda_on_cpu"}', f'-I{REPO / "tests" / "sim" / "include"}',
            *[f'-I{pkg / d}' for d in INCLUDE_DIRS]]


def build_sanitized_program(sanitize: str = 'undefined') -> Path:
    """oracle/_ref/ref_driver_<sanitize>: the rewritten sources and the driver's stand-alone main (-DREF_DRIVER_MAIN) as ONE ordinary program built with
    -fsanitize=<sanitize> (findings are printed, the run goes on). Run it on a file written by oracle.reference.dump_scene. Needs build() to have written oracle/_ref/src (a reference tree)."""
    pkg = reference_tree()
    assert pkg is not None and build() is not None
    exe = OUT / f'ref_driver_{sanitize}'
    sources = [OUT / 'src' / (Path(f).stem + '.cpp') for f in HOST_FILES] + [HERE / 'ref_driver.cpp']
    subprocess.run(['g++', *_flags(pkg), '-g', '-O1', f'-fsanitize={sanitize}', '-DREF_DRIVER_MAIN', *map(str, sources), '-o', str(exe)], check=True)
    return exe


def build(force: bool = False) -> Path | None:
    """Returns the library's path, or None when there is no reference tree (and no library can be made)."""
    pkg = reference_tree()
    if pkg is None:
        print('oracle/build_ref.py: no reference tree (FGS_REFERENCE_TREE) -- the reference-on-CPU library is not built; the committed fixtures stand in')
        return LIB if LIB.exists() else None
    if not force and LIB.exists() and LIB.stat().st_mtime >= max(p.stat().st_mtime for p in _inputs(pkg)):
        return LIB
    src = OUT / 'src'
    src.mkdir(parents=True, exist_ok=True)
    sources = []
    for f in HOST_FILES:
        text, n = rewrite_launches((pkg / f).read_text())
        assert n > 0 and '<<<' not in text, f'{f}: launch syntax left after the rewrite'
        dst = src / (Path(f).stem + '.cpp')
        dst.write_text(text)
        sources.append(dst)
    flags = _flags(pkg)
    objs = []
    procs = []
    for s in [*sources, HERE / 'ref_driver.cpp']:
        o = OUT / (s.stem + '.o')
        objs.append(o)
        procs.append(subprocess.Popen(['g++', *flags, '-c', str(s), '-o', str(o)]))
    if any(p.wait() != 0 for p in procs):
        raise RuntimeError('oracle/build_ref.py: the reference does not compile against oracle/cuda_on_cpu')
    subprocess.run(['g++', '-shared', '-o', str(LIB), *map(str, objs)], check=True)
    return LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv)
    if '--ubsan-program' in sys.argv:
        print(build_sanitized_program('undefined'))
